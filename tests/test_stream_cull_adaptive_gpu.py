"""Culled streamed adaptive passes on the GPU (csrc/rt_stream_cull_adaptive.hip).  Results are unchanged by
definition, so every frame and refined count here is compared three ways: with the same context without RT_FLAG_STREAM_CULL, bit for
bit; for degree <= 2 with the CPU oracle's composition; at tau < 0 with the RT_FLAG_STREAM | RT_FLAG_SSAAk frame.  `culled` is
RT_FLAG_STREAM | RT_FLAG_SSAAk | RT_FLAG_SSAA_ADAPTIVE | RT_FLAG_STREAM_ADAPTIVE | RT_FLAG_STREAM_CULL.  The conditions that keep these
tests from being vacuous, and the wave cone itself, are held on the CPU in tests/test_stream_cull_adaptive_host.py, for the very cases
of tests/tools/stream_cull_adaptive_scenes.py used here."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, compare, scene_path
from test_ssaa_adaptive_fuzz_gpu import identical, mismatch
from test_ssaa_adaptive_gpu import ada_flags, kflag

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ssaa_adaptive_ref as ada  # noqa: E402
import ssaa_geometry_ref as geo  # noqa: E402
import ssaa_ref  # noqa: E402
import stream_adaptive_scenes as A  # noqa: E402
import stream_cull_adaptive_scenes as CA  # noqa: E402
import stream_cull_lab as SC  # noqa: E402
import stream_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu

F32, U8, INF, TAU = CA.F32, CA.U8, CA.INF, CA.TAU


def unculled(pkg, k, extra=0):
    return pkg.RT_FLAG_STREAM | ada_flags(pkg, k, pkg.RT_FLAG_STREAM_ADAPTIVE | extra)


def culled(pkg, k, extra=0):
    return unculled(pkg, k, extra) | pkg.RT_FLAG_STREAM_CULL


def want_of(out, fmt):
    return ssaa_ref.quantise(out) if fmt == U8 else out


def frames_of(pkg, sc, cam, flags, fmt, taus, decision, coses=(None,), **kw):
    """{(tau, min_cos): (frame, refined)} from ONE context whose stream-cull-adaptive decision must be `decision`."""
    r = pkg.Renderer(sc, device=0, flags=flags, fmt=fmt, **kw)
    out = {}
    try:
        assert r.stream_cull_adaptive is decision and r.streamed_adaptive, (r.stream_cull_adaptive, r.stream_cull, r.streamed_adaptive)
        for tau in taus:
            for c in coses:
                r.set_ssaa_threshold(tau)
                if c is not None:
                    r.set_ssaa_geometry(c)
                r.update(cam)
                out[(tau, c)] = (r.download().copy(), r.refined)
    finally:
        r.cleanup_update()
    return out


def plain(pkg, sc, cam, flags, fmt=F32):
    r = pkg.Renderer(sc, device=0, flags=flags, fmt=fmt)
    try:
        r.update(cam)
        return r.download().copy()
    finally:
        r.cleanup_update()


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CA.SCENES, ids=[" ".join(str(v) for v in key) for key in CA.SCENES])
def test_scenes(pkg, key):
    """k = 2 and 4, both formats, tau in {-1, 0, 1/32, +inf}."""
    sc, cam = CA.scene(pkg, key)
    p = CA.frame(key)
    for k in (2, 4):
        s = CA.frame(key, k)
        for fmt in (F32, U8):
            got = frames_of(pkg, sc, cam, culled(pkg, k), fmt, CA.TAUS, True)
            ref = frames_of(pkg, sc, cam, unculled(pkg, k), fmt, CA.TAUS, False)
            for tau in CA.TAUS:
                frame, n = got[(tau, None)]
                assert identical(frame, ref[(tau, None)][0]) and n == ref[(tau, None)][1], (key, k, fmt, tau, mismatch(frame, ref[(tau, None)][0]))
                want = want_of(ada.compose(p, s, k, tau), fmt)
                assert identical(frame, want), (key, k, fmt, tau, mismatch(frame, want))
                assert n == int(ada.refine_mask(p, tau).sum()), (key, k, fmt, tau, n)
            full = plain(pkg, sc, cam, pkg.RT_FLAG_STREAM | kflag(pkg, k), fmt)
            assert identical(got[(-1.0, None)][0], full), (key, k, fmt, mismatch(got[(-1.0, None)][0], full))


def cubic_and_field(pkg, w, h, with_quadric):
    """A shipped degree-3 scene enlarged by the 65-sphere field (two chunks) -- and, with_quadric, by one ellipsoid with cross terms, so
    that the kernel for general quadrics AND degree 3 runs."""
    sc = pkg.Scene.load_from_file(scene_path("clebsch")).set_size(w, h)
    a = S.field(pkg, 65, S.FIELD_SEED, w=w, h=h, mirrors=True, depth=1).arrays()
    for i in range(len(a["reflection"])):
        sc.add_object(a["coefs"][i], a["albedo"][i], float(a["reflection"][i]))
    if with_quadric:
        sc.add_object(S.ellipsoid(np.array([3.0, 2.0, 18.0]), np.array([1.5, 0.8, 1.1]), np.array([0.3, -0.2, 0.1])), (0.9, 0.6, 0.3), 0.3)
    return sc


@pytest.mark.parametrize("with_quadric", [False, True], ids=["cubic", "cubic+quadric"])
def test_cubic_scene_with_a_field(pkg, with_quadric):
    """Degree 3 is held to the library's own frames: the unculled context, and at tau < 0 the RT_FLAG_STREAM | RT_FLAG_SSAAk frame."""
    w, h = 48, 36
    sc = cubic_and_field(pkg, w, h, with_quadric)
    for k, fmt in ((2, U8), (4, F32)):
        got = frames_of(pkg, sc, None, culled(pkg, k), fmt, (-1.0, TAU), True)
        ref = frames_of(pkg, sc, None, unculled(pkg, k), fmt, (-1.0, TAU), False)
        for tau in (-1.0, TAU):
            assert identical(got[(tau, None)][0], ref[(tau, None)][0]) and got[(tau, None)][1] == ref[(tau, None)][1], (k, tau, mismatch(got[(tau, None)][0], ref[(tau, None)][0]))
        assert 0 < got[(TAU, None)][1] < w * h == got[(-1.0, None)][1]
        assert identical(got[(-1.0, None)][0], plain(pkg, sc, None, pkg.RT_FLAG_STREAM | kflag(pkg, k), fmt))


def test_geometry(pkg):
    """RT_FLAG_SSAA_GEOMETRY at min_cos -inf and 0.9: the G pass and the classifier are untouched, the refine pass culls."""
    key = CA.GEOMETRY
    sc, cam = A.scene(pkg, key)
    p = A.frame(key)
    obj, nrm = A.planes(key)
    g = pkg.RT_FLAG_SSAA_GEOMETRY
    for k, fmt in ((2, F32), (4, U8)):
        s = A.frame(key, k)
        got = frames_of(pkg, sc, cam, culled(pkg, k, g), fmt, (TAU, INF), True, coses=CA.GEO_COSES)
        ref = frames_of(pkg, sc, cam, unculled(pkg, k, g), fmt, (TAU, INF), False, coses=CA.GEO_COSES)
        for tau in (TAU, INF):
            for c in CA.GEO_COSES:
                frame, n = got[(tau, c)]
                assert identical(frame, ref[(tau, c)][0]) and n == ref[(tau, c)][1], (k, tau, c)
                want = want_of(geo.compose(p, s, k, tau, obj, nrm, c), fmt)
                assert identical(frame, want), (k, tau, c, mismatch(frame, want))
                assert n == int((ada.refine_mask(p, tau) | geo.geo_mask(obj, nrm, c)).sum())


# ---- 2. bands ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CA.BANDS, ids=[f"world{c[1]}-band{c[2]}" for c in CA.BANDS])
def test_bands(pkg, case):
    """Every rank's rows equal the single context's, the unculled rank's and the oracle's: the K = 1 halo kernel with waves that straddle
    two halo slots and with off-image halo rows."""
    key, world, band, k, fmt = case
    sc, cam = A.scene(pkg, key)
    p, s = A.frame(key), A.frame(key, k)
    h = p.shape[0]
    for tau in (0.0, TAU):
        want = want_of(ada.compose(p, s, k, tau), fmt)
        mask = ada.refine_mask(p, tau)
        single, n = frames_of(pkg, sc, cam, culled(pkg, k), fmt, (tau,), True)[(tau, None)]
        assert identical(single, want) and n == int(mask.sum()), (tau, mismatch(single, want))
        seen = np.zeros(h, dtype=bool)
        for rank in range(world):
            rows = pkg.band_rows_of_rank(h, band, world, rank)
            kw = dict(rank=rank, world=world, band_rows=band)
            got, n = frames_of(pkg, sc, cam, culled(pkg, k), fmt, (tau,), True, **kw)[(tau, None)]
            ref, m = frames_of(pkg, sc, cam, unculled(pkg, k), fmt, (tau,), False, **kw)[(tau, None)]
            assert got.shape[0] == len(rows) and identical(got, ref) and n == m, (rank, tau, mismatch(got, ref))
            assert identical(got, single[rows]) and identical(got, want[rows]), (rank, tau, mismatch(got, want[rows]))
            assert n == int(mask[rows].sum()), (rank, tau, n)
            seen[rows] = True
        assert seen.all()


# ---- 3. RT_FLAG_FAST ---------------------------------------------------------------------------------------------------------------------------
def test_fast_variant(pkg):
    """Bit for bit the unculled FAST context (the same arithmetic per tested object), and 1e-5 relative against strict, at most
    max(3, 0.2 % of the pixels) beyond it."""
    for key, k in ((CA.FIELDS[3], 4), (CA.MIXED, 2)):
        sc, cam = CA.scene(pkg, key)
        f = pkg.RT_FLAG_FAST
        fast = frames_of(pkg, sc, cam, culled(pkg, k, f), F32, (-1.0, TAU), True)
        ref = frames_of(pkg, sc, cam, unculled(pkg, k, f), F32, (-1.0, TAU), False)
        for tau in (-1.0, TAU):
            assert identical(fast[(tau, None)][0], ref[(tau, None)][0]) and fast[(tau, None)][1] == ref[(tau, None)][1], (key, tau)
        strict = frames_of(pkg, sc, cam, culled(pkg, k), F32, (-1.0,), True)[(-1.0, None)][0]
        h, w = strict.shape[:2]
        c = compare(fast[(-1.0, None)][0][..., :3], strict[..., :3])
        print("FAST against strict:", key, k, c)
        assert fast[(-1.0, None)][1] == w * h and c["n_bad_pixels"] <= max(3, int(0.002 * w * h)), (key, c)


# ---- 4. the decision -----------------------------------------------------------------------------------------------------------------------------
def test_decision_false_is_the_context_as_it_is_today(pkg, monkeypatch):
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    f = pkg
    key = CA.FIELDS[2]
    sc, cam = CA.scene(pkg, key)
    one_chunk, _ = A.scene(pkg, ("field", "sphere", 64, 64, 48, True, 4, 2.6))
    small = ada_flags(pkg, 2, f.RT_FLAG_STREAM_ADAPTIVE)
    # (scene, flags, the same context without what the pull request reads, rt_get_stream_cull, rt_get_streamed_adaptive)
    cases = [(sc, culled(pkg, 2, f.RT_FLAG_NOCULL), unculled(pkg, 2, f.RT_FLAG_NOCULL), False, True),
             (one_chunk, culled(pkg, 2), unculled(pkg, 2), True, True),
             (sc, small | f.RT_FLAG_STREAM_CULL, small, False, False),
             (sc, unculled(pkg, 2), unculled(pkg, 2), False, True)]
    for i, (scene, flags, same, cull, streamed_adaptive) in enumerate(cases):
        r, q = pkg.Renderer(scene, device=0, flags=flags, ssaa_threshold=TAU), pkg.Renderer(scene, device=0, flags=same, ssaa_threshold=TAU)
        try:
            assert r.stream_cull_adaptive is False and r.stream_cull is cull and r.streamed_adaptive is streamed_adaptive, i
            with pytest.raises(pkg.RtError) as e:
                r.stream_cull_adaptive_stats()
            assert e.value.code == -1 and "rt_debug_stream_cull_adaptive" in e.value.message, i
            for _ in range(2):
                r.update(cam)
                q.update(cam)
            assert identical(r.download(), q.download()) and r.refined == q.refined > 0, i
        finally:
            r.cleanup_update()
            q.cleanup_update()


def test_without_the_environment_switch_there_are_no_work_words(pkg, monkeypatch):
    monkeypatch.delenv("MI355RT_STREAM_CULL_STATS", raising=False)
    sc, cam = CA.scene(pkg, CA.FIELDS[2])
    r = pkg.Renderer(sc, device=0, flags=culled(pkg, 2), ssaa_threshold=TAU)
    try:
        assert r.stream_cull_adaptive is True
        r.update(cam)
        with pytest.raises(pkg.RtError) as e:
            r.stream_cull_adaptive_stats()
        assert e.value.code == -1 and "rt_debug_stream_cull_adaptive" in e.value.message
    finally:
        r.cleanup_update()


# ---- 5. statistics ---------------------------------------------------------------------------------------------------------------------------------
def test_statistics(pkg, monkeypatch):
    """The cluster scene, k = 4, tau = -1: every pixel is listed in whole-block runs of 64, so a wave is four pixels of one block and every
    ray is proven.  [0] == D0 exactly; [0] - [1] >= L; [1] >= the (wave, chunk) pairs with a primary hit; fewer shadow entries swept than
    decided; nothing ran unculled or without a cone; the plain pass's words are the plain pass's alone; a second frame doubles every word."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    e = CA.stats_expectation()
    assert e["L"] >= e["D0"] / 4
    sc, _ = CA.scene(pkg, CA.CLUSTER)
    r = pkg.Renderer(sc, device=0, flags=culled(pkg, 4), ssaa_threshold=-1.0)
    only_plain = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL)
    try:
        assert r.stream_cull_adaptive is True and r.stream_cull_adaptive_stats() == [0] * 8
        r.update()
        only_plain.update()
        w = r.stream_cull_adaptive_stats()
        print("work words", w, "expected", e)
        assert r.refined == 64 * 48
        assert w[0] == e["D0"] == (64 * 48 * 16 // 64) * e["n_chunks"]
        assert w[7] == 0
        assert w[0] - w[1] >= e["L"]
        assert w[1] >= e["H"]
        assert w[5] < w[4] <= 64 * w[3]
        assert w[6] == 0
        assert r.stream_cull_stats() == only_plain.stream_cull_stats() and r.stream_cull_stats()[0] > 0
        assert identical(r.download(), ada.compose(CA.frame(CA.CLUSTER), CA.frame(CA.CLUSTER, 4), 4, -1.0))
        r.update()
        assert r.stream_cull_adaptive_stats() == [2 * x for x in w]   # cumulative
    finally:
        r.cleanup_update()
        only_plain.cleanup_update()


# ---- 6. scene updates and graphs -------------------------------------------------------------------------------------------------------------
def test_set_scene_clusters_exchange_places(pkg):
    sc, moved = CA.scene(pkg, CA.CLUSTER)[0], CA.scene(pkg, ("cluster", True))[0]
    coefs = moved.arrays()["coefs"]
    r = pkg.Renderer(sc, device=0, flags=culled(pkg, 2), ssaa_threshold=TAU)
    try:
        assert r.stream_cull_adaptive is True
        r.update()
        before = r.download().copy()
        r.set_scene(coefs=coefs)
        r.update()
        after, n = r.download().copy(), r.refined
        assert r.set_scene_status()["applied"] == 1
    finally:
        r.cleanup_update()
    fresh = frames_of(pkg, moved, None, culled(pkg, 2), F32, (TAU,), True)[(TAU, None)]
    assert not identical(after, before) and identical(after, fresh[0]) and n == fresh[1] > 0
    want = ada.compose(CA.frame(("cluster", True)), CA.frame(("cluster", True), 2), 2, TAU)
    assert identical(after, want), mismatch(after, want)


def test_set_scene_and_frame_in_one_graph_replayed_twice(pkg):
    """... with a threshold change between the replays: the graph keeps the tau it was captured with."""
    import torch
    sc, moved = CA.scene(pkg, CA.CLUSTER)[0], CA.scene(pkg, ("cluster", True))[0]
    steps = [moved.arrays()["coefs"], sc.arrays()["coefs"]]
    want = [frames_of(pkg, x, None, culled(pkg, 2), F32, (TAU,), True)[(TAU, None)][0] for x in (moved, sc)]
    assert not identical(want[0], want[1])
    r = pkg.Renderer(sc, device=0, flags=culled(pkg, 2), ssaa_threshold=TAU)
    s = torch.cuda.Stream()
    g = None
    try:
        r.update(stream=s.cuda_stream, timed=False)
        with torch.cuda.stream(s):
            arr = torch.from_numpy(steps[0].copy()).to("cuda:0")
            buf = torch.empty((r.local_rows, r.width, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            r.set_scene_into(coefs=arr.data_ptr(), stream=s.cuda_stream)
            r.update(dev_fb=buf.data_ptr(), stream=s.cuda_stream, timed=False)
        for rep in range(2):
            with torch.cuda.stream(s):
                arr.copy_(torch.from_numpy(steps[rep].copy()))
                buf.view(torch.int32).fill_(0x7FC00000)
                g.replay()
            s.synchronize()
            assert identical(buf.cpu().numpy(), want[rep]), rep
            r.set_ssaa_threshold(-1.0)
        assert r.set_scene_status()["applied"] == 2
    finally:
        torch.cuda.synchronize()
        del g
        r.cleanup_update()


# ---- 7. the multi-GPU layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", ["one device twice", "two devices"])
@pytest.mark.parametrize("transport", ["dense", "sparse"])
def test_multi_renderer(pkg, transport, devices):
    import torch
    if devices == "two devices" and torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    key = CA.FIELDS[3]
    sc, cam = CA.scene(pkg, key)
    extra = pkg.RT_MULTI_SPARSE if transport == "sparse" else 0
    single = frames_of(pkg, sc, cam, culled(pkg, 2), F32, (0.0, TAU), True)
    m = pkg.MultiRenderer(sc, [0, 0] if devices == "one device twice" else [0, 1], band_rows=8, parts=2, flags=culled(pkg, 2) | extra)
    try:
        for tau in (TAU, 0.0):
            m.set_ssaa_threshold(tau)
            for _ in range(2):
                m.update()
            got = m.download()
            assert identical(got, single[(tau, None)][0]), (transport, tau, mismatch(got, single[(tau, None)][0]))
    finally:
        m.cleanup_update()


# ---- 8. init_update() / update() ------------------------------------------------------------------------------------------------------------
ADAPTER = r"""
import ctypes as C, os, re, subprocess, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "tools"))
import __graft_entry__ as g
import ssaa_adaptive_ref as ada
import stream_cull_adaptive_scenes as CA
pkg = g.load_package()
key = CA.FIELDS[3]
sc, cam = CA.scene(pkg, key)
want = ada.compose(CA.frame(key), CA.frame(key, 4), 4, CA.TAU)
a = sc.arrays()
upd = C.CDLL(pkg.UPDATE_LIB_PATH)
names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
update = getattr(upd, re.search(r"\b(_Z\d+updateRKN3glm3matI\S*)\b", names).group(1))
cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
update.argtypes, update.restype = [C.c_void_p], C.c_float
upd.mi355rt_update_download.argtypes = [C.c_void_p, C.c_size_t]
cam = np.ascontiguousarray(pkg.IDENTITY if cam is None else cam, dtype=np.float64)
init(7, sc._h)
ms = update(cam.ctypes.data)
out = np.zeros((a["height"], a["width"], 4), np.float32)
rc = upd.mi355rt_update_download(out.ctypes.data_as(C.c_void_p), out.nbytes)
cleanup()
mask = ada.refine_mask(CA.frame(key), CA.TAU)
print("frame", rc, ms > 0.0, bool(np.array_equal(out.view(np.uint32), want.view(np.uint32))), bool(mask.any() and not mask.all()))
"""


def test_init_update_with_the_environment_switches():
    """The reference's back-end contract (ctypes on libmi355rt_update.so, a fresh process) on the 193-sphere field."""
    env = dict(os.environ, MI355RT_STREAM="1", MI355RT_STREAM_CULL="1", MI355RT_STREAM_ADAPTIVE="1", MI355RT_SSAA="4", MI355RT_SSAA_ADAPTIVE="0.03125")
    out = subprocess.run([sys.executable, "-c", ADAPTER, ROOT], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "frame 0 True True True", out.stdout
