"""Streamed adaptive supersampling on the GPU (RT_FLAG_STREAM_ADAPTIVE; csrc/rt_stream_adaptive.hip).  The
reference is the CPU oracle's composition (ssaa_adaptive_ref / ssaa_geometry_ref on the oracle's frames and planes), bit for bit, for
strict contexts and surfaces of degree <= 2 in both formats, and the context without the flag wherever rt_create accepts that one;
degree 3 is held to the library's own streamed frames, RT_FLAG_FAST to the project's 1e-5 bar.  `forced` is RT_FLAG_STREAM |
RT_FLAG_SSAAk | RT_FLAG_SSAA_ADAPTIVE | RT_FLAG_STREAM_ADAPTIVE: the streamed passes on a scene of any size.  The conditions that keep
these tests from being vacuous are asserted on the oracle alone in tests/test_stream_adaptive_host.py, for the very cases of
tests/tools/stream_adaptive_scenes.py used here."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, compare, scene_path
from test_gpu_parity import random_cubic_scene
from test_ssaa_adaptive_fuzz_gpu import identical, mismatch
from test_ssaa_adaptive_gpu import ada_flags, kflag

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ssaa_adaptive_ref as ada  # noqa: E402
import ssaa_geometry_ref as geo  # noqa: E402
import ssaa_ref  # noqa: E402
import stream_adaptive_scenes as A  # noqa: E402

pytestmark = pytest.mark.gpu

F32, U8, INF, TAU = A.F32, A.U8, A.INF, A.TAU


def forced(pkg, k, extra=0):
    return pkg.RT_FLAG_STREAM | ada_flags(pkg, k, pkg.RT_FLAG_STREAM_ADAPTIVE | extra)


def want_of(out, fmt):
    return ssaa_ref.quantise(out) if fmt == U8 else out


def frames_of(pkg, sc, cam, flags, fmt, taus, streamed_adaptive, streamed=None, coses=(None,), **kw):
    """{(tau, min_cos): (frame, refined)} from ONE context; where rt_create refuses it, the RtError itself."""
    try:
        r = pkg.Renderer(sc, device=0, flags=flags, fmt=fmt, **kw)
    except pkg.RtError as e:
        return e
    out = {}
    try:
        assert r.streamed_adaptive is streamed_adaptive and (streamed is None or r.streamed is streamed)
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


# ---- 1. forced, chunk boundaries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", A.FORCED, ids=[" ".join(str(v) for v in key) for key in A.FORCED])
def test_forced_chunk_boundaries(pkg, key):
    """k = 2 and 4, both formats, tau in {-1, 0, 1/32, +inf}: the oracle's composition, the refined count, and the frame of the context
    without RT_FLAG_STREAM and RT_FLAG_STREAM_ADAPTIVE (the staged passes behind the wavefront kernel)."""
    sc, cam = A.scene(pkg, key)
    p = A.frame(key)
    for k in (2, 4):
        s = A.frame(key, k)
        for fmt in (F32, U8):
            got = frames_of(pkg, sc, cam, forced(pkg, k), fmt, A.TAUS, True, True)
            staged = frames_of(pkg, sc, cam, ada_flags(pkg, k), fmt, A.TAUS, False, False)
            for tau in A.TAUS:
                frame, n = got[(tau, None)]
                want = want_of(ada.compose(p, s, k, tau), fmt)
                assert identical(frame, want), (key, k, fmt, tau, mismatch(frame, want))
                assert n == int(ada.refine_mask(p, tau).sum()), (key, k, fmt, tau, n)
                assert identical(frame, staged[(tau, None)][0]) and n == staged[(tau, None)][1], (key, k, fmt, tau)


# ---- 2. bands ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.BANDS, ids=[f"world{c[1]}-band{c[2]}" for c in A.BANDS])
def test_bands(pkg, case):
    """Every rank's rows equal the single context's rows and the oracle's, and the per-rank refined counts agree: the halo pass (K = 1)
    with waves that straddle halo slots and with off-image halo rows."""
    key, world, band, k, fmt = case
    sc, cam = A.scene(pkg, key)
    p, s = A.frame(key), A.frame(key, k)
    h = p.shape[0]
    for tau in (0.0, TAU):
        want = want_of(ada.compose(p, s, k, tau), fmt)
        mask = ada.refine_mask(p, tau)
        single, n = frames_of(pkg, sc, cam, forced(pkg, k), fmt, (tau,), True)[(tau, None)]
        assert identical(single, want) and n == int(mask.sum()), (tau, mismatch(single, want))
        seen = np.zeros(h, dtype=bool)
        for rank in range(world):
            rows = pkg.band_rows_of_rank(h, band, world, rank)
            got, n = frames_of(pkg, sc, cam, forced(pkg, k), fmt, (tau,), True, rank=rank, world=world, band_rows=band)[(tau, None)]
            assert got.shape[0] == len(rows)
            assert identical(got, single[rows]) and identical(got, want[rows]), (rank, tau, mismatch(got, want[rows]))
            assert n == int(mask[rows].sum()), (rank, tau, n)
            seen[rows] = True
        assert seen.all()


# ---- 3. geometry -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", A.GEO_LAYOUTS, ids=[f"rank{l[1]}of{l[0]}" for l in A.GEO_LAYOUTS])
def test_geometry(pkg, layout):
    """Forced plus RT_FLAG_SSAA_GEOMETRY: ssaa_geometry_ref.compose on the oracle's planes, and the context without the two flags."""
    world, rank, band = layout
    key = A.GEOMETRY
    sc, cam = A.scene(pkg, key)
    p = A.frame(key)
    obj, nrm = A.planes(key)
    rows = pkg.band_rows_of_rank(p.shape[0], band, world, rank)
    for k, fmt in ((2, F32), (4, U8)):
        s = A.frame(key, k)
        kw = dict(rank=rank, world=world, band_rows=band)
        got = frames_of(pkg, sc, cam, forced(pkg, k, pkg.RT_FLAG_SSAA_GEOMETRY), fmt, A.GEO_TAUS, True, coses=A.GEO_COSES, **kw)
        staged = frames_of(pkg, sc, cam, ada_flags(pkg, k, pkg.RT_FLAG_SSAA_GEOMETRY), fmt, A.GEO_TAUS, False, coses=A.GEO_COSES, **kw)
        for tau in A.GEO_TAUS:
            for c in A.GEO_COSES:
                frame, n = got[(tau, c)]
                want = want_of(geo.compose(p, s, k, tau, obj, nrm, c), fmt)[rows]
                mask = (ada.refine_mask(p, tau) | geo.geo_mask(obj, nrm, c))[rows]
                assert identical(frame, want), (layout, k, tau, c, mismatch(frame, want))
                assert n == int(mask.sum()), (layout, k, tau, c, n)
                assert identical(frame, staged[(tau, c)][0]) and n == staged[(tau, c)][1], (layout, k, tau, c)


# ---- 4. beyond each limit, without RT_FLAG_STREAM ------------------------------------------------------------------------------------------
def test_beyond_the_ray_lists_limit(pkg):
    """569 objects: the staged ray-list kernel cannot hold them, the wavefront (or simple) kernel can -- the plain pass stays what it is."""
    key = A.BEYOND_LIST
    sc, cam = A.scene(pkg, key)
    p, s = A.frame(key), A.frame(key, 2)
    for extra in (0, pkg.RT_FLAG_SIMPLE):
        e = frames_of(pkg, sc, cam, ada_flags(pkg, 2, extra), F32, (TAU,), False)
        assert isinstance(e, pkg.RtError) and e.code == -2 and "rt_create: adaptive supersampling stages 163872 bytes of LDS per workgroup (limit 160 KiB)" in e.message
        for fmt in (F32, U8):
            got = frames_of(pkg, sc, cam, ada_flags(pkg, 2, extra | pkg.RT_FLAG_STREAM_ADAPTIVE), fmt, (-1.0, TAU), True, False)
            for tau in (-1.0, TAU):
                want = want_of(ada.compose(p, s, 2, tau), fmt)
                assert identical(got[(tau, None)][0], want), (extra, fmt, tau, mismatch(got[(tau, None)][0], want))
                assert got[(tau, None)][1] == int(ada.refine_mask(p, tau).sum())


def test_beyond_the_wavefront_kernels_limit(pkg):
    key = A.beyond_wavefront(pkg)
    sc, cam = A.scene(pkg, key)
    p, s = A.frame(key), A.frame(key, 2)
    e = frames_of(pkg, sc, cam, ada_flags(pkg, 2), F32, (TAU,), False)
    assert isinstance(e, pkg.RtError) and e.code == -2 and e.message.startswith("rt_create: scene needs ") and e.message.endswith(" bytes of LDS per workgroup (limit 160 KiB)")
    got = frames_of(pkg, sc, cam, ada_flags(pkg, 2, pkg.RT_FLAG_STREAM_ADAPTIVE), F32, (TAU,), True, True)[(TAU, None)]
    want = ada.compose(p, s, 2, TAU)
    assert identical(got[0], want) and got[1] == int(ada.refine_mask(p, TAU).sum()), mismatch(got[0], want)
    e = frames_of(pkg, sc, cam, ada_flags(pkg, 2, pkg.RT_FLAG_STREAM_ADAPTIVE | pkg.RT_FLAG_COUNT), F32, (TAU,), True)
    assert isinstance(e, pkg.RtError) and e.code == -2 and "streamed passes book no counters" in e.message


def test_beyond_the_g_passes_limit(pkg):
    key = A.BEYOND_GBUFFER
    sc, cam = A.scene(pkg, key)
    p, s = A.frame(key), A.frame(key, 2)
    obj, nrm = A.planes(key)
    g = pkg.RT_FLAG_SSAA_GEOMETRY
    e = frames_of(pkg, sc, cam, ada_flags(pkg, 2, g), F32, (TAU,), False)   # (the first of the three checks answers: the wavefront kernel's)
    assert isinstance(e, pkg.RtError) and e.code == -2 and e.message.startswith("rt_create: scene needs ")
    e = frames_of(pkg, sc, cam, ada_flags(pkg, 2, g | pkg.RT_FLAG_SIMPLE), F32, (TAU,), False)
    assert isinstance(e, pkg.RtError) and e.code == -2 and e.message.startswith("rt_create: adaptive supersampling stages ")
    got = frames_of(pkg, sc, cam, ada_flags(pkg, 2, g | pkg.RT_FLAG_STREAM_ADAPTIVE), F32, (TAU, INF), True, True, coses=(-INF, 0.9))
    for tau in (TAU, INF):
        for c in (-INF, 0.9):
            want = geo.compose(p, s, 2, tau, obj, nrm, c)
            assert identical(got[(tau, c)][0], want), (tau, c, mismatch(got[(tau, c)][0], want))
            assert got[(tau, c)][1] == int((ada.refine_mask(p, tau) | geo.geo_mask(obj, nrm, c)).sum())


def test_simple_geometry_context_beyond_every_limit(pkg):
    """RT_FLAG_SIMPLE | RT_FLAG_SSAA_GEOMETRY on the 2 562 spheres: with the flag none of the three size checks fires (a sphere costs the G
    pass 64 bytes of LDS, the wavefront kernel 80 and the ray list 288, so without the flag a sphere scene meets the G pass's refusal only
    behind the other two), the plain pass is streamed as for every simple context of that size, and the frame is the default context's."""
    key = A.BEYOND_GBUFFER
    sc, cam = A.scene(pkg, key)
    g = pkg.RT_FLAG_SSAA_GEOMETRY | pkg.RT_FLAG_STREAM_ADAPTIVE
    a = frames_of(pkg, sc, cam, ada_flags(pkg, 4, g | pkg.RT_FLAG_SIMPLE), U8, (TAU,), True, True, coses=(0.9,))[(TAU, 0.9)]
    b = frames_of(pkg, sc, cam, ada_flags(pkg, 4, g), U8, (TAU,), True, True, coses=(0.9,))[(TAU, 0.9)]
    assert identical(a[0], b[0]) and a[1] == b[1] > 0


# ---- 5. degree 3 -----------------------------------------------------------------------------------------------------------------------------
def plain(pkg, sc, cam, flags):
    r = pkg.Renderer(sc, device=0, flags=flags)
    try:
        r.update(cam)
        return r.download().copy()
    finally:
        r.cleanup_update()


def check_cubic(pkg, make, cam, w, h, k):
    sc = make(w, h)
    got = frames_of(pkg, sc, cam, forced(pkg, k), F32, (-1.0, TAU), True, True)
    full = plain(pkg, sc, cam, pkg.RT_FLAG_STREAM | kflag(pkg, k))
    assert identical(got[(-1.0, None)][0], full) and got[(-1.0, None)][1] == w * h, mismatch(got[(-1.0, None)][0], full)
    p, s = plain(pkg, sc, cam, pkg.RT_FLAG_STREAM), plain(pkg, make(k * w, k * h), cam, pkg.RT_FLAG_STREAM)
    want = ada.compose(p, s, k, TAU)
    assert identical(got[(TAU, None)][0], want), mismatch(got[(TAU, None)][0], want)
    mask = ada.refine_mask(p, TAU)
    assert got[(TAU, None)][1] == int(mask.sum()) and mask.any() and not mask.all()


@pytest.mark.parametrize("seed", [0, 1])
def test_random_cubic_scenes(pkg, seed):
    cam = random_cubic_scene(pkg, seed, 64, 48)[1]
    check_cubic(pkg, lambda w, h: random_cubic_scene(pkg, seed, w, h)[0], cam, 64, 48, 2 if seed % 2 else 4)


def test_shipped_cubic_scene(pkg):
    check_cubic(pkg, lambda w, h: pkg.Scene.load_from_file(scene_path("clebsch")).set_size(w, h), None, 64, 48, 2)


# ---- 6. RT_FLAG_FAST -------------------------------------------------------------------------------------------------------------------------
def test_fast_variant_to_its_bar(pkg):
    """Every pixel refined, against the strict frame: 1e-5 relative per channel, at most max(3, 0.2 % of the pixels) beyond it."""
    for key, k in ((A.FORCED[4], 4), (A.FORCED[-1], 2)):
        sc, cam = A.scene(pkg, key)
        strict = frames_of(pkg, sc, cam, forced(pkg, k), F32, (-1.0,), True)[(-1.0, None)][0]
        fast, n = frames_of(pkg, sc, cam, forced(pkg, k, pkg.RT_FLAG_FAST), F32, (-1.0,), True)[(-1.0, None)]
        h, w = strict.shape[:2]
        c = compare(fast[..., :3], strict[..., :3])
        print("FAST against strict:", key, k, c)
        assert n == w * h and np.all(fast[..., 3] == 1.0) and c["n_bad_pixels"] <= max(3, int(0.002 * w * h)), (key, c)


# ---- 7. the flag alone on a small scene --------------------------------------------------------------------------------------------------
def test_the_flag_alone_changes_nothing(pkg):
    key = A.FORCED[3]
    sc, cam = A.scene(pkg, key)
    for extra in (0, pkg.RT_FLAG_SIMPLE, pkg.RT_FLAG_SSAA_GEOMETRY):
        a = frames_of(pkg, sc, cam, ada_flags(pkg, 2, extra | pkg.RT_FLAG_STREAM_ADAPTIVE), F32, (TAU,), False, False)[(TAU, None)]
        b = frames_of(pkg, sc, cam, ada_flags(pkg, 2, extra), F32, (TAU,), False, False)[(TAU, None)]
        assert identical(a[0], b[0]) and a[1] == b[1] > 0, extra
    counters = []
    for extra in (pkg.RT_FLAG_STREAM_ADAPTIVE, 0):
        r = pkg.Renderer(sc, device=0, flags=ada_flags(pkg, 2, extra | pkg.RT_FLAG_COUNT), ssaa_threshold=TAU)
        try:
            assert not r.streamed_adaptive
            r.update(cam)
            counters.append(r.counters())
        finally:
            r.cleanup_update()
    assert counters[0] == counters[1] and counters[0]["primary_rays"] > sc.desc().width * sc.desc().height
    # with the decision true the streamed passes book no counters: RT_ERR_SCENE from rt_create, on this small scene through RT_FLAG_STREAM's own refusal first
    with pytest.raises(pkg.RtError) as e:
        pkg.Renderer(sc, device=0, flags=forced(pkg, 2, pkg.RT_FLAG_COUNT))
    assert e.value.code == -1 and "RT_FLAG_STREAM is not available with RT_FLAG_COUNT" in e.value.message
    big, _ = A.scene(pkg, A.BEYOND_LIST)
    with pytest.raises(pkg.RtError) as e:
        pkg.Renderer(big, device=0, flags=ada_flags(pkg, 2, pkg.RT_FLAG_STREAM_ADAPTIVE | pkg.RT_FLAG_COUNT))
    assert e.value.code == -2 and "streamed passes book no counters" in e.value.message


# ---- 8. graphs and scene updates -------------------------------------------------------------------------------------------------------------
def test_two_cameras_in_one_graph_replayed_twice(pkg):
    """... and rt_set_ssaa_threshold between the replays: the graph keeps the tau it was captured with."""
    import torch
    key = A.FORCED[4]
    sc, _ = A.scene(pkg, key)
    cams = [np.ascontiguousarray(pkg.IDENTITY, dtype=np.float64).reshape(16), pkg.camera_matrix((0.5, 0.3, -1.0), 88.0, 2.0)]
    want = [frames_of(pkg, sc, cam, forced(pkg, 2, pkg.RT_FLAG_SSAA_GEOMETRY), F32, (TAU,), True, coses=(0.9,))[(TAU, 0.9)][0] for cam in cams]
    assert not identical(want[0], want[1])
    r = pkg.Renderer(sc, device=0, flags=forced(pkg, 2, pkg.RT_FLAG_SSAA_GEOMETRY), ssaa_threshold=TAU, ssaa_min_cos=0.9)
    s = torch.cuda.Stream()
    g = None
    try:
        r.update(cams[1], stream=s.cuda_stream, timed=False)   # (first call on this stream before the capture)
        torch.cuda.synchronize()
        bufs = [torch.empty((r.local_rows, r.width, 4), dtype=torch.float32, device="cuda:0") for _ in cams]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for cam, buf in zip(cams, bufs):
                r.update(cam, dev_fb=buf.data_ptr(), stream=s.cuda_stream, timed=False)
        for rep in range(2):
            with torch.cuda.stream(s):
                for b in bufs:
                    b.view(torch.int32).fill_(0x7FC00000)
                g.replay()
            s.synchronize()
            for i, buf in enumerate(bufs):
                assert identical(buf.cpu().numpy(), want[i]), (rep, i)
            r.set_ssaa_threshold(-1.0)
    finally:
        torch.cuda.synchronize()
        del g
        r.cleanup_update()


def test_set_scene_moves_the_569_object_field(pkg):
    sc, cam = A.scene(pkg, A.BEYOND_LIST)
    a = sc.arrays()
    coefs = a["coefs"].copy()
    spheres = np.arange(len(coefs) - 1)   # (the last object is the floor)
    c = -0.5 * coefs[spheres, 16:19]
    r2 = (c * c).sum(axis=1) - coefs[spheres, 19]
    c2 = c + np.random.default_rng(5).uniform(-0.7, 0.7, c.shape)
    coefs[spheres, 16:19] = -2.0 * c2
    coefs[spheres, 19] = (c2 * c2).sum(axis=1) - r2
    moved = pkg.desc_from_arrays(a["width"], a["height"], a["vertical_fov"], a["bg_color"], a["max_reflections"], coefs, a["reflection"], a["albedo"],
                                 a["light_is_spherical"], a["light_p"], a["light_color"])
    flags = ada_flags(pkg, 2, pkg.RT_FLAG_STREAM_ADAPTIVE)
    r = pkg.Renderer(sc, device=0, flags=flags, ssaa_threshold=TAU)
    try:
        assert r.streamed_adaptive and not r.streamed
        r.update(cam)
        before = r.download().copy()
        r.set_scene(coefs=coefs)
        r.update(cam)
        after, n = r.download().copy(), r.refined
    finally:
        r.cleanup_update()
    fresh = frames_of(pkg, moved, cam, flags, F32, (TAU,), True)[(TAU, None)]
    assert not identical(after, before) and identical(after, fresh[0]) and n == fresh[1]


def test_frames_interleaved_with_queries_are_unchanged(pkg):
    key = A.FORCED[4]
    sc, cam = A.scene(pkg, key)
    want = want_of(ada.compose(A.frame(key), A.frame(key, 4), 4, TAU), U8)
    r = pkg.Renderer(sc, device=0, flags=forced(pkg, 4), fmt=U8, ssaa_threshold=TAU)
    q = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_QUERIES)
    try:
        assert q.streamed_queries
        r.update(cam)
        assert identical(r.download(), want)
        assert (q.gbuffer()[0].cpu().numpy() >= 0).any()
        r.update(cam)
        assert identical(r.download(), want)
        assert len(q.trace([[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0], [0.0, -0.3, 1.0]])) == 2
        q.update()
        r.update(cam)
        assert identical(r.download(), want)
    finally:
        r.cleanup_update()
        q.cleanup_update()


# ---- 9. the multi-GPU layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["dense", "sparse"])
def test_multi_renderer(pkg, transport):
    key = A.FORCED[4]
    sc, cam = A.scene(pkg, key)
    extra = pkg.RT_MULTI_SPARSE if transport == "sparse" else 0
    single = frames_of(pkg, sc, cam, forced(pkg, 2), F32, (0.0, TAU), True)
    assert identical(single[(TAU, None)][0], ada.compose(A.frame(key), A.frame(key, 2), 2, TAU))
    m = pkg.MultiRenderer(sc, [0, 0], band_rows=8, parts=2, flags=forced(pkg, 2) | extra)
    try:
        for tau in (TAU, 0.0):
            m.set_ssaa_threshold(tau)
            for _ in range(2):
                m.update()
            got = m.download()
            assert identical(got, single[(tau, None)][0]), (transport, tau, mismatch(got, single[(tau, None)][0]))
    finally:
        m.cleanup_update()


# ---- 10. init_update() / update() ------------------------------------------------------------------------------------------------------------
ADAPTER = r"""
import ctypes as C, os, re, subprocess, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "tools"))
import __graft_entry__ as g
import ssaa_adaptive_ref as ada
import stream_adaptive_scenes as A
pkg = g.load_package()
sc, cam = A.scene(pkg, A.BEYOND_LIST)
want = ada.compose(A.frame(A.BEYOND_LIST), A.frame(A.BEYOND_LIST, 2), 2, A.TAU)
a = sc.arrays()
upd = C.CDLL(pkg.UPDATE_LIB_PATH)
names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
update = getattr(upd, re.search(r"\b(_Z\d+updateRKN3glm3matI\S*)\b", names).group(1))
cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
update.argtypes, update.restype = [C.c_void_p], C.c_float
upd.mi355rt_update_download.argtypes = [C.c_void_p, C.c_size_t]
cam = np.ascontiguousarray(cam, dtype=np.float64)
init(7, sc._h)
ms = update(cam.ctypes.data)
out = np.zeros((a["height"], a["width"], 4), np.float32)
rc = upd.mi355rt_update_download(out.ctypes.data_as(C.c_void_p), out.nbytes)
cleanup()
print("frame", rc, ms > 0.0, bool(np.array_equal(out.view(np.uint32), want.view(np.uint32))), bool(ada.refine_mask(A.frame(A.BEYOND_LIST), A.TAU).any()))
"""


def adapter(**env):
    return subprocess.run([sys.executable, "-c", ADAPTER, ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))


def test_init_update_with_the_environment_switch():
    """The reference's back-end contract (ctypes on libmi355rt_update.so, a fresh process) on the 569-object field."""
    env = dict(MI355RT_SSAA="2", MI355RT_SSAA_ADAPTIVE="0.03125")
    out = adapter(MI355RT_STREAM_ADAPTIVE="1", **env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "frame 0 True True True", out.stdout
    out = adapter(MI355RT_STREAM_ADAPTIVE="0", **env)   # without the switch rt_create's refusal answers, as ever
    assert out.returncode != 0 and "adaptive supersampling stages 163872 bytes" in out.stderr, (out.stdout, out.stderr)
    out = adapter(MI355RT_STREAM_ADAPTIVE="yes", **env)
    assert out.returncode != 0 and "mi355rt: MI355RT_STREAM_ADAPTIVE: expected 0 or 1" in out.stderr, (out.stdout, out.stderr)
