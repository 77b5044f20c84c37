"""The streamed frame kernel on the GPU (RT_FLAG_STREAM and scenes too large for LDS; csrc/rt_stream.hip).  The
reference is the CPU oracle, bit for bit, for strict contexts and surfaces of degree <= 2 in both formats; degree 3 and RT_FLAG_FAST are
held to the bars of tests/test_gpu_parity.py.  The conditions that keep these tests from being vacuous (which objects own pixels, the
large scene's shadow) are asserted on the oracle alone in tests/test_stream_host.py, for the very scenes and seeds used here."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, compare, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cubic_device_lab as D  # noqa: E402  (the oracle under the device's cbrt / acos / cos)
import raw_desc_scenes as R  # noqa: E402
import ssaa_ref  # noqa: E402
import stream_scenes as S  # noqa: E402
from test_gpu_parity import mixed_scene  # noqa: E402
from test_raw_descriptor_gpu import rgba8_of  # noqa: E402

pytestmark = pytest.mark.gpu

F32, U8 = 0, 1
QUADRIC = ["quadratic", "20spheres", "reflection_test"]
CUBIC = ["clebsch", "cubic", "cayley", "dingdong", "monkey_saddle"]
MOVED = ((1.5, 0.5, -2.0), 80.0, -6.0)


@pytest.fixture(autouse=True)
def the_feature(pkg):
    """Nearly every test here fails without the feature for its own reason (the flag, `Renderer.streamed`, the refused scene).  The few that
    compare an unforced small context with something else would not; they are part of the feature's suite, so they ask for it too."""
    assert pkg.RT_FLAG_STREAM == 8192


def frame(pkg, sc, cam=None, frames=1, expect_streamed=True, **kw):
    r = pkg.Renderer(sc, device=0, **kw)
    try:
        assert r.streamed == expect_streamed
        for _ in range(frames):
            r.update(cam)
        return r.download()
    finally:
        r.cleanup_update()


def check_both_formats(pkg, sc, want, what, cam=None, flags=None, **kw):
    """The streamed RGBA32F frame is the oracle's, the RGBA8 frame its stated quantisation."""
    flags = pkg.RT_FLAG_STREAM if flags is None else flags
    got = frame(pkg, sc, cam, flags=flags, **kw)
    assert np.all(got[..., 3] == 1.0) and R.same_as_oracle(got[..., :3], want), (what, R.n_diff(got[..., :3], want))
    got8 = frame(pkg, sc, cam, flags=flags, fmt=pkg.RT_FMT_RGBA8, **kw)
    q, ok = rgba8_of(want)
    assert got8.dtype == np.uint8 and not ((got8 != q)[..., :3] & ok).any() and np.all(got8[..., 3] == 255), what


def shipped(pkg, name, w, h, max_refl=None):
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
    return sc.set_max_reflections(max_refl) if max_refl is not None else sc


@functools.lru_cache(maxsize=None)
def shipped_oracle(name, w, h, max_refl=None, cam_bytes=None):
    import __graft_entry__ as graft
    cam = None if cam_bytes is None else np.frombuffer(cam_bytes, dtype=np.float64)
    return graft.load_oracle().load_scene(scene_path(name)).with_size(w, h, max_refl).render(cam=cam, nthreads=8)


@functools.lru_cache(maxsize=None)
def large_n():
    import __graft_entry__ as graft
    return S.first_count_beyond_lds(graft.load_package())


@functools.lru_cache(maxsize=None)
def large_want(big_last=True):
    import __graft_entry__ as graft
    pkg = graft.load_package()
    return S.oracle_of(pkg, S.field(pkg, large_n(), S.LARGE_SEED, big_last=big_last)).render(nthreads=8)


# ---- chunk boundaries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.COUNTS)
@pytest.mark.parametrize("kind", ["sphere", "quadric"])
def test_chunk_boundaries(pkg, kind, n):
    """1 .. 193 objects of one class: the last chunk holds 1, 63, 64 entries or a single one behind a full chunk.  Without mirrors and
    with mirrors at depths 0, 1 and 4, both formats; the 37 x 21 frame has partial tiles and partial 8 x 8 blocks."""
    for mirrors, depth in ((False, 0), (True, 0), (True, 1), (True, 4)):
        sc = S.field(pkg, n, S.FIELD_SEED, kind, mirrors=mirrors, depth=depth)
        check_both_formats(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), (kind, n, mirrors, depth))
    sc = S.field(pkg, n, S.FIELD_SEED, kind, w=37, h=21, mirrors=True, depth=1)
    check_both_formats(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), (kind, n, "37 x 21"))


def test_65_planes(pkg):
    for depth in (0, 1, 4):
        sc = S.planes(pkg, 65, 5, depth=depth)
        check_both_formats(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), ("planes", depth))
    sc = S.planes(pkg, 65, 5, w=37, h=21, depth=1)
    check_both_formats(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), "planes, 37 x 21")


@pytest.mark.parametrize("seed", range(6))
def test_mixed_scenes(pkg, seed):
    """Every class of degree <= 2 in one scene (tests/test_gpu_parity.py: mixed_scene) with a point and a directional light more."""
    for w, h in ((64, 48), (37, 21)):
        sc = mixed_scene(pkg, seed, w, h)
        sc.add_light("spherical", [3.0, 9.0, 4.0], (1.0, 0.9, 0.8), 400.0)
        sc.add_light("directional", [-0.3, -1.0, 0.4], (0.7, 0.8, 1.0), 0.9)
        check_both_formats(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), ("mixed", seed, w, h))


@pytest.mark.parametrize("seed", range(8))
def test_raw_descriptor_scenes(pkg, seed):
    """The generator of tests/tools/raw_desc_scenes.py: odd light vectors, non-finite colours and ratios, negative backgrounds, moved
    cameras, sizes down to one pixel (capped at 80 x 60) -- nothing of which the streamed kernel may treat specially, since it skips
    nothing.  The default kernel's frame is the same bits."""
    osc, cam = R.scene(seed)
    osc.width, osc.height = min(osc.width, 80), min(osc.height, 60)
    d = R.desc(pkg, osc)
    want = osc.render(cam=cam, nthreads=8)
    check_both_formats(pkg, d, want, ("raw", seed), cam=cam)
    assert R.same(frame(pkg, d, cam, flags=pkg.RT_FLAG_STREAM), frame(pkg, d, cam, frames=2, expect_streamed=False))


# ---- the reason for the feature ---------------------------------------------------------------------------------------------------------
def test_scene_beyond_the_lds_limit_renders(pkg):
    """The first sphere count the default kernel cannot hold, plus one large sphere appended last whose shadow falls on the field:
    created with flags = 0, streamed, and the oracle's frame; a small default context is not streamed."""
    sc = S.field(pkg, large_n(), S.LARGE_SEED, big_last=True)
    want = large_want()
    # (a smoke check only.  The real condition -- the last sphere's shadow changes a pixel that sphere does not own -- is asserted on the oracle
    # in tests/test_stream_host.py::test_large_field_shows_every_chunk_and_the_last_spheres_shadow for this very scene: S.LARGE_SEED and
    # big_last=True.  Change the seed there and here together.)
    assert (want != large_want(False)).any()
    check_both_formats(pkg, sc, want, "large field", flags=0)
    small = pkg.Renderer(S.field(pkg, 65, S.FIELD_SEED), device=0)
    assert small.streamed is False
    small.cleanup_update()
    one_less = pkg.Renderer(S.field(pkg, large_n() - 1, S.LARGE_SEED), device=0)
    assert one_less.streamed is False   # (the count is the first one beyond the limit)
    one_less.cleanup_update()


def test_simple_context_beyond_its_limit_renders_the_same_frame(pkg):
    sc = S.field(pkg, large_n(), S.LARGE_SEED, big_last=True)
    got = frame(pkg, sc, flags=pkg.RT_FLAG_SIMPLE)
    assert R.same_as_oracle(got[..., :3], large_want())
    # a simple context within its own limit stays the simple kernel
    assert R.same(frame(pkg, S.field(pkg, 193, S.FIELD_SEED), flags=pkg.RT_FLAG_SIMPLE, expect_streamed=False),
                  frame(pkg, S.field(pkg, 193, S.FIELD_SEED), flags=pkg.RT_FLAG_STREAM))


def test_large_mixed_scene_with_mirrors(pkg):
    """About 2 000 spheres, ellipsoids and two planes, every fifth object a mirror, depth 2."""
    sc = S.mixed_large(pkg, 2000, S.MIXED_SEED)
    check_both_formats(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), "large mixed", flags=0)


# ---- cross-checks on device results alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QUADRIC)
def test_streamed_equals_default_and_nocull(pkg, name):
    sc = shipped(pkg, name, 96, 72, 4)
    for cam in (None, pkg.camera_matrix(*MOVED)):
        a = frame(pkg, sc, cam, flags=pkg.RT_FLAG_STREAM)
        assert R.same(a, frame(pkg, sc, cam, frames=2, expect_streamed=False)), name
        assert R.same(a, frame(pkg, sc, cam, flags=pkg.RT_FLAG_STREAM | pkg.RT_FLAG_NOCULL)), name


def shade_of_primary(pkg, r, cam=None):
    """rt_shade_rays on the rays rt_primary_rays forms for this context's frame, on the device."""
    import torch
    rays, _ = r.primary_rays(cam)
    out = torch.empty((r.height, r.width, 4), dtype=torch.float32, device=rays.device)
    r.shade_into(rays.data_ptr(), r.height * r.width, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", QUADRIC + CUBIC)
def test_streamed_equals_shade_rays_on_primary_rays(pkg, name):
    """The definition, on the device alone: the same source under -ffp-contract=off.  Bit for bit for every degree (the five shipped
    cubic scenes included: measured equal on all of them, so asserted)."""
    sc = shipped(pkg, name, 80, 60, 4)
    r = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_STREAM)
    try:
        for cam in (None, pkg.camera_matrix(*MOVED)):
            r.update(cam)
            got, want = r.download(), shade_of_primary(pkg, r, cam)
            print(name, "pixels that differ from rt_shade_rays(rt_primary_rays):", R.n_diff(got, want))
            assert R.same(got, want), name
    finally:
        r.cleanup_update()


@pytest.mark.parametrize("name", CUBIC)
def test_cubic_scenes_to_their_bar(pkg, oracle, name):
    """1e-5 relative per channel; at most max(3, 0.2 % of the pixels) beyond it against the glibc oracle, none against the oracle under
    the device's cbrt / acos / cos.  The large-count path of degree 3 (the index list in chunks) is taken past its first chunk by
    tests/test_cubic_chunks_gpu.py, on fields of 64, 65 and 129 degree-3 objects."""
    w, h = 80, 60
    got = frame(pkg, shipped(pkg, name, w, h), flags=pkg.RT_FLAG_STREAM)
    c = compare(got[..., :3], shipped_oracle(name, w, h))
    print(name, c)
    assert c["n_bad_pixels"] <= max(3, int(0.002 * w * h)), c
    c = D.compare_device_libm(pkg, got[..., :3], oracle.load_scene(scene_path(name)).with_size(w, h))
    assert c["n_bad_pixels"] == 0, c


# ---- context kinds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [F32, U8], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("k", [2, 4])
def test_supersampling(pkg, k, fmt):
    """The streamed kernel renders the internal k x finer frame; the resolve is unchanged (tests/tools/ssaa_ref.py on the oracle's samples)."""
    w, h = 40, 30
    flag = pkg.RT_FLAG_SSAA2 if k == 2 else pkg.RT_FLAG_SSAA4
    for name in ("reflection_test", "quadratic"):
        want = ssaa_ref.resolve(shipped_oracle(name, k * w, k * h, 4), k)
        want = ssaa_ref.quantise(want) if fmt == U8 else want
        got = frame(pkg, shipped(pkg, name, w, h, 4), flags=pkg.RT_FLAG_STREAM | flag, fmt=fmt)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8)), name


def test_rank_1_of_3_with_bands_of_8(pkg):
    w, h = 64, 50   # (a ragged last band)
    sc = shipped(pkg, "reflection_test", w, h, 4)
    r = pkg.Renderer(sc, device=0, rank=1, world=3, band_rows=8, flags=pkg.RT_FLAG_STREAM)
    try:
        r.update()
        rows = r.row_map()
        assert len(rows) == r.local_rows and 0 < len(rows) < h
        assert R.same_as_oracle(r.download()[..., :3], shipped_oracle("reflection_test", w, h, 4)[rows])
    finally:
        r.cleanup_update()


def test_moved_camera(pkg):
    cam = pkg.camera_matrix((1.5, 2.0, -3.0), 78.0, 9.0)
    for name in ("20spheres", "quadratic"):
        want = shipped_oracle(name, 80, 60, None, np.ascontiguousarray(cam, dtype=np.float64).tobytes())
        check_both_formats(pkg, shipped(pkg, name, 80, 60), want, name, cam=cam)
    sc = S.field(pkg, large_n(), S.LARGE_SEED, big_last=True)
    cam = pkg.camera_matrix((0.5, 0.3, -1.0), 88.0, 2.0)
    got = frame(pkg, sc, cam)
    assert R.same_as_oracle(got[..., :3], S.oracle_of(pkg, sc).render(cam=cam, nthreads=8))


def test_fast_variant_to_its_bar(pkg):
    """RT_FLAG_FAST: its own arithmetic; 1e-5 relative, at most max(2, 0.2 % of the pixels) beyond it, as the FAST frames of
    tests/test_gpu_parity.py."""
    w, h = 80, 60
    for name in QUADRIC + CUBIC:
        got = frame(pkg, shipped(pkg, name, w, h), flags=pkg.RT_FLAG_STREAM | pkg.RT_FLAG_FAST)
        c = compare(got[..., :3], shipped_oracle(name, w, h))
        assert c["n_bad_pixels"] <= max(2, int(0.002 * w * h)), (name, c)
    sc = S.field(pkg, large_n(), S.LARGE_SEED, big_last=True)
    c = compare(frame(pkg, sc, flags=pkg.RT_FLAG_FAST)[..., :3], large_want())
    assert c["n_bad_pixels"] <= max(2, int(0.002 * 64 * 48)), c


@pytest.mark.parametrize("transport", ["dense", "sparse"])
def test_multi_renderer(pkg, transport):
    extra = pkg.RT_MULTI_SPARSE if transport == "sparse" else 0
    for sc, want, flags in ((shipped(pkg, "reflection_test", 80, 60, 4), shipped_oracle("reflection_test", 80, 60, 4), pkg.RT_FLAG_STREAM),
                            (S.field(pkg, large_n(), S.LARGE_SEED, big_last=True), large_want(), 0)):
        m = pkg.MultiRenderer(sc, [0, 0], band_rows=8, parts=2, flags=flags | extra)
        try:
            for _ in range(2):
                m.update()
            got = m.download()
            assert R.same_as_oracle(got[..., :3], want), transport
            sent, dense = m.last_transfer()
            assert sent > 0 and dense == got.shape[0] * got.shape[1] * 16
        finally:
            m.cleanup_update()


# ---- no frame state -----------------------------------------------------------------------------------------------------------------------
def test_two_cameras_in_one_graph_replayed_twice(pkg):
    import torch
    sc = S.field(pkg, 129, S.FIELD_SEED, mirrors=True, depth=1)
    cams = [np.ascontiguousarray(pkg.IDENTITY, dtype=np.float64).reshape(16), pkg.camera_matrix((0.5, 0.3, -1.0), 88.0, 2.0)]
    plain = [frame(pkg, sc, cam, flags=pkg.RT_FLAG_STREAM) for cam in cams]
    assert not R.same(plain[0], plain[1])
    r = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_STREAM)
    s = torch.cuda.Stream()
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
            for k, buf in enumerate(bufs):
                assert R.same(buf.cpu().numpy(), plain[k]), (rep, k)
    finally:
        torch.cuda.synchronize()
        del g
        r.cleanup_update()


def test_frames_interleaved_with_queries_are_unchanged(pkg):
    sc = shipped(pkg, "reflection_test", 80, 60, 4)
    r = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_STREAM)
    try:
        r.update()
        first = r.download().copy()
        obj = r.gbuffer()[0].cpu().numpy()
        assert (obj >= 0).any()
        r.update()
        assert R.same(r.download(), first)
        hits = r.trace([[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0], [0.0, -0.3, 1.0]])
        assert len(hits) == 2
        r.gbuffer(pkg.camera_matrix(*MOVED))
        r.update()
        assert R.same(r.download(), first)
    finally:
        r.cleanup_update()


# ---- rt_set_scene -------------------------------------------------------------------------------------------------------------------------
def test_set_scene_moves_the_large_field(pkg):
    """Every sphere of the large field moved (same radii): the streamed kernel reads the blob rt_set_scene rebuilds."""
    sc = S.field(pkg, large_n(), S.LARGE_SEED, big_last=True)
    a = sc.arrays()
    coefs = a["coefs"].copy()
    c = -0.5 * coefs[:, 16:19]
    r2 = (c * c).sum(axis=1) - coefs[:, 19]
    rng = np.random.default_rng(5)
    c2 = c + rng.uniform(-0.7, 0.7, c.shape)
    coefs[:, 16:19] = -2.0 * c2
    coefs[:, 19] = (c2 * c2).sum(axis=1) - r2
    moved = pkg.desc_from_arrays(a["width"], a["height"], a["vertical_fov"], a["bg_color"], a["max_reflections"], coefs, a["reflection"], a["albedo"],
                                 a["light_is_spherical"], a["light_p"], a["light_color"])
    r = pkg.Renderer(sc, device=0)
    try:
        assert r.streamed
        r.update()
        before = r.download().copy()
        r.set_scene(coefs=coefs)
        r.update()
        after = r.download().copy()
    finally:
        r.cleanup_update()
    assert not R.same(after, before) and R.same(after, frame(pkg, moved))


# ---- refusals that need a device ---------------------------------------------------------------------------------------------------------
def test_refusals_on_a_streamed_context(pkg):
    import torch
    for sc, flags in ((shipped(pkg, "quadratic", 64, 48), pkg.RT_FLAG_STREAM), (S.field(pkg, large_n(), S.LARGE_SEED), 0),
                      (S.field(pkg, large_n(), S.LARGE_SEED), pkg.RT_FLAG_SIMPLE)):
        r = pkg.Renderer(sc, device=0, flags=flags)
        try:
            assert r.streamed
            r.update()
            msg = torch.zeros(r.sparse_msg_bytes(16) // 4, dtype=torch.int32, device="cuda:0")
            with pytest.raises(pkg.RtError) as e:
                r.update_sparse(msg.data_ptr(), 16)
            assert e.value.code == -1 and "rt_render_sparse" in e.value.message
            with pytest.raises(pkg.RtError) as e:
                r.counters()
            assert e.value.code == -1 and "rt_get_counters" in e.value.message and "streamed" in e.value.message
            with pytest.raises(pkg.RtError) as e:
                r.counters_detail()
            assert e.value.code == -1
        finally:
            r.cleanup_update()


def test_large_scene_refusals_of_rt_create(pkg):
    sc = S.field(pkg, large_n(), S.LARGE_SEED)
    with pytest.raises(pkg.RtError) as e:
        pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_COUNT)
    assert e.value.code == -2 and "streamed kernel books no counters" in e.value.message
    with pytest.raises(pkg.RtError) as e:   # ... and so for a simple context beyond its own limit
        pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_SIMPLE | pkg.RT_FLAG_COUNT)
    assert e.value.code == -2 and "streamed kernel books no counters" in e.value.message
    # an adaptive context is refused as ever, by the same two checks in the same order and with their messages: the refine pass has no
    # streamed kernel
    for extra, text in ((0, r"rt_create: scene needs \d+ bytes of LDS per workgroup \(limit 160 KiB\)$"),
                        (pkg.RT_FLAG_SSAA_GEOMETRY, r"rt_create: scene needs \d+ bytes of LDS per workgroup \(limit 160 KiB\)$"),
                        (pkg.RT_FLAG_SIMPLE, r"rt_create: adaptive supersampling stages \d+ bytes of LDS per workgroup \(limit 160 KiB\)$")):
        with pytest.raises(pkg.RtError, match=text) as e:
            pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA_ADAPTIVE | extra)
        assert e.value.code == -2
    # ... and so are the entry points that still stage the tables
    r = pkg.Renderer(S.field(pkg, 160 * 1024 // 64 + 1, S.LARGE_SEED), device=0)
    try:
        for call, who in ((r.gbuffer, "rt_render_gbuffer"), (lambda: r.pick([(1, 1)]), "rt_pick"), (r.object_extents, "rt_object_extents_host"),
                          (lambda: r.trace([[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]]), "rt_trace_rays_host")):
            with pytest.raises(pkg.RtError, match=rf"{who}: scene needs \d+ bytes of LDS per workgroup \(limit 160 KiB\)") as e:
                call()
            assert e.value.code == -2
    finally:
        r.cleanup_update()


# ---- init_update() / update() -------------------------------------------------------------------------------------------------------------
ADAPTER = r"""
import ctypes as C, os, re, subprocess, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "tools"))
import __graft_entry__ as g
import stream_scenes as S
pkg = g.load_package()
if sys.argv[2] == "field":
    sc = S.field(pkg, S.first_count_beyond_lds(pkg), S.LARGE_SEED, big_last=True)
    want = S.oracle_of(pkg, sc).render(nthreads=8)
else:
    sc = pkg.Scene.load_from_file(sys.argv[2]).set_size(80, 60)
    want = g.load_oracle().load_scene(sys.argv[2]).with_size(80, 60).render(nthreads=8)
a = sc.arrays()
upd = C.CDLL(pkg.UPDATE_LIB_PATH)
names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
update = getattr(upd, re.search(r"\b(_Z\d+updateRKN3glm3matI\S*)\b", names).group(1))
cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
update.argtypes, update.restype = [C.c_void_p], C.c_float
upd.mi355rt_update_download.argtypes = [C.c_void_p, C.c_size_t]
cam = np.ascontiguousarray(pkg.IDENTITY, dtype=np.float64)
init(7, sc._h)
ms = update(cam.ctypes.data)
out = np.zeros((a["height"], a["width"], 4), np.float32)
rc = upd.mi355rt_update_download(out.ctypes.data_as(C.c_void_p), out.nbytes)
cleanup()
print("frame", rc, ms > 0.0, bool(np.array_equal(out[..., :3].view(np.uint32), want.view(np.uint32))), bool(np.all(out[..., 3] == 1.0)))
"""


def adapter(arg, **env):
    return subprocess.run([sys.executable, "-c", ADAPTER, ROOT, arg], capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))


def test_init_update_on_the_large_field():
    """The reference's back-end contract (ctypes on libmi355rt_update.so, a fresh process): init_update() succeeds on a scene the
    reference's window opens, and update() draws the oracle's frame."""
    out = adapter("field")
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "frame 0 True True True", out.stdout


def test_init_update_with_the_environment_switch():
    out = adapter(scene_path("quadratic"), MI355RT_STREAM="1")
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "frame 0 True True True", out.stdout
    # the switch reaches rt_create as RT_FLAG_STREAM: together with adaptive supersampling the flag's own refusal answers
    out = adapter(scene_path("quadratic"), MI355RT_STREAM="1", MI355RT_SSAA="2", MI355RT_SSAA_ADAPTIVE="")
    assert out.returncode != 0 and "RT_FLAG_STREAM is not available with RT_FLAG_SSAA_ADAPTIVE" in out.stderr, (out.stdout, out.stderr)
    out = adapter(scene_path("quadratic"), MI355RT_STREAM="yes")
    assert out.returncode != 0 and "mi355rt: MI355RT_STREAM: expected 0 or 1" in out.stderr, (out.stdout, out.stderr)
