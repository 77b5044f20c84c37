"""rt_trace_paths / rt_primary_rays / rt_pick_paths / mi355rt_update_pick_path on the GPU (csrc/rt_paths.hip)
against the reference composer tests/tools/paths_ref.py, against rays_ref.primary_rays and against the library's own rt_trace_rays /
rt_pick / rt_shade_rays / rt_render.  Strict contexts unless said otherwise.  Every comparison is on all bits (integer views); against
the composer a NaN has to meet a NaN (raw_desc_scenes.same_as_oracle).  Two device results are always compared on all bits."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import paths_ref  # noqa: E402
import rays_ref  # noqa: E402
import raw_desc_scenes as R  # noqa: E402
import cubic_device_lab as D  # noqa: E402  (the oracle under the device's cbrt / acos / cos)
from paths_ref import CAP, ESCAPED, MISS, SURFACE  # noqa: E402
from test_gpu_parity import CUBIC, mixed_scene, oracle_from, random_cubic_scene  # noqa: E402
from test_rays_gpu import arbitrary_rays, hits_of, primary_cases, rescaled, to_device, trace_dev  # noqa: E402
from test_shade_gpu import ARBITRARY, booked, frame_of, mirror_scene, shade_dev  # noqa: E402
from test_shade_host import FAR_RAY, RATIO_ABOVE, RATIO_BELOW, facing_mirrors, far_plane, ratio_scene  # noqa: E402
from test_paths_host import CONE_RAYS, DEPTH_CAM, MIRROR_RAYS, MOVED, cone_scene, depth_scene  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 40, 30
F = np.float32


def ends_of(tensor):
    return tensor.cpu().numpy().reshape(-1).view(paths_ref.END_DTYPE)


def paths_dev(r, rays, m=None, last=True, stream=None, timed=True, d_rays=None):
    """rt_trace_paths on device tensors: (segments [m, n], last [n] or None, ends [n]); every output starts as NaN / -1 words."""
    import torch
    n = len(rays) if d_rays is None else d_rays.numel() // 6
    m = r._max_segments(m)
    d_rays = to_device(rays) if d_rays is None else d_rays
    seg = torch.full((max(m, 1) * n, 6), float("nan"), dtype=torch.float64, device="cuda:0")
    lst = torch.full((n, 6), float("nan"), dtype=torch.float64, device="cuda:0")
    end = torch.full((n, 4), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ms = r.paths_into(d_rays.data_ptr(), n, m, seg.data_ptr() if m else None, lst.data_ptr() if last else None, end.data_ptr(), stream=stream, timed=timed)
    assert (ms is not None and ms >= 0.0) if timed else ms is None
    torch.cuda.synchronize()
    return hits_of(seg).reshape(max(m, 1), n)[:m], (hits_of(lst) if last else None), ends_of(end)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_composer(got, want, what=""):
    seg, last, ends = got
    wseg, wlast, wends = want
    assert paths_ref.ends_as_composer(ends, wends) and paths_ref.same_as_composer(last, wlast) and paths_ref.same_as_composer(seg, wseg), (what, paths_ref.describe(got, want))


def assert_consistent(r, rays, got, what=""):
    """On device results alone: plane 0 is rt_trace_rays' output, last is plane segments - 1, ends.object is last.object."""
    seg, last, ends = got
    assert bits_equal(seg[0], trace_dev(r, rays)), (what, "plane 0")
    assert np.array_equal(ends["object"], last["object"]), what
    n = len(rays)
    k = ends["segments"].astype(np.int64) - 1
    assert k.max() < len(seg) and k.min() >= -1
    pick = seg[np.maximum(k, 0), np.arange(n)].copy()
    pick[k < 0] = paths_ref.miss_records(1)[0]
    assert bits_equal(np.ascontiguousarray(pick), last), (what, "last")
    unreached = np.arange(len(seg))[:, None] >= ends["segments"][None, :]
    assert bits_equal(np.ascontiguousarray(seg[unreached]), paths_ref.miss_records(int(unreached.sum()))), (what, "unreached planes")


def check(pkg, r, osc, rays, what="", m=None):
    got = paths_dev(r, rays, m)
    assert_composer(got, paths_ref.paths(osc, rays, m), what)
    assert_consistent(r, rays, got, what)
    return got


# ---- the context's own primary rays ---------------------------------------------------------------------------------------------------
def primary_dev(r, cam=None, rect=None, **kw):
    out, ms = r.primary_rays(cam, rect, **kw)
    return out.cpu().numpy().reshape(-1).view(rays_ref.RAY_DTYPE)


def test_primary_rays_are_the_references(pkg, oracle):
    sc = pkg.Scene.load_from_file(scene_path("reflection_test")).set_size(64, 48)
    osc = oracle_from(pkg, oracle, sc)
    r = pkg.Renderer(sc, device=0)
    r3 = pkg.Renderer(sc, device=0, rank=1, world=3, band_rows=5)
    for cam in (None, pkg.camera_matrix(*MOVED)):
        whole = primary_dev(r, cam)
        assert bits_equal(whole, rays_ref.primary_rays(osc, cam))
        for rect in ((17, 5, 17, 5), (0, 30, 9, 47), (50, 0, 63, 11), (3, 7, 40, 29)):
            x0, y0, x1, y1 = rect
            want = rays_ref.primary_rays(osc, cam, np.arange(y0, y1 + 1), np.arange(x0, x1 + 1))
            assert bits_equal(primary_dev(r, cam, rect), want), rect
            assert bits_equal(primary_dev(r3, cam, rect), want), (rect, "a rank of three")   # any global row, whatever the rank owns
        assert bits_equal(primary_dev(r3, cam), whole)
        # the frame, the pick records and the list form of the kernel
        frame = frame_of(pkg, sc, cam)
        frame[0].cleanup_update()
        got, rec = shade_dev(r, whole, hits=True)
        assert bits_equal(got, frame[1].reshape(-1, 4))
        xy = np.stack([np.tile(np.arange(64), 48), np.repeat(np.arange(48), 64)], axis=1)
        assert bits_equal(rec, r.pick(xy, cam)) and bits_equal(trace_dev(r, whole), rec)
        some = xy[np.random.default_rng(5).permutation(len(xy))[:700]]
        seg, ends = r.pick_paths(some, cam)
        idx = some[:, 1] * 64 + some[:, 0]
        pseg, plast, pends = paths_dev(r, whole[idx])
        assert bits_equal(seg, pseg) and bits_equal(ends, pends) and bits_equal(seg[0], r.pick(some, cam))
    r.cleanup_update()
    r3.cleanup_update()
    for flags in (pkg.RT_FLAG_SSAA2, pkg.RT_FLAG_SSAA4 | pkg.RT_FLAG_SSAA_ADAPTIVE):
        rs = pkg.Renderer(sc, device=0, flags=flags)
        with pytest.raises(pkg.RtError, match="rt_primary_rays.*RT_FLAG_SSAA"):
            rs.primary_rays()
        with pytest.raises(pkg.RtError, match="rt_pick_paths.*RT_FLAG_SSAA"):
            rs.pick_paths([(1, 1)])
        rs.cleanup_update()


# ---- paths against the composer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(14))
def test_primary_rays_as_explicit_rays(pkg, oracle, case):
    what, make, moved = primary_cases(pkg)[case]
    sc = make().set_size(W, H)
    cam = pkg.camera_matrix(*MOVED) if moved else None
    osc = oracle_from(pkg, oracle, sc)
    r = pkg.Renderer(sc, device=0)
    rays = primary_dev(r, cam)
    assert bits_equal(rays, rays_ref.primary_rays(osc, cam))
    seg, last, ends = check(pkg, r, osc, rays, what)
    r.cleanup_update()
    if what == "reflection_test":
        assert {MISS, SURFACE, ESCAPED} <= set(ends["end"].tolist()) and ends["segments"].max() > 1


@pytest.mark.parametrize("name", list(ARBITRARY))
def test_arbitrary_rays(pkg, oracle, name):
    import torch
    sc = ARBITRARY[name](pkg)
    osc = oracle_from(pkg, oracle, sc)
    n = 1500
    rays = arbitrary_rays(osc, n, 5)
    r = pkg.Renderer(sc, device=0)
    seg, last, ends = check(pkg, r, osc, rays, name)
    assert (ends["end"] == MISS).sum() > n // 10 and (ends["end"] == SURFACE).sum() > n // 10 and (name != "mixed" or ends["segments"].max() > 1)
    for k in (1, 63, 64, 65, 255, 256, 257, 1000):   # partial waves and partial workgroups, at an offset so that every slice differs
        a = min(k, n - k)
        sl = slice(a, a + k)
        pseg, plast, pends = paths_dev(r, rays[sl])
        assert bits_equal(pseg, np.ascontiguousarray(seg[:, sl])) and bits_equal(plast, last[sl]) and bits_equal(pends, ends[sl]), (name, k)
    if name == "mixed":
        # more rays than one trip of the grid-stride loop (at most four workgroups of 256 rays per CU): every copy's bits equal the first's
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        reps = (256 * 4 * cus) // 1000 + 2
        big = np.tile(rays[:1000], reps)[: reps * 1000 - 37]
        assert len(big) > 256 * 4 * cus + 256
        bseg, blast, bends = paths_dev(r, big, 2)
        at = np.arange(len(big)) % 1000
        assert bits_equal(bends, ends[at]) and bits_equal(blast, last[at]) and bits_equal(bseg, np.ascontiguousarray(seg[:2, at])), (name, "grid-stride")
    r.cleanup_update()


@pytest.mark.parametrize("mirror", [False, True])
def test_derived_rays_outside_the_proven_range(pkg, oracle, mirror):
    """The 1e104 plane (the hit point leaves the proven range) and the cone's apex (the normal is NaN): the bounce goes through the dense
    expansion, finds nothing and the path escapes."""
    for osc, rays, first in ((far_plane(oracle, mirror), rays_ref.make_rays(*FAR_RAY), 1), (cone_scene(oracle, mirror), rays_ref.make_rays(*CONE_RAYS), 0)):
        r = pkg.Renderer(R.desc(pkg, osc), device=0)
        seg, last, ends = check(pkg, r, osc, rays, mirror)
        r.cleanup_update()
        assert ends[0].tolist() == ((1, ESCAPED, 0.5, first) if mirror else (1, SURFACE, 1.0, first))


@pytest.mark.parametrize("max_refl", [0, 1, 5])
def test_reflection_depths(pkg, oracle, max_refl):
    sc = depth_scene(pkg, max_refl)
    osc = oracle_from(pkg, oracle, sc)
    r = pkg.Renderer(sc, device=0)
    rays = primary_dev(r, pkg.camera_matrix(*DEPTH_CAM))
    seg, last, ends = check(pkg, r, osc, rays, max_refl)
    r.cleanup_update()
    assert ends["segments"].max() == max_refl + 1 if max_refl < 5 else ends["segments"].max() > 2
    assert max_refl == 5 or (ends["end"] == CAP).any()


def test_facing_mirrors_and_ratio_boundaries(pkg, oracle):
    rays = rays_ref.make_rays(*MIRROR_RAYS)
    for max_refl, value in ((0, 0.5), (2, 0.125), (5, 0.015625)):
        osc = facing_mirrors(oracle, max_refl)
        r = pkg.Renderer(R.desc(pkg, osc), device=0)
        seg, last, ends = check(pkg, r, osc, rays, max_refl)
        r.cleanup_update()
        assert ends.tolist() == [(max_refl + 1, CAP, value, max_refl % 2), (max_refl + 1, CAP, value, 1 - max_refl % 2)]
    for ratio, want in ((RATIO_ABOVE, (1, ESCAPED, RATIO_ABOVE, 0)), (RATIO_BELOW, (1, SURFACE, 1.0, 0)), (float("nan"), (1, SURFACE, 1.0, 0))):
        osc = ratio_scene(oracle, ratio)
        r = pkg.Renderer(R.desc(pkg, osc), device=0)
        seg, last, ends = check(pkg, r, osc, rays[:1], ratio)
        r.cleanup_update()
        assert ends[0].tolist() == want


@pytest.mark.parametrize("scale", [0.5, 2.0])
def test_unnormalised_direction_through_a_mirror(pkg, oracle, scale):
    sc = mirror_scene(pkg)
    osc = oracle_from(pkg, oracle, sc).with_size(W, H)
    rays = rays_ref.primary_rays(osc)
    rays["d"] *= scale
    r = pkg.Renderer(sc, device=0)
    seg, last, ends = check(pkg, r, osc, rays, scale)
    r.cleanup_update()
    assert np.all(seg["object"][0] == 0) and (ends["object"] == 1).any() and np.all(ends["segments"][ends["object"] == 1] == 2)   # the sphere shows in the mirror


def test_max_segments_is_a_storage_limit_only(pkg, oracle):
    sc = depth_scene(pkg, 2)
    osc = oracle_from(pkg, oracle, sc)
    r = pkg.Renderer(sc, device=0)
    rays = primary_dev(r, pkg.camera_matrix(*DEPTH_CAM))
    full = paths_dev(r, rays)
    assert len(full[0]) == 3 and (full[2]["segments"] == 3).any()
    for m in (0, 1, 3, 5):
        seg, last, ends = paths_dev(r, rays, m)
        assert bits_equal(last, full[1]) and bits_equal(ends, full[2]), m
        assert len(seg) == m and bits_equal(np.ascontiguousarray(seg[:3]), np.ascontiguousarray(full[0][:m])), m
        assert bits_equal(np.ascontiguousarray(seg[3:]), paths_ref.miss_records((max(m - 3, 0), len(rays)))), m
        nseg, none, nends = paths_dev(r, rays, m, last=False)
        assert none is None and bits_equal(nseg, seg) and bits_equal(nends, ends), (m, "without last")
    r.cleanup_update()


# ---- degree 3 ------------------------------------------------------------------------------------------------------------------------
def cubic_check(pkg, oracle, sc, osc, rays, what):
    """As cubic_check of tests/test_shade_gpu.py holds rt_shade_rays: the composer under the device's cbrt / acos / cos is the reference,
    and the rays that differ are bounded by max(3, int(0.002 * 64 * 48)).  A ray differs when its ending (segments, end, object) does, or
    a stored t by more than the 1e-5 relative of conftest.compare.  The composer under glibc is compared first, so that the share of
    the bound that libm alone takes is on record."""
    r = pkg.Renderer(sc, device=0)
    got = paths_dev(r, rays)
    r.cleanup_update()
    glibc = paths_ref.paths(osc, rays)
    ref, _, rounds = oracle.under_libm(lambda: paths_ref.paths(osc, rays), D.evaluator(D.lib(pkg)))

    def differing(a, b):
        bad = (a[2]["segments"] != b[2]["segments"]) | (a[2]["end"] != b[2]["end"]) | (a[2]["object"] != b[2]["object"])
        ta, tb = np.where(np.isfinite(a[0]["t"]), a[0]["t"], 0.0), np.where(np.isfinite(b[0]["t"]), b[0]["t"], 0.0)
        return int((bad | (np.abs(ta - tb) > 1e-5 * np.abs(tb) + 1e-7).any(axis=0)).sum())
    n_libm, n_bad = differing(glibc, ref), differing(got, ref)
    print(f"{what}: glibc composer vs device-libm composer {n_libm} differing rays; rt_trace_paths vs device-libm composer {n_bad} of {len(rays)}, libm rounds {rounds}")
    assert n_bad <= max(3, int(0.002 * 64 * 48)), (what, n_bad)
    assert (got[2]["end"] == SURFACE).any() and len(np.unique(got[0]["t"][0])) > 100   # (the cubic scene fills the view: no miss is asked for)


@pytest.mark.parametrize("name", CUBIC)
def test_shipped_scenes_of_degree_three(pkg, oracle, name):
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(64, 48)
    osc = oracle.load_scene(scene_path(name)).with_size(64, 48)
    cubic_check(pkg, oracle, sc, osc, rescaled(rays_ref.primary_rays(osc, pkg.camera_matrix((0.3, 0.2, -4.0), 90.0, 0.0)), 1), name)


@pytest.mark.parametrize("seed", range(3))
def test_random_scenes_of_degree_three(pkg, oracle, seed):
    sc, cam = random_cubic_scene(pkg, seed, 64, 48)
    osc = oracle_from(pkg, oracle, sc)
    cubic_check(pkg, oracle, sc, osc, rescaled(rays_ref.primary_rays(osc, cam), seed), f"random cubic {seed}")


# ---- contexts, frames, graphs, scene updates -----------------------------------------------------------------------------------------------
def test_every_context_kind_answers_alike(pkg, oracle):
    sc = mixed_scene(pkg, 3, w=97, h=61)
    rays = arbitrary_rays(oracle_from(pkg, oracle, sc), 500, 21)
    r = pkg.Renderer(sc, device=0)
    ref = paths_dev(r, rays)
    r.cleanup_update()
    assert ref[2]["segments"].max() > 1
    kinds = [dict(flags=pkg.RT_FLAG_SSAA2), dict(flags=pkg.RT_FLAG_SSAA4), dict(flags=pkg.RT_FLAG_SSAA4 | pkg.RT_FLAG_SSAA_ADAPTIVE),
             dict(flags=pkg.RT_FLAG_SSAA4 | pkg.RT_FLAG_SSAA_ADAPTIVE | pkg.RT_FLAG_SSAA_GEOMETRY), dict(rank=1, world=3, band_rows=5), dict(fmt=pkg.RT_FMT_RGBA8),
             dict(flags=pkg.RT_FLAG_NOCULL | pkg.RT_FLAG_SIMPLE), dict(flags=pkg.RT_FLAG_STREAM)]
    for kw in kinds:
        r = pkg.Renderer(sc, device=0, **kw)
        got = paths_dev(r, rays)
        host = r.paths(rays["o"], rays["d"])
        r.cleanup_update()
        for a, b, c in zip(got, ref, host):
            assert bits_equal(a, b) and bits_equal(c, b), kw


def test_paths_are_invisible_to_the_frames(pkg, oracle):
    sc = depth_scene(pkg, 3, seed=4242, w=160, h=90)
    views = [pkg.camera_matrix((0.0, 0.0, 0.0), 90.0, 0.0), pkg.camera_matrix(*DEPTH_CAM)]
    rays = arbitrary_rays(oracle_from(pkg, oracle, sc), 1000, 8)
    count = pkg.RT_FLAG_STRICT | pkg.RT_FLAG_COUNT
    fresh = pkg.Renderer(sc, device=0, flags=count)
    want = []
    for cam in views:
        fresh.update(cam)
        want.append((fresh.download().copy(), fresh.counters(), [t.cpu().numpy() for t in fresh.gbuffer(cam)[:3]]))
    ref = paths_dev(fresh, rays)
    fresh.cleanup_update()
    r = pkg.Renderer(sc, device=0, flags=count)
    for cam, (frame, cnt, planes) in zip(views, want):
        assert all(bits_equal(a, b) for a, b in zip(paths_dev(r, rays), ref))
        r.update(cam)
        assert all(bits_equal(a, b) for a, b in zip(paths_dev(r, rays, timed=False), ref))
        assert bits_equal(r.download(), frame) and booked(r.counters()) == booked(cnt)   # RT_FLAG_COUNT books none of the paths' rays
        assert all(bits_equal(t.cpu().numpy(), p) for t, p in zip(r.gbuffer(cam)[:3], planes))
    r.cleanup_update()
    assert want[0][1]["primary_rays"] == 160 * 90


def test_primary_rays_paths_and_colours_in_one_graph(pkg, oracle):
    import torch
    sc = depth_scene(pkg, 2)
    r = pkg.Renderer(sc, device=0)
    cam = pkg.camera_matrix(*DEPTH_CAM)
    n, m = W * H, 3
    rays = primary_dev(r, cam)
    plain, colours = paths_dev(r, rays), shade_dev(r, rays)[0]
    s = torch.cuda.Stream()
    d_rays = torch.zeros((n, 6), dtype=torch.float64, device="cuda:0")
    seg, lst = torch.zeros((m * n, 6), dtype=torch.float64, device="cuda:0"), torch.zeros((n, 6), dtype=torch.float64, device="cuda:0")
    end, rgba = torch.zeros((n, 4), dtype=torch.int32, device="cuda:0"), torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):   # one stream: the three kernels form a single chain
        r.primary_rays_into(cam, None, d_rays.data_ptr(), stream=s.cuda_stream, timed=False)
        r.paths_into(d_rays.data_ptr(), n, m, seg.data_ptr(), lst.data_ptr(), end.data_ptr(), stream=s.cuda_stream, timed=False)
        r.shade_into(d_rays.data_ptr(), n, rgba.data_ptr(), stream=s.cuda_stream, timed=False)
    for _ in range(2):
        for t in (d_rays, seg, lst, end, rgba):
            t.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert bits_equal(d_rays.cpu().numpy().reshape(-1).view(rays_ref.RAY_DTYPE), rays)
        assert bits_equal(hits_of(seg).reshape(m, n), plain[0]) and bits_equal(hits_of(lst), plain[1]) and bits_equal(ends_of(end), plain[2])
        assert bits_equal(rgba.cpu().numpy(), colours)
    r.cleanup_update()


def test_after_a_scene_update_the_paths_are_the_new_scenes(pkg, oracle):
    sc = depth_scene(pkg, 2)
    osc = oracle_from(pkg, oracle, sc)
    r = pkg.Renderer(sc, device=0)
    rays = primary_dev(r, pkg.camera_matrix(*DEPTH_CAM))
    before = check(pkg, r, osc, rays, "before")
    moved = R.copy_scene(osc)
    refl = osc.reflection.copy()
    assert (refl > 1e-7).any()
    refl[refl > 1e-7] *= np.float32(0.5)   # every mirror stays a mirror: the layout rule holds
    for ob, v in zip(moved.objects, refl):
        ob.reflection_ratio = float(v)
    r.set_scene(reflection=refl)
    after = check(pkg, r, moved, rays, "after")
    r.cleanup_update()
    assert not bits_equal(after[2], before[2]) and np.array_equal(after[2]["segments"], before[2]["segments"])


# ---- picking through mirrors, the host entry points, refusals, the FAST build -------------------------------------------------------------
def update_lib(pkg):
    upd = C.CDLL(pkg.UPDATE_LIB_PATH)
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
    update = getattr(upd, re.search(r"\b(_Z\d*6updateRKN3glm\w+)\b", names).group(1))
    cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
    init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
    update.argtypes, update.restype = [C.c_void_p], C.c_float
    upd.mi355rt_update_pick_path.argtypes = [C.c_uint, C.c_uint, C.POINTER(pkg.Hit), C.c_uint, C.POINTER(pkg.PathEnd)]
    return upd, init, update, cleanup


def test_pick_through_the_mirror(pkg, oracle):
    """The mirror plane of mirror_scene fills the view and the sphere stands behind the camera: rt_pick reports the mirror for the centre
    pixel, the path reports the sphere.  Also through mi355rt_update_pick_path of libmi355rt_update.so (ctypes, as
    tests/test_shade_gpu.py drives mi355rt_update_shade)."""
    sc = mirror_scene(pkg)
    r = pkg.Renderer(sc, device=0)
    xy = [(32, 24), (0, 0), (63, 47)]
    seg, ends = r.pick_paths(xy)
    pick = r.pick(xy)
    assert seg.shape == (5, 3) and bits_equal(seg[0], pick) and pick["object"].tolist() == [0, 0, 0]
    assert ends[0].tolist()[:2] == (2, SURFACE) and ends["object"][0] == 1 and seg["object"][1, 0] == 1 and ends["ratio"][0] == F(0.9)
    assert ends[1].tolist()[:2] == (1, ESCAPED) and ends["object"][1] == 0
    none, ends0 = r.pick_paths(xy, max_segments=0)
    assert none.shape == (0, 3) and bits_equal(ends0, ends)
    r.cleanup_update()
    upd, init, update, cleanup = update_lib(pkg)
    out, end = (pkg.Hit * 5)(), pkg.PathEnd()
    assert upd.mi355rt_update_pick_path(32, 24, out, 5, C.byref(end)) == -1
    init(42, sc._h)
    try:
        assert upd.mi355rt_update_pick_path(32, 24, out, 5, C.byref(end)) == -1 and b"no update() call yet" in pkg.lib().rt_last_error()
        cam = np.ascontiguousarray(pkg.IDENTITY, dtype=np.float64)
        update(cam.ctypes.data_as(C.c_void_p))
        assert upd.mi355rt_update_pick_path(32, 24, out, 5, C.byref(end)) == 0, pkg.lib().rt_last_error()
    finally:
        cleanup()
    got = np.frombuffer(bytes(out), dtype=rays_ref.HIT_DTYPE)
    assert bits_equal(got, np.ascontiguousarray(seg[:, 0])) and (end.segments, end.end, end.object) == (2, SURFACE, 1)


def test_refusals(pkg):
    import torch
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(W, H)
    r = pkg.Renderer(sc, device=0)
    bufs = [torch.zeros((64, 6), dtype=torch.float64, device="cuda:0") for _ in range(4)]
    p, s, l, e = (b.data_ptr() for b in bufs)

    def refused(call, *words):
        with pytest.raises(pkg.RtError) as err:
            call()
        assert err.value.code == -1 and any(w in str(err.value) for w in words) and "rt_" in str(err.value), str(err.value)
    refused(lambda: r.paths_into(None, 4, 1, s, l, e), "null")
    refused(lambda: r.paths_into(p, 4, 0, None, l, None), "null")
    refused(lambda: r.paths_into(p, 0, 1, s, l, e), "n is 0")
    refused(lambda: r.paths_into(p, 4, 65, s, l, e), "exceeds 64")
    refused(lambda: r.paths_into(p, 4, 1, None, l, e), "if and only if")
    refused(lambda: r.paths_into(p, 4, 0, s, l, e), "if and only if")
    for bad in range(4):
        a = [p, s, l, e]
        a[bad] += 8
        refused(lambda: r.paths_into(a[0], 4, 1, a[1], a[2], a[3]), "aligned")
    refused(lambda: r.paths_into(p, 8, 1, p + 48 * 7, l, e), "overlap")        # segments over the rays
    refused(lambda: r.paths_into(p, 8, 2, s, s + 48 * 15, e), "overlap")       # last inside the second plane
    refused(lambda: r.paths_into(p, 8, 1, s, l, l + 48 * 7), "overlap")        # ends over last
    refused(lambda: r.paths_into(p, 8, 1, s, None, p + 16), "overlap")         # ends inside the rays
    r.paths_into(p, 8, 2, p + 48 * 8, p + 48 * 24, p + 48 * 32)                # adjacent ranges are fine
    refused(lambda: r.paths(np.zeros((0, 3)), np.zeros((0, 3))), "n is 0")
    refused(lambda: r.primary_rays_into(None, None, None), "null")
    refused(lambda: r.primary_rays_into(None, None, p + 8), "aligned")
    refused(lambda: r.primary_rays_into(None, (3, 0, 2, 0), p), "not a rectangle")
    refused(lambda: r.primary_rays_into(None, (0, 0, W, 0), p), "inside the")
    refused(lambda: r.pick_paths([(W, 0)]), "outside")
    refused(lambda: r.pick_paths([(0, 0)], max_segments=65), "exceeds 64")
    refused(lambda: r.pick_paths(np.zeros((0, 2))), "n is 0")
    r.cleanup_update()


def test_fast_build_statistics(pkg, oracle):
    """FAST against strict on the primary rays of three scenes: only what holds by construction is asserted -- a ray that misses in both
    builds has end == MISS in both, and segments <= max_reflections + 1 -- and the differing endings are printed."""
    for name in ("20spheres", "reflection_test", "clebsch"):
        w, h = 160, 90
        sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
        ra, rb = pkg.Renderer(sc, device=0), pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_FAST)
        rays = primary_dev(ra)
        a, b = paths_dev(ra, rays), paths_dev(rb, rays)
        ta, tb = trace_dev(ra, rays), trace_dev(rb, rays)
        ra.cleanup_update()
        rb.cleanup_update()
        both_miss = (ta["object"] < 0) & (tb["object"] < 0)
        assert both_miss.any() and np.all(a[2]["end"][both_miss] == MISS) and np.all(b[2]["end"][both_miss] == MISS)
        assert b[2]["segments"].max() <= sc.desc().max_reflections + 1 and a[2]["segments"].max() <= sc.desc().max_reflections + 1
        print(f"FAST vs strict rt_trace_paths, {name} {w}x{h}: end differs at {int((a[2]['end'] != b[2]['end']).sum())}, object at "
              f"{int((a[2]['object'] != b[2]['object']).sum())}, segments at {int((a[2]['segments'] != b[2]['segments']).sum())} of {len(rays)} rays")
