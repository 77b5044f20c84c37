"""The primary-hit G-buffer and pixel picking on the GPU (rt_render_gbuffer / rt_pick, csrc/rt_gbuffer.hip)
against the reference composer tests/tools/gbuffer_ref.py.  Surfaces of degree <= 2, strict build: every comparison is on the raw bits
(`t` as uint64, normals as uint32, so +inf and signed zeros count)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, compare, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gbuffer_ref  # noqa: E402
import cubic_device_lab as D  # noqa: E402  (the oracle under the device's cbrt / acos / cos)
from test_gpu_parity import QUADRIC, CUBIC, mixed_scene, oracle_from, random_cubic_scene, random_scene  # noqa: E402

pytestmark = pytest.mark.gpu

MOVED = ((0.4, 0.3, -1.5), 84.0, -3.0)   # a moved camera: position, yaw, pitch


def planes(pkg, sc, cam=None, **kw):
    """(object, t, normal) of a fresh context as numpy arrays."""
    r = pkg.Renderer(sc, device=0, **kw)
    o, t, n, ms = r.gbuffer(cam)
    out = (o.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy())
    r.cleanup_update()
    assert ms is not None and ms >= 0.0
    return out


def same_bits(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and
            np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))


def assert_exact(got, ref, what=""):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.float32 and got[2].shape[-1] == 4
    assert np.array_equal(got[0], ref["object"]), (what, "object", int((got[0] != ref["object"]).sum()))
    assert np.array_equal(got[1].view(np.uint64), ref["t"].view(np.uint64)), (what, "t", int((got[1].view(np.uint64) != ref["t"].view(np.uint64)).sum()))
    assert np.array_equal(got[2].view(np.uint32), ref["normal"].view(np.uint32)), (what, "normal", int((got[2].view(np.uint32) != ref["normal"].view(np.uint32)).any(axis=-1).sum()))


def check_scene(pkg, oracle, sc, cam=None, what="", **kw):
    got = planes(pkg, sc, cam, **kw)
    ref = gbuffer_ref.compose(oracle_from(pkg, oracle, sc), cam)
    assert_exact(got, ref, what)
    return got, ref


@pytest.mark.parametrize("name", QUADRIC)
def test_shipped_scenes_of_degree_two(pkg, oracle, name):
    """96 x 72 from the start pose and from a moved camera, a size that is no multiple of 16 or 8, and a single pixel."""
    for w, h, cam in ((96, 72, None), (96, 72, pkg.camera_matrix(*MOVED)), (97, 61, None), (1, 1, None)):
        sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
        got, ref = check_scene(pkg, oracle, sc, cam, what=(name, w, h))
        if (w, h) == (96, 72):
            assert (got[0] >= 0).any() and (got[0] < 0).any()


def fuzz_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tests", "tools", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    return fz


@pytest.mark.parametrize("seed", range(14))
def test_random_sphere_fields(pkg, oracle, seed):
    """Up to 150 spheres (three culling chunks) with and without a plane, moved cameras; seed 13 has no object at all."""
    n = [3, 8, 20, 40, 70, 130, 150][seed % 7]
    if seed == 13:
        sc = pkg.Scene.new(40, 30, 50.0, 2, (0.3, 0.6, 0.9))
        sc.add_light("directional", [0, -1, 0])
    else:
        sc = random_scene(pkg, 300 + seed, n, 1 + seed % 3, w=40, h=30, with_plane=seed % 2 == 0, mirrors=seed % 3 == 0)
    cam = oracle.camera_matrix(pos=(seed * 0.3 - 1.0, 0.5, -4.0), yaw_deg=90.0 + 2 * seed, pitch_deg=-3.0 + seed) if seed % 3 else None
    got, _ = check_scene(pkg, oracle, sc, cam, what=seed)
    if seed == 13:
        assert np.all(got[0] == -1) and np.all(np.isposinf(got[1])) and not got[2].any()
    elif n > 64:
        assert len(np.unique(got[0])) > 5
    assert same_bits(got, planes(pkg, sc, cam, flags=pkg.RT_FLAG_NOCULL))


@pytest.mark.parametrize("seed", range(14))
def test_random_mixed_class_scenes(pkg, oracle, seed):
    sc = mixed_scene(pkg, seed, w=48, h=36)
    cam = pkg.camera_matrix(pos=(0.3 * (seed % 5) - 0.6, 0.2 * (seed % 3), -1.0 * (seed % 4)), yaw_deg=90.0 + (seed % 7) - 3, pitch_deg=(seed % 5) - 2.0)
    check_scene(pkg, oracle, sc, cam, what=seed)


@pytest.mark.parametrize("seed", [158, 534] + list(range(2000, 2012)))
def test_fuzz_parity_scenes(pkg, oracle, seed):
    """tests/tools/fuzz_parity.py scenes: odd image sizes down to one pixel, scene scales 0.1 .. 100, huge / tiny / imaginary spheres,
    quadrics, planes, random cameras; 158 and 534 are the two scenes with block cones wider than a half-space."""
    sc, cam = fuzz_module().scene(seed)
    check_scene(pkg, oracle, sc, cam, what=seed)


def test_edge_scenes(pkg, oracle):
    W, H = 48, 36
    bg = (0.1, 0.1, 0.1)
    # two identical spheres: the lowest index wins
    s = pkg.Scene.new(W, H, 50.0, 2, bg)
    for _ in range(2):
        s.add_object(pkg.surface_make("sphere", [0.5, 0.2, 9], [2.0]), (1, 1, 1))
    got, _ = check_scene(pkg, oracle, s, what="twins")
    assert set(np.unique(got[0]).tolist()) == {-1, 0}
    # camera inside a sphere (normals point away from the eye: never flipped), a sphere behind the camera, one in front
    s = pkg.Scene.new(W, H, 60.0, 2, bg)
    s.add_object(pkg.surface_make("sphere", [0, 0, 0], [50.0]), (0.9, 0.8, 0.7))
    s.add_object(pkg.surface_make("sphere", [0, 0, -8], [2.0]), (0.9, 0.8, 0.7))
    s.add_object(pkg.surface_make("sphere", [1, 0, 8], [1.0]), (0.2, 0.9, 0.2))
    got, ref = check_scene(pkg, oracle, s, what="inside")
    assert set(np.unique(got[0]).tolist()) == {0, 2}
    inside = got[0] == 0
    assert np.all((got[2][inside][:, :3].astype(np.float64) * ref["dir"][inside]).sum(axis=-1) > 0.0)
    # a plane seen edge-on (it contains the eye and the viewing direction) over a floor
    s = pkg.Scene.new(W, H, 50.0, 2, bg)
    s.add_object(pkg.surface_make("plane", [0, 0, 0], [0, 1, 0]), (1, 1, 1))
    s.add_object(pkg.surface_make("plane", [0, 0, 0], [1, 0, 0]), (1, 1, 1))
    s.add_object(pkg.surface_make("plane", [0, -2, 0], [0, 1, 0]), (1, 1, 1))
    check_scene(pkg, oracle, s, what="edge-on")
    check_scene(pkg, oracle, s.set_size(W + 1, H + 1), what="edge-on, odd size (a pixel row and column through the planes)")
    # a hit beyond MAX_T is a miss
    s = pkg.Scene.new(W, H, 50.0, 2, bg)
    s.add_object(pkg.surface_make("sphere", [0, 0, 2.0e6], [5.0e5]), (1, 1, 1))
    s.add_object(pkg.surface_make("sphere", [3.0e5, 0, 9.0e5], [1.0e5]), (1, 1, 1))
    got, _ = check_scene(pkg, oracle, s, what="far")
    assert set(np.unique(got[0]).tolist()) == {-1, 1}
    # coordinates near 1e6 (cf. test_huge_coordinates_do_not_break_culling)
    rng = np.random.default_rng(3)
    off = np.array([1.0e6, -2.0e6, 3.0e6])
    s = pkg.Scene.new(W, H, 50.0, 2, bg)
    for i in range(12):
        s.add_object(pkg.surface_make("sphere", rng.uniform([-8, -5, 8], [8, 5, 30]) + off, [float(rng.uniform(0.5, 2.5))]), rng.uniform(0, 1, 3))
    cam = np.eye(4).reshape(16).copy()
    cam[12:15] = off
    got, _ = check_scene(pkg, oracle, s, cam, what="huge")
    assert len(np.unique(got[0])) > 4
    # a mirror shows itself, not what it reflects
    s = pkg.Scene.new(W, H, 50.0, 4, bg)
    s.add_object(pkg.surface_make("plane", [0, 0, 12], [0, 0, -1]), (0.9, 0.9, 0.9), 0.9)
    s.add_object(pkg.surface_make("sphere", [0, 0, -6], [2.0]), (0.9, 0.1, 0.1))
    s.add_light("directional", [0, -1, 1])
    got, _ = check_scene(pkg, oracle, s, what="mirror")
    assert np.all(got[0] == 0)


def cubic_check(pkg, oracle, sc, osc, cam, what):
    got = planes(pkg, sc, cam)
    ref, _, rounds = oracle.under_libm(lambda: gbuffer_ref.compose(osc, cam), D.evaluator(D.lib(pkg)))
    nobj = int((got[0] != ref["object"]).sum())
    hit = ref["object"] >= 0
    rel = np.abs(got[1][hit] - ref["t"][hit]) / np.abs(ref["t"][hit])
    c = compare(got[2], ref["normal"])
    print(f"{what}: object differs at {nobj} pixels, max rel t {float(rel.max()) if rel.size else 0.0:.3e}, normals {c}, libm rounds {rounds}")
    assert nobj == 0, what
    assert np.array_equal(np.isposinf(got[1]), ~hit)
    assert np.all(rel <= 1e-8), (what, float(rel.max()))
    assert c["n_bad_pixels"] == 0, (what, c)


@pytest.mark.parametrize("name", CUBIC)
def test_shipped_scenes_of_degree_three(pkg, oracle, name):
    w, h = 64, 48
    for cam in (None, pkg.camera_matrix((0.3, 0.2, -4.0), 90.0, 0.0)):
        cubic_check(pkg, oracle, pkg.Scene.load_from_file(scene_path(name)).set_size(w, h), oracle.load_scene(scene_path(name)).with_size(w, h), cam, name)


@pytest.mark.parametrize("seed", range(6))
def test_random_scenes_of_degree_three(pkg, oracle, seed):
    sc, cam = random_cubic_scene(pkg, seed, 64, 48)
    cubic_check(pkg, oracle, sc, oracle_from(pkg, oracle, sc), cam, f"random cubic {seed}")


@pytest.mark.parametrize("world,band", [(3, 5), (4, 1)])
def test_ranks_place_their_rows_by_row_map(pkg, world, band):
    w, h = 97, 61
    sc = random_scene(pkg, 99, 14, 3, w=w, h=h)
    cam = pkg.camera_matrix(*MOVED)
    full = planes(pkg, sc, cam)
    built = (np.full((h, w), -7, np.int32), np.full((h, w), np.nan), np.full((h, w, 4), np.nan, np.float32))
    for rank in range(world):
        r = pkg.Renderer(sc, device=0, rank=rank, world=world, band_rows=band)
        rows = r.row_map()
        o, t, n, _ = r.gbuffer(cam)
        assert o.shape == (len(rows), w) and t.shape == (len(rows), w) and n.shape == (len(rows), w, 4)
        for dst, src in zip(built, (o, t, n)):
            dst[rows] = src.cpu().numpy()
        r.cleanup_update()
    assert same_bits(built, full)


def test_every_subset_of_planes_writes_only_what_was_asked_for(pkg):
    import torch
    w, h = 97, 61
    sc = pkg.Scene.load_from_file(scene_path("quadratic")).set_size(w, h)
    full = planes(pkg, sc)
    r = pkg.Renderer(sc, device=0)
    sizes = (w * h * 4, w * h * 8, w * h * 16)
    for mask in range(1, 8):
        bufs = [torch.full((nb + 64,), 0xAB, dtype=torch.uint8, device="cuda:0") for nb in sizes]
        ptrs = [b.data_ptr() if mask & (1 << i) else None for i, b in enumerate(bufs)]
        r.gbuffer_into(None, *ptrs)
        torch.cuda.synchronize()
        for i, (b, nb) in enumerate(zip(bufs, sizes)):
            host = b.cpu().numpy()
            assert np.all(host[nb:] == 0xAB), (mask, i, "guard bytes")
            if mask & (1 << i):
                assert np.array_equal(host[:nb], np.ascontiguousarray(full[i]).view(np.uint8).reshape(-1)), (mask, i)
            else:
                assert np.all(host[:nb] == 0xAB), (mask, i, "a plane that was not asked for was written")
    with pytest.raises(pkg.RtError) as e:
        r.gbuffer_into(None, None, None, None)
    assert e.value.code == -1 and "null" in str(e.value)
    r.cleanup_update()


def test_planes_do_not_depend_on_format_or_kernel_flags(pkg):
    cam = pkg.camera_matrix(*MOVED)
    for sc in (pkg.Scene.load_from_file(scene_path("20spheres")).set_size(97, 61), mixed_scene(pkg, 3, w=97, h=61)):
        ref = planes(pkg, sc, cam)
        assert same_bits(ref, planes(pkg, sc, cam, fmt=pkg.RT_FMT_RGBA8))
        for fl in (pkg.RT_FLAG_SIMPLE, pkg.RT_FLAG_NOLEAN, pkg.RT_FLAG_NOCULL, pkg.RT_FLAG_COUNT, pkg.RT_FLAG_STATIC_ORDER | pkg.RT_FLAG_NOSCAN):
            assert same_bits(ref, planes(pkg, sc, cam, flags=fl)), fl


def test_the_pass_is_invisible_to_the_frames_and_to_itself(pkg):
    """render, gbuffer, render (cut camera), gbuffer, render: the colour frames equal the same three renders of a fresh context, and a
    pose's G-buffer is the same before and after other poses and on a second stream."""
    import torch
    w, h = 320, 180
    sc = random_scene(pkg, 4242, 40, 4, w=w, h=h, with_plane=False)
    front, away, side = pkg.camera_matrix((0.0, 0.0, 0.0), 90.0, 0.0), pkg.camera_matrix((0.0, 0.0, 0.0), -90.0, 0.0), pkg.camera_matrix((14.0, 2.0, 20.0), 160.0, -5.0)
    fresh = pkg.Renderer(sc, device=0)
    want = []
    for cam in (front, away, side):
        fresh.update(cam)
        want.append(fresh.download().copy())
    fresh.cleanup_update()
    r = pkg.Renderer(sc, device=0)
    frames, gbs = [], []

    def gb(cam, stream=None):
        o, t, n, _ = r.gbuffer(cam, stream=stream.cuda_stream if stream else None, timed=stream is None)
        if stream:
            stream.synchronize()
        return o.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy()
    r.update(front)
    frames.append(r.download().copy())
    gbs.append(gb(front))
    r.update(away)
    frames.append(r.download().copy())
    gbs.append(gb(side))
    r.update(side)
    frames.append(r.download().copy())
    for a, b in zip(frames, want):
        assert np.array_equal(a, b)
    s2 = torch.cuda.Stream()
    assert same_bits(gbs[0], gb(front)) and same_bits(gbs[1], gb(side)) and same_bits(gbs[0], gb(front, s2)) and same_bits(gbs[1], gb(side, s2))
    assert not same_bits(gbs[0], gbs[1])
    r.update(front)
    assert np.array_equal(r.download(), want[0])
    r.cleanup_update()


def test_three_passes_captured_into_one_graph(pkg):
    import torch
    w, h = 320, 180
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(w, h)
    cams = [None, pkg.camera_matrix(*MOVED), pkg.camera_matrix((0.5, 0.0, 1.0), 95.0, 3.0)]
    r = pkg.Renderer(sc, device=0)
    s = torch.cuda.Stream()
    plain = []
    for cam in cams:
        o, t, n, _ = r.gbuffer(cam, stream=s.cuda_stream, timed=False)
        s.synchronize()
        plain.append((o.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy()))
    bufs = [(torch.zeros((h, w), dtype=torch.int32, device="cuda:0"), torch.zeros((h, w), dtype=torch.float64, device="cuda:0"),
             torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")) for _ in cams]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for cam, (o, t, n) in zip(cams, bufs):
            r.gbuffer_into(cam, o.data_ptr(), t.data_ptr(), n.data_ptr(), stream=s.cuda_stream, timed=False)
    g.replay()
    torch.cuda.synchronize()
    for want, (o, t, n) in zip(plain, bufs):
        assert same_bits((o.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy()), want)
    assert not same_bits(plain[0], plain[1])
    r.cleanup_update()


def pick_tuple(rec):
    return rec["object"], rec["t"], rec["normal"]


@pytest.mark.parametrize("name", ["20spheres", "quadratic", "clebsch"])
@pytest.mark.parametrize("fast", [False, True])
def test_pick_equals_the_planes(pkg, oracle, name, fast):
    """200 random pixels: object, t and normal of rt_pick are the planes' entries bit for bit, in the strict and in the FAST build (one
    per-lane function); strict, degree <= 2: `point` is o + t * d of the composer, bit for bit."""
    w, h = 96, 72
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
    cam = pkg.camera_matrix(*MOVED) if name != "clebsch" else None
    fl = pkg.RT_FLAG_FAST if fast else 0
    r = pkg.Renderer(sc, device=0, flags=fl)
    o, t, n, _ = r.gbuffer(cam)
    o, t, n = o.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy()
    rng = np.random.default_rng(11)
    xy = np.stack([rng.integers(0, w, 200), rng.integers(0, h, 200)], axis=1)
    rec = r.pick(xy, cam)
    assert rec.dtype == pkg.HIT_DTYPE and len(rec) == 200
    x, y = xy[:, 0], xy[:, 1]
    assert np.array_equal(rec["object"], o[y, x])
    assert np.array_equal(rec["t"].view(np.uint64), t[y, x].view(np.uint64))
    assert np.array_equal(rec["normal"].view(np.uint32), n[y, x, :3].view(np.uint32))
    miss = rec["object"] < 0
    assert miss.any() and (~miss).any()
    assert not rec["point"][miss].any() and not rec["normal"][miss].any()
    if not fast and name != "clebsch":
        osc = oracle.load_scene(scene_path(name)).with_size(w, h)
        for i in range(0, 200, 4):
            ref = gbuffer_ref.compose(osc, cam, rows=[y[i]], cols=[x[i]])
            assert rec["object"][i] == ref["object"][0, 0]
            assert np.array_equal(rec["point"][i].view(np.uint64), ref["point"][0, 0].view(np.uint64)), i
    # n = 1 and n = 5000 (all pixels of the frame's first 5000 in row order)
    one = r.pick([(int(x[0]), int(y[0]))], cam)
    assert one.tobytes() == rec[:1].tobytes()
    idx = np.arange(5000)
    many = r.pick(np.stack([idx % w, idx // w], axis=1), cam)
    assert np.array_equal(many["object"], o.reshape(-1)[:5000]) and np.array_equal(many["t"].view(np.uint64), t.reshape(-1)[:5000].view(np.uint64))
    assert np.array_equal(many["normal"].view(np.uint32), n.reshape(-1, 4)[:5000, :3].view(np.uint32))
    r.cleanup_update()


def test_pick_reaches_rows_the_rank_does_not_own_and_refuses_bad_calls(pkg):
    w, h = 96, 72
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(w, h)
    full = planes(pkg, sc)
    r = pkg.Renderer(sc, device=0, rank=1, world=3, band_rows=5)
    foreign = np.setdiff1d(np.arange(h), r.row_map())
    xy = np.array([(x, y) for y in foreign[::3] for x in range(0, w, 7)])
    rec = r.pick(xy)
    assert np.array_equal(rec["object"], full[0][xy[:, 1], xy[:, 0]]) and np.array_equal(rec["t"].view(np.uint64), full[1][xy[:, 1], xy[:, 0]].view(np.uint64))
    assert (rec["object"] >= 0).any()
    for bad in ([(w, 0)], [(0, h)], [(3, 3), (w, 3)], [(0xFFFFFFFF, 0)]):
        with pytest.raises(pkg.RtError) as e:
            r.pick(bad)
        assert e.value.code == -1 and "outside" in str(e.value)
    with pytest.raises(pkg.RtError) as e:
        r.pick(np.zeros((0, 2), dtype=np.uint32))
    assert e.value.code == -1
    r.cleanup_update()
    for fl in (pkg.RT_FLAG_SSAA2, pkg.RT_FLAG_SSAA4, pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA_ADAPTIVE):
        r = pkg.Renderer(sc, device=0, flags=fl)
        with pytest.raises(pkg.RtError) as e:
            r.pick([(1, 1)])
        assert e.value.code == -1 and "SSAA" in str(e.value)
        with pytest.raises(pkg.RtError) as e:
            r.gbuffer()
        assert e.value.code == -1 and "SSAA" in str(e.value)
        r.cleanup_update()


def test_fast_build_statistics(pkg):
    """FAST against strict is not asserted beyond shapes (the reference of a FAST context is its own arithmetic); the numbers printed
    here are the ones in DESIGN.md section 12."""
    for name in ("20spheres", "quadratic", "clebsch"):
        sc = pkg.Scene.load_from_file(scene_path(name)).set_size(480, 270)
        a, b = planes(pkg, sc), planes(pkg, sc, flags=pkg.RT_FLAG_FAST)
        assert all(x.shape == y.shape and x.dtype == y.dtype for x, y in zip(a, b))
        both = (a[0] >= 0) & (b[0] >= 0)
        rel = np.abs(a[1][both] - b[1][both]) / np.abs(a[1][both])
        print(f"FAST vs strict, {name} 480x270: object differs at {int((a[0] != b[0]).sum())} pixels, max rel t difference {float(rel.max()):.3e}, "
              f"normals not bit-equal at {int((a[2].view(np.uint32) != b[2].view(np.uint32)).any(axis=-1).sum())} pixels")


def test_full_size(pkg, oracle):
    """20spheres at 1920 x 1080 without reflections: the pixels with an object are the hits of a counting render of the same context
    (rt_counters.hits is held to the oracle by test_counters_fuzz_gpu.py), and 64 rows spread over the frame equal the composer."""
    w, h = 1920, 1080
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(w, h).set_max_reflections(0)
    r = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_COUNT)
    r.update()
    hits = r.counters()["hits"]
    o, t, n, ms = r.gbuffer()
    r.cleanup_update()
    o, t, n = o.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy()
    assert int((o >= 0).sum()) == hits > 0
    rows = np.unique(np.concatenate([np.linspace(0, h - 1, 62).astype(np.int64), [539, 540]]))
    assert len(rows) == 64
    ref = gbuffer_ref.compose(oracle.load_scene(scene_path("20spheres")).with_size(w, h, 0), rows=rows)
    assert (ref["object"] >= 0).sum() > 10000
    assert_exact((o[rows], t[rows], n[rows]), ref, "1080p rows")


def test_pick_driver_through_update_h(pkg):
    """tests/host_driver/pick_driver.cpp (scene.h + update.h + mi355rt_update_pick): the printed bits are Renderer.pick's."""
    w, h = 96, 72
    sc = pkg.Scene.load_from_file(scene_path("quadratic")).set_size(w, h)
    r = pkg.Renderer(sc, device=0)
    xy = [(48, 36), (10, 60), (80, 12)]
    rec = r.pick(xy)
    r.cleanup_update()
    assert (rec["object"] >= 0).any()
    args = [str(v) for p in xy for v in p]
    out = subprocess.run([pkg.PICK_DRIVER_PATH, scene_path("quadratic"), str(w), str(h)] + args + [str(w), "0"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 4 and lines[3].split()[2:] == ["refused", "-1"]
    for line, p, want in zip(lines, xy, rec):
        f = line.split()
        assert (int(f[0]), int(f[1])) == p and int(f[2]) == want["object"]
        vals = np.array([float.fromhex(v) for v in f[3:]])
        assert np.array_equal(vals[:4].view(np.uint64), np.concatenate([[want["t"]], want["point"]]).view(np.uint64))
        assert np.array_equal(vals[4:].astype(np.float32).view(np.uint32), want["normal"].view(np.uint32))
    env = dict(os.environ, MI355RT_DEVICES="0,0")
    out = subprocess.run([pkg.PICK_DRIVER_PATH, scene_path("quadratic"), str(w), str(h), "48", "36"], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and out.stdout.split()[2:] == ["refused", "-1"], (out.stdout, out.stderr)   # the multi-GPU layer has no pick
