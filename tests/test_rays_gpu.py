"""Ray queries on the GPU (rt_trace_rays / rt_occluded_rays / rt_trace_rays_host, csrc/rt_rays.hip) against the
reference composer tests/tools/rays_ref.py.  Strict contexts unless said otherwise; every comparison is on the raw bits (integer
views, so +inf, NaN and signed zeros count) unless said otherwise."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, compare, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gbuffer_ref  # noqa: E402
import rays_ref  # noqa: E402
import cubic_device_lab as D  # noqa: E402  (the oracle under the device's cbrt / acos / cos)
from test_gpu_parity import QUADRIC, CUBIC, mixed_scene, oracle_from, random_cubic_scene, random_scene  # noqa: E402

pytestmark = pytest.mark.gpu

MOVED = ((0.4, 0.3, -1.5), 84.0, -3.0)   # a moved camera: position, yaw, pitch
W, H = 64, 48


def to_device(rays):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float64).reshape(-1, 6)).to("cuda:0")


def hits_of(tensor):
    return tensor.cpu().numpy().reshape(-1).view(rays_ref.HIT_DTYPE)


def trace_dev(r, rays, stream=None, timed=True):
    """rt_trace_rays on device tensors: HIT_DTYPE records."""
    import torch
    d_rays = to_device(rays)
    out = torch.full((len(rays), 6), float("nan"), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ms = r.trace_into(d_rays.data_ptr(), len(rays), out.data_ptr(), stream=stream, timed=timed)
    assert (ms is not None and ms >= 0.0) if timed else ms is None
    torch.cuda.synchronize()
    return hits_of(out)


def occluded_dev(r, rays, t_max=None):
    out, ms = r.occluded(rays["o"], rays["d"], t_max)
    assert ms >= 0.0 and out.dtype.itemsize == 4
    return out.cpu().numpy()


def assert_records(got, want, what=""):
    assert got.dtype == rays_ref.HIT_DTYPE and rays_ref.same_records(got, want), (what, rays_ref.describe_difference(got, want))


def sphere_field(pkg, n=70):
    rng = np.random.default_rng(77)
    s = pkg.Scene.new(W, H, 60.0, 2, (0.1, 0.1, 0.1))
    for _ in range(n):
        s.add_object(pkg.surface_make("sphere", rng.uniform([-10, -7, 6], [10, 7, 30]), [float(rng.uniform(0.3, 1.5))]), rng.uniform(0, 1, 3))
    s.add_light("directional", [0, -1, 0.3])
    return s


def primary_cases(pkg):
    cases = [(name, lambda name=name: pkg.Scene.load_from_file(scene_path(name)).set_size(W, H), True) for name in QUADRIC]
    cases += [(f"random {seed}", lambda seed=seed: random_scene(pkg, 700 + seed, [3, 8, 20, 12, 5, 16][seed], 1 + seed % 3, w=W, h=H, with_plane=seed % 2 == 0), seed % 2 == 1)
              for seed in range(6)]
    cases.append(("70 spheres", lambda: sphere_field(pkg), False))
    cases += [(f"mixed {seed}", lambda seed=seed: mixed_scene(pkg, seed, w=W, h=H), seed % 2 == 0) for seed in range(4)]
    return cases


@pytest.mark.parametrize("case", range(14))
def test_primary_rays_as_explicit_rays(pkg, oracle, case):
    """The primary rays of a 64 x 48 frame as explicit rays: the records equal the composer and rt_pick of a plain context."""
    what, make, moved = primary_cases(pkg)[case]
    sc = make()
    cam = pkg.camera_matrix(*MOVED) if moved else None
    osc = oracle_from(pkg, oracle, sc)
    rays = rays_ref.primary_rays(osc, cam)
    want = rays_ref.closest(osc, rays)
    r = pkg.Renderer(sc, device=0)
    got = trace_dev(r, rays)
    assert_records(got, want, what)
    xy = np.stack([np.tile(np.arange(W), H), np.repeat(np.arange(H), W)], axis=1)
    assert_records(r.pick(xy, cam), got, (what, "rt_pick"))
    r.cleanup_update()
    if case < 3 or what == "70 spheres":
        assert (got["object"] >= 0).any() and (got["object"] < 0).any()
    if what == "70 spheres":
        assert got["object"].max() >= 64   # the second 64-entry chunk of the sphere table is reached


def arbitrary_rays(osc, n, seed):
    """Origins per ray: inside spheres, on surfaces (`point` of a previous hit), 1e5 away, negative-zero coordinates; directions scaled by
    1e-3 .. 1e3 plus the exact zero vector, |d|^2 <= 1e-7, single NaN components, +-inf components, and components beyond 1e100."""
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, dtype=rays_ref.RAY_DTYPE)
    coefs = osc.coefs
    spheres = [c for c in coefs if not c[:10].any() and c[10] == c[11] == c[12] == 1.0 and not c[13:16].any()]
    first = rays_ref.closest(osc, rays_ref.primary_rays(osc.with_size(16, 12)))
    on_surface = first["point"][first["object"] >= 0]
    for i in range(n):
        kind = i % 8
        if kind == 0 and spheres:
            c = spheres[int(rng.integers(len(spheres)))]
            o = -0.5 * c[16:19] + rng.uniform(-0.2, 0.2, 3)   # near the centre: inside
        elif kind == 1 and len(on_surface):
            o = on_surface[int(rng.integers(len(on_surface)))]
        elif kind == 2:
            v = rng.normal(size=3)
            o = 1e5 * v / np.linalg.norm(v)
        elif kind == 3:
            o = rng.uniform(-3, 3, 3)
            o[rng.integers(3)] = -0.0
        else:
            o = rng.uniform([-12, -8, -5], [12, 8, 30])
        target = rng.uniform([-10, -6, 5], [10, 8, 35])
        d = target - o if kind != 2 else -o + rng.normal(size=3) * 5.0
        d = d / np.linalg.norm(d) * 10.0 ** rng.uniform(-3, 3)
        odd = i % 29
        if odd == 0:
            d = np.zeros(3)
        elif odd == 1:
            d = d / np.linalg.norm(d) * 10.0 ** rng.uniform(-8, -3.6)   # |d|^2 <= 1e-7: the reference's linear branch
        elif odd == 2:
            d[rng.integers(3)] = np.nan
        elif odd == 3:
            d[rng.integers(3)] = np.inf * rng.choice([-1.0, 1.0])
        elif odd == 4:
            o = o.copy()
            o[rng.integers(3)] = np.nan
        elif odd == 5:
            d[rng.integers(3)] = 1e120 * rng.choice([-1.0, 1.0])
        elif odd == 6:
            d = np.array([-0.0, 0.0, 1.0]) * rng.choice([-1.0, 1.0])
        rays["o"][i], rays["d"][i] = o, d
    return rays


ARBITRARY = {"20spheres": lambda pkg: pkg.Scene.load_from_file(scene_path("20spheres")).set_size(W, H),
             "quadratic": lambda pkg: pkg.Scene.load_from_file(scene_path("quadratic")).set_size(W, H),
             "mixed": lambda pkg: mixed_scene(pkg, 2, w=W, h=H)}


@pytest.mark.parametrize("name", list(ARBITRARY))
def test_arbitrary_rays(pkg, oracle, name):
    import torch
    sc = ARBITRARY[name](pkg)
    osc = oracle_from(pkg, oracle, sc)
    n = 4000
    rays = arbitrary_rays(osc, n, 5)
    rng = np.random.default_rng(9)
    t_max = np.where(rng.random(n) < 0.5, 1e6, 10.0 ** rng.uniform(-2, 3, n))
    t_max[::97] = np.nan
    t_max[5::101] = np.inf
    want = rays_ref.closest(osc, rays)
    want_blocked, want_blocked_default = rays_ref.occluded(osc, rays, t_max), rays_ref.occluded(osc, rays)
    assert (want["object"] >= 0).sum() > n // 10 and (want["object"] < 0).sum() > n // 10 and 0 < want_blocked.sum() < want_blocked_default.sum() < n
    r = pkg.Renderer(sc, device=0)
    assert_records(trace_dev(r, rays), want, name)
    assert np.array_equal(occluded_dev(r, rays, t_max), want_blocked) and np.array_equal(occluded_dev(r, rays), want_blocked_default)
    for k in (1, 63, 64, 65, 255, 257, 1000):   # partial waves and partial workgroups, at an offset so that every slice differs
        sl = slice(k, 2 * k)
        assert_records(trace_dev(r, rays[sl]), want[sl], (name, k))
        assert np.array_equal(occluded_dev(r, rays[sl], t_max[sl]), want_blocked[sl]), (name, k)
    # more rays than one trip of the grid-stride loop: the grid is at most four workgroups of 256 rays per CU
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = (256 * 4 * cus) // n + 2
    big = np.tile(rays, reps)[: reps * n - 37]
    assert len(big) > 256 * 4 * cus + 256
    assert_records(trace_dev(r, big), np.tile(want, reps)[: len(big)], (name, "grid-stride"))
    assert np.array_equal(occluded_dev(r, big, np.tile(t_max, reps)[: len(big)]), np.tile(want_blocked, reps)[: len(big)])
    r.cleanup_update()


def plane_scenes(pkg, oracle, origin_z):
    s = pkg.Scene.new(8, 8, 50.0, 0, (0, 0, 0))
    s.add_object(pkg.surface_make("plane", [0, 0, origin_z], [0, 0, 1]), (1, 1, 1))
    return s, oracle_from(pkg, oracle, s)


def test_boundaries_of_the_definitions(pkg, oracle):
    """t exactly EPS: the closest hit accepts it, occlusion does not.  A plane at t = 2: not blocked with t_max = 2, blocked with the next double."""
    sc, osc = plane_scenes(pkg, oracle, -1e-7)
    rays = rays_ref.make_rays([[0.0, 0.0, 0.0]] * 2, [[0.0, 0.0, -1.0], [0.0, 0.0, -0.5]])
    r = pkg.Renderer(sc, device=0)
    got = trace_dev(r, rays)
    assert got["object"].tolist() == [0, 0] and got["t"][0] == 1e-7
    assert_records(got, rays_ref.closest(osc, rays))
    assert occluded_dev(r, rays).tolist() == [0, 1] == rays_ref.occluded(osc, rays).tolist()
    r.cleanup_update()
    sc, osc = plane_scenes(pkg, oracle, 2.0)
    rays = rays_ref.make_rays([[0.0, 0.0, 0.0]] * 4, [[0.0, 0.0, 1.0]] * 4)
    tm = [2.0, np.nextafter(2.0, 3.0), np.nan, np.inf]
    r = pkg.Renderer(sc, device=0)
    assert trace_dev(r, rays)["t"].tolist() == [2.0] * 4
    assert occluded_dev(r, rays, tm).tolist() == [0, 1, 0, 1] == rays_ref.occluded(osc, rays, tm).tolist()
    r.cleanup_update()


@pytest.mark.parametrize("seed", [0, 1])
def test_the_references_shadow_decisions(pkg, oracle, seed):
    """Every hit x light shadow ray of a lit frame, formed on the host as the header says: rt_occluded_rays equals the composer, and the
    unblocked rays are as many as the oracle's surface_color evaluations of that frame."""
    sc = random_scene(pkg, 900 + seed, 14, 4, w=W, h=H, with_plane=True).set_max_reflections(0)
    osc = oracle_from(pkg, oracle, sc)
    assert {int(l.is_spherical) for l in osc.lights} == {0, 1}
    rays = rays_ref.primary_rays(osc)
    n64 = np.zeros((len(rays), 3))
    hits = rays_ref.closest(osc, rays, normals64=n64)
    srays, tmax, _, _ = rays_ref.shadow_rays(osc, hits, n64)
    want = rays_ref.occluded(osc, srays, tmax)
    r = pkg.Renderer(sc, device=0)
    got = occluded_dev(r, srays, tmax)
    r.cleanup_update()
    assert np.array_equal(got, want) and 0 < want.sum() < len(want)
    _, cnt = osc.render(counters=True)
    assert int((got == 0).sum()) == cnt["surface_colors"] and len(srays) == cnt["shadow_rays"]


def test_through_a_mirror(pkg, oracle):
    """The mirror scene of test_gbuffer_gpu.py::test_edge_scenes: the G-buffer sees only the mirror; following orc_reflect_ray from
    the hit points finds the sphere behind the camera."""
    s = pkg.Scene.new(W, H, 50.0, 4, (0.1, 0.1, 0.1))
    s.add_object(pkg.surface_make("plane", [0, 0, 12], [0, 0, -1]), (0.9, 0.9, 0.9), 0.9)
    s.add_object(pkg.surface_make("sphere", [0, 0, -6], [2.0]), (0.9, 0.1, 0.1))
    s.add_light("directional", [0, -1, 1])
    osc = oracle_from(pkg, oracle, s)
    rays = rays_ref.primary_rays(osc)
    n64 = np.zeros((len(rays), 3))
    first = rays_ref.closest(osc, rays, normals64=n64)
    assert np.all(first["object"] == 0)
    dp = C.POINTER(C.c_double)
    bounce = np.zeros(len(rays), dtype=rays_ref.RAY_DTYPE)
    out = np.zeros(3)
    for i in range(len(rays)):
        d, nv = np.ascontiguousarray(rays["d"][i]), np.ascontiguousarray(n64[i])
        oracle.lib().orc_reflect_ray(d.ctypes.data_as(dp), nv.ctypes.data_as(dp), out.ctypes.data_as(dp))
        bounce["o"][i], bounce["d"][i] = first["point"][i], out
    r = pkg.Renderer(s, device=0)
    assert_records(trace_dev(r, rays), first)
    got = trace_dev(r, bounce)
    r.cleanup_update()
    assert_records(got, rays_ref.closest(osc, bounce))
    assert (got["object"] == 1).any() and (got["object"] == -1).any()


def cubic_check(pkg, oracle, sc, osc, rays, what):
    """As cubic_check of tests/test_gbuffer_gpu.py: object equal at every ray, t within that file's 1e-8 relative under the
    device-libm evaluator, normals by conftest.compare.  No ray is left out."""
    r = pkg.Renderer(sc, device=0)
    got = trace_dev(r, rays)
    r.cleanup_update()
    ref, _, rounds = oracle.under_libm(lambda: rays_ref.closest(osc, rays), D.evaluator(D.lib(pkg)))
    nobj = int((got["object"] != ref["object"]).sum())
    hit = ref["object"] >= 0
    rel = np.abs(got["t"][hit] - ref["t"][hit]) / np.abs(ref["t"][hit])
    c = compare(got["normal"], ref["normal"])
    print(f"{what}: object differs at {nobj} of {len(rays)} rays, max rel t {float(rel.max()) if rel.size else 0.0:.3e}, normals {c}, libm rounds {rounds}")
    assert nobj == 0, what
    assert np.array_equal(np.isposinf(got["t"]), ~hit)
    assert np.all(rel <= 1e-8), (what, float(rel.max()))
    assert c["n_bad_pixels"] == 0, (what, c)
    assert hit.any()


def rescaled(rays, seed):
    """Directions with |d| within [0.5, 2] (the G-buffer's are unit vectors)."""
    out = rays.copy()
    out["d"] *= np.random.default_rng(seed).uniform(0.5, 2.0, (len(rays), 1))
    return out


@pytest.mark.parametrize("name", CUBIC)
def test_shipped_scenes_of_degree_three(pkg, oracle, name):
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(W, H)
    osc = oracle.load_scene(scene_path(name)).with_size(W, H)
    cubic_check(pkg, oracle, sc, osc, rescaled(rays_ref.primary_rays(osc, pkg.camera_matrix((0.3, 0.2, -4.0), 90.0, 0.0)), 1), name)


@pytest.mark.parametrize("seed", range(3))
def test_random_scenes_of_degree_three(pkg, oracle, seed):
    sc, cam = random_cubic_scene(pkg, seed, W, H)
    osc = oracle_from(pkg, oracle, sc)
    cubic_check(pkg, oracle, sc, osc, rescaled(rays_ref.primary_rays(osc, cam), seed), f"random cubic {seed}")


def test_every_context_kind_answers_alike(pkg, oracle):
    for sc in (pkg.Scene.load_from_file(scene_path("20spheres")).set_size(97, 61), mixed_scene(pkg, 3, w=97, h=61)):
        rays = arbitrary_rays(oracle_from(pkg, oracle, sc), 500, 21)
        tm = np.random.default_rng(2).uniform(0.5, 50.0, 500)
        r = pkg.Renderer(sc, device=0)
        ref, ref_b = trace_dev(r, rays), occluded_dev(r, rays, tm)
        r.cleanup_update()
        assert (ref["object"] >= 0).any()
        kinds = [dict(flags=pkg.RT_FLAG_SSAA4), dict(flags=pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA_ADAPTIVE | pkg.RT_FLAG_SSAA_GEOMETRY),
                 dict(rank=1, world=3, band_rows=5), dict(fmt=pkg.RT_FMT_RGBA8), dict(flags=pkg.RT_FLAG_SIMPLE), dict(flags=pkg.RT_FLAG_NOCULL),
                 dict(flags=pkg.RT_FLAG_NOLEAN), dict(flags=pkg.RT_FLAG_STREAM)]
        for kw in kinds:
            r = pkg.Renderer(sc, device=0, **kw)
            assert_records(trace_dev(r, rays), ref, kw)
            assert_records(r.trace(rays["o"], rays["d"]), ref, (kw, "host"))
            assert np.array_equal(occluded_dev(r, rays, tm), ref_b), kw
            r.cleanup_update()


def test_queries_are_invisible_to_the_frames_and_to_each_other(pkg, oracle):
    import torch
    w, h = 320, 180
    sc = random_scene(pkg, 4242, 40, 4, w=w, h=h, with_plane=False)
    front, away, side = pkg.camera_matrix((0.0, 0.0, 0.0), 90.0, 0.0), pkg.camera_matrix((0.0, 0.0, 0.0), -90.0, 0.0), pkg.camera_matrix((14.0, 2.0, 20.0), 160.0, -5.0)
    fresh = pkg.Renderer(sc, device=0)
    want = []
    for cam in (front, away, side):
        fresh.update(cam)
        want.append(fresh.download().copy())
    rays = arbitrary_rays(oracle_from(pkg, oracle, sc), 2000, 8)
    ref, ref_b = trace_dev(fresh, rays), occluded_dev(fresh, rays)
    fresh.cleanup_update()
    r = pkg.Renderer(sc, device=0)
    s2 = torch.cuda.Stream()
    frames = []
    r.update(front)
    frames.append(r.download().copy())
    assert_records(trace_dev(r, rays), ref)
    r.update(away)
    frames.append(r.download().copy())
    assert_records(trace_dev(r, rays, stream=s2.cuda_stream, timed=False), ref, "second stream")
    assert np.array_equal(occluded_dev(r, rays), ref_b)
    r.update(side)
    frames.append(r.download().copy())
    for a, b in zip(frames, want):
        assert np.array_equal(a, b)
    assert_records(trace_dev(r, rays), ref, "after three frames")
    r.update(front)
    assert np.array_equal(r.download(), want[0])
    r.cleanup_update()


def test_three_queries_captured_into_one_graph(pkg, oracle):
    import torch
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(W, H)
    rays = arbitrary_rays(oracle_from(pkg, oracle, sc), 3000, 4)
    parts = [rays[:1000], rays[1000:1900], rays[1900:]]
    r = pkg.Renderer(sc, device=0)
    plain = [trace_dev(r, parts[0]), trace_dev(r, parts[1]), occluded_dev(r, parts[2])]
    s = torch.cuda.Stream()
    d_rays = [to_device(p) for p in parts]
    outs = [torch.zeros((len(parts[0]), 6), dtype=torch.float64, device="cuda:0"), torch.zeros((len(parts[1]), 6), dtype=torch.float64, device="cuda:0"),
            torch.full((len(parts[2]),), -9, dtype=torch.int32, device="cuda:0")]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r.trace_into(d_rays[0].data_ptr(), len(parts[0]), outs[0].data_ptr(), stream=s.cuda_stream, timed=False)
        r.trace_into(d_rays[1].data_ptr(), len(parts[1]), outs[1].data_ptr(), stream=s.cuda_stream, timed=False)
        r.occluded_into(d_rays[2].data_ptr(), None, len(parts[2]), outs[2].data_ptr(), stream=s.cuda_stream, timed=False)
    g.replay()
    torch.cuda.synchronize()
    assert_records(hits_of(outs[0]), plain[0])
    assert_records(hits_of(outs[1]), plain[1])
    assert np.array_equal(outs[2].cpu().numpy(), plain[2]) and plain[2].any()
    r.cleanup_update()


def test_host_entry_points(pkg, oracle):
    """rt_trace_rays_host equals the device entry point; mi355rt_update_trace of libmi355rt_update.so (ctypes: init_update receives the
    loaded scene's Scene object, the first member of the rt_scene handle) equals both and refuses before init_update."""
    sc = pkg.Scene.load_from_file(scene_path("quadratic")).set_size(W, H)
    rays = arbitrary_rays(oracle_from(pkg, oracle, sc), 700, 3)
    r = pkg.Renderer(sc, device=0)
    dev = trace_dev(r, rays)
    host = r.trace(rays["o"], rays["d"])
    assert host.dtype == pkg.HIT_DTYPE
    assert_records(host, dev)
    assert_records(r.trace(rays["o"][:3], rays["d"][:3]), dev[:3])   # (the staging buffers do not shrink)
    assert_records(r.trace(np.tile(rays["o"], (3, 1)), np.tile(rays["d"], (3, 1))), np.tile(dev, 3))   # (... and grow)
    r.cleanup_update()
    assert (dev["object"] >= 0).any()
    upd = C.CDLL(pkg.UPDATE_LIB_PATH)
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
    cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
    init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
    upd.mi355rt_update_trace.argtypes = [C.POINTER(pkg.Ray), C.c_uint, C.POINTER(pkg.Hit)]
    out = np.zeros(len(rays), dtype=pkg.HIT_DTYPE)
    args = (rays.ctypes.data_as(C.POINTER(pkg.Ray)), len(rays), out.ctypes.data_as(C.POINTER(pkg.Hit)))
    assert upd.mi355rt_update_trace(*args) == -1 and b"init_update" in pkg.lib().rt_last_error()
    init(42, sc._h)
    try:
        assert upd.mi355rt_update_trace(*args) == 0, pkg.lib().rt_last_error()   # (no update() call needed: a ray query uses no camera)
    finally:
        cleanup()
    assert_records(out, dev)
    assert upd.mi355rt_update_trace(*args) == -1


def test_refusals(pkg):
    import torch
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(W, H)
    r = pkg.Renderer(sc, device=0)
    buf = torch.zeros((64, 6), dtype=torch.float64, device="cuda:0")
    out = torch.zeros((64, 6), dtype=torch.float64, device="cuda:0")
    flags = torch.zeros((64,), dtype=torch.int32, device="cuda:0")
    p, q, f = buf.data_ptr(), out.data_ptr(), flags.data_ptr()

    def refused(call, *words):
        with pytest.raises(pkg.RtError) as e:
            call()
        assert e.value.code == -1 and any(w in str(e.value) for w in words), str(e.value)
    refused(lambda: r.trace_into(None, 4, q), "null")
    refused(lambda: r.trace_into(p, 4, None), "null")
    refused(lambda: r.occluded_into(None, None, 4, f), "null")
    refused(lambda: r.occluded_into(p, None, 4, None), "null")
    refused(lambda: r.trace_into(p, 0, q), "n is 0")
    refused(lambda: r.occluded_into(p, None, 0, f), "n is 0")
    refused(lambda: r.trace(np.zeros((0, 3)), np.zeros((0, 3))), "n is 0")
    refused(lambda: r.trace_into(p + 8, 4, q), "aligned")
    refused(lambda: r.trace_into(p, 4, q + 8), "aligned")
    refused(lambda: r.occluded_into(p + 8, None, 4, f), "aligned")
    refused(lambda: r.trace_into(p, 8, p), "overlap")
    refused(lambda: r.trace_into(p, 8, p + 48 * 7), "overlap")
    refused(lambda: r.trace_into(p + 48 * 7, 8, p), "overlap")
    refused(lambda: r.occluded_into(p, None, 8, p + 16), "overlap")
    refused(lambda: r.occluded_into(p, q, 8, q + 32), "overlap")
    assert pkg.lib().rt_trace_rays_host(r._h, None, 4, None, None) == -1 and b"null" in pkg.lib().rt_last_error()
    r.trace_into(p, 8, p + 48 * 8)   # adjacent ranges are fine
    r.cleanup_update()


def test_fast_build_statistics(pkg, oracle):
    """FAST against strict on the primary rays of three scenes, in the style of test_gbuffer_gpu.py::test_fast_build_statistics: the
    figures are printed; only the agreement of `object` is held, to 99 %."""
    for name in ("20spheres", "quadratic", "clebsch"):
        w, h = 160, 90
        sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
        rays = rays_ref.primary_rays(oracle.load_scene(scene_path(name)).with_size(w, h))
        ra, rb = pkg.Renderer(sc, device=0), pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_FAST)
        a, b = trace_dev(ra, rays), trace_dev(rb, rays)
        ra.cleanup_update()
        rb.cleanup_update()
        both = (a["object"] >= 0) & (b["object"] >= 0)
        rel = np.abs(a["t"][both] - b["t"][both]) / np.abs(a["t"][both])
        agree = float((a["object"] == b["object"]).mean())
        print(f"FAST vs strict ray queries, {name} {w}x{h}: object differs at {int((a['object'] != b['object']).sum())} of {len(rays)} rays ({100 * agree:.3f} % agree), "
              f"max rel t difference {float(rel.max()):.3e}, normals not bit-equal at {int((a['normal'].view(np.uint32) != b['normal'].view(np.uint32)).any(axis=-1).sum())} rays")
        assert agree >= 0.99, (name, agree)


def test_at_scale(pkg, oracle):
    """The 1024 x 1024 primary rays of 20spheres as explicit rays (the reference's direction formula in numpy float64, held to
    orc_primary_dir on a sample): object, t and normal of one rt_trace_rays call equal rt_render_gbuffer's planes, compared on the device."""
    import torch
    n = 1024
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(n, n)
    osc = oracle.load_scene(scene_path("20spheres")).with_size(n, n)
    ndc = (np.arange(n) + 0.5) / n   # src/update-cpu.cpp:84-89 with the identity camera
    th = np.tan(0.5 * osc.vertical_fov)
    cx, cy = (2.0 * ndc - 1.0) * (float(n) / float(n)) * th, (2.0 * ndc - 1.0) * th
    wx, wy, wz = np.broadcast_to(cx, (n, n)), np.broadcast_to(cy[:, None], (n, n)), np.ones((n, n))
    inv = 1.0 / np.sqrt((wx * wx + wy * wy) + wz * wz)
    rays = np.zeros((n, n), dtype=rays_ref.RAY_DTYPE)
    rays["d"] = np.stack([wx * inv, wy * inv, wz * inv], axis=-1)
    rng = np.random.default_rng(1)
    for y, x in zip(rng.integers(0, n, 300).tolist(), rng.integers(0, n, 300).tolist()):
        assert np.array_equal(rays["d"][y, x].view(np.uint64), rays_ref.primary_rays(osc, rows=[y], cols=[x])["d"][0].view(np.uint64))
    r = pkg.Renderer(sc, device=0)
    o, t, nrm, _ = r.gbuffer()
    d_rays = to_device(rays.reshape(-1))
    hits = torch.empty((n * n, 6), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ms = r.trace_into(d_rays.data_ptr(), n * n, hits.data_ptr())
    r.cleanup_update()
    assert 0.0 <= ms < 1000.0
    words = hits.view(torch.int32).reshape(n, n, 12)
    assert torch.equal(words[..., 11], o), int((words[..., 11] != o).sum())
    assert torch.equal(hits.reshape(n, n, 6)[..., 0].view(torch.int64), t.view(torch.int64))
    assert torch.equal(words[..., 8:11], nrm.view(torch.int32)[..., :3])
    assert int((o >= 0).sum()) > 10000
