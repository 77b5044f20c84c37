"""rt_shade_rays / rt_shade_rays_host / mi355rt_update_shade on the GPU (csrc/rt_shade_rays.hip) against the
reference composer tests/tools/shade_ref.py and against rt_render's own RGBA32F frames.  Strict contexts unless said otherwise.  Colours
are compared on their bits (integer views, so signed zeros and infinities count); a NaN channel has to be a NaN on both sides, since
IEEE 754 leaves a NaN's sign and payload open and the device and the host's glibc spell it differently
(raw_desc_scenes.same_as_oracle).  Two device results are always compared on all bits."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, compare, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import rays_ref  # noqa: E402
import raw_desc_scenes as R  # noqa: E402
import shade_ref  # noqa: E402
import cubic_device_lab as D  # noqa: E402  (the oracle under the device's cbrt / acos / cos)
from test_gpu_parity import CUBIC, mixed_scene, oracle_from, random_cubic_scene, random_scene  # noqa: E402
from test_rays_gpu import MOVED, arbitrary_rays, hits_of, primary_cases, rescaled, to_device, trace_dev  # noqa: E402
from test_shade_host import FAR_LIT, FAR_RAY, RATIO_ABOVE, RATIO_BELOW, facing_mirrors, far_plane, ratio_scene, scene_of  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 64, 48
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def shade_dev(r, rays, hits=False, stream=None, timed=True):
    """rt_shade_rays on device tensors: ([n, 4] float32, HIT_DTYPE records or None)."""
    import torch
    d_rays = to_device(rays)
    out = torch.full((len(rays), 4), float("nan"), dtype=torch.float32, device="cuda:0")
    rec = torch.full((len(rays), 6), float("nan"), dtype=torch.float64, device="cuda:0") if hits else None
    torch.cuda.synchronize()
    ms = r.shade_into(d_rays.data_ptr(), len(rays), out.data_ptr(), rec.data_ptr() if hits else None, stream=stream, timed=timed)
    assert (ms is not None and ms >= 0.0) if timed else ms is None
    torch.cuda.synchronize()
    return out.cpu().numpy(), (hits_of(rec) if hits else None)


def assert_colours(got, want, what=""):
    """Against the composer: NaN where it has NaN, the same bits everywhere else; alpha 1.0f."""
    assert got.shape == want.shape and got.dtype == np.float32
    n = np.isnan(want)
    assert np.array_equal(np.isnan(got), n) and np.array_equal(bits(got)[~n], bits(want)[~n]), (what, shade_ref.describe_difference(got, want))
    assert np.all(bits(got[:, 3]) == bits(F(1.0)))


def assert_same_bits(a, b, what=""):
    assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (what, shade_ref.describe_difference(a, b))


def assert_records(got, want, what=""):
    assert got.dtype == rays_ref.HIT_DTYPE and rays_ref.same_records(got, want), (what, rays_ref.describe_difference(got, want))


def assert_records_as_composer(got, want, what=""):
    """Records against the composer's: as same_records, with a NaN normal component a NaN on both sides."""
    g, w = got.copy(), want.copy()
    n = np.isnan(w["normal"])
    assert np.array_equal(np.isnan(g["normal"]), n), what
    g["normal"][n] = 0.0
    w["normal"][n] = 0.0
    assert_records(g, w, what)


def frame_of(pkg, sc, cam=None, **kw):
    r = pkg.Renderer(sc, device=0, **kw)
    r.update(cam)
    img = r.download().copy()
    return r, img


# ---- primary rays as explicit rays -------------------------------------------------------------------------------------------------
COMPOSED = ("20spheres", "reflection_test", "random 0")


@pytest.mark.parametrize("case", range(14))
def test_primary_rays_as_explicit_rays(pkg, oracle, case):
    """The primary rays of a 64 x 48 frame as explicit rays: the colours are the RGBA32F frame of rt_render on the same context, the
    records are rt_trace_rays'; three cases also against the composer at 48 x 36."""
    what, make, moved = primary_cases(pkg)[case]
    sc = make()
    cam = pkg.camera_matrix(*MOVED) if moved else None
    osc = oracle_from(pkg, oracle, sc)
    rays = rays_ref.primary_rays(osc, cam)
    r, frame = frame_of(pkg, sc, cam)
    got, rec = shade_dev(r, rays, hits=True)
    assert_same_bits(got, frame.reshape(-1, 4), what)
    assert_records(rec, trace_dev(r, rays), what)
    assert_same_bits(shade_dev(r, rays)[0], got, (what, "without hits"))
    r.cleanup_update()
    if case < 3 or what == "70 spheres":
        assert (rec["object"] >= 0).any() and (rec["object"] < 0).any()
    if what == "70 spheres":
        assert rec["object"].max() >= 64   # the second 64-entry chunk of the sphere table is reached
    if what == "reflection_test":
        r0, frame0 = frame_of(pkg, make().set_max_reflections(0), cam)
        assert_same_bits(shade_dev(r0, rays)[0], frame0.reshape(-1, 4), (what, "max_reflections 0"))
        r0.cleanup_update()
        assert (bits(frame0) != bits(frame)).any()   # the mirrors show
    if what in COMPOSED:
        small = osc.with_size(48, 36)
        rays = rays_ref.primary_rays(small, cam)
        want, want_rec = shade_ref.shade(small, rays, hits=True)
        r = pkg.Renderer(sc.set_size(48, 36), device=0)
        got, rec = shade_dev(r, rays, hits=True)
        r.cleanup_update()
        assert_colours(got, want, (what, "composer"))
        assert_records(rec, want_rec, (what, "composer"))


def test_the_composed_cases_exist(pkg):
    assert set(COMPOSED) <= {c[0] for c in primary_cases(pkg)}


# ---- arbitrary rays ----------------------------------------------------------------------------------------------------------------
ARBITRARY = {"20spheres": lambda pkg: pkg.Scene.load_from_file(scene_path("20spheres")).set_size(W, H),
             "quadratic": lambda pkg: pkg.Scene.load_from_file(scene_path("quadratic")).set_size(W, H),
             "mixed": lambda pkg: mixed_scene(pkg, 2, w=W, h=H)}   # mirrors, a point light, planes and general quadrics


@pytest.mark.parametrize("name", list(ARBITRARY))
def test_arbitrary_rays(pkg, oracle, name):
    import torch
    sc = ARBITRARY[name](pkg)
    osc = oracle_from(pkg, oracle, sc)
    if name == "mixed":
        assert (osc.reflection > 1e-7).any() and osc.light_is_spherical.any() and not osc.light_is_spherical.all()
    n = 1500
    rays = arbitrary_rays(osc, n, 5)
    seg = np.zeros(n, dtype=np.int64)
    want, want_rec = shade_ref.shade(osc, rays, hits=True, segments=seg)
    hit = want_rec["object"] >= 0
    assert hit.sum() > n // 10 and (~hit).sum() > n // 10 and (name != "mixed" or seg.max() > 1)
    r = pkg.Renderer(sc, device=0)
    got, rec = shade_dev(r, rays, hits=True)
    assert_colours(got, want, name)
    assert_records(rec, want_rec, name)
    for k in (1, 63, 64, 65, 255, 256, 257, 1000):   # partial waves and partial workgroups, at an offset so that every slice differs
        a = min(k, n - k)
        sl = slice(a, a + k)
        part, part_rec = shade_dev(r, rays[sl], hits=True)
        assert_same_bits(part, got[sl], (name, k))
        assert_records(part_rec, rec[sl], (name, k))
    # more rays than one trip of the grid-stride loop (at most four workgroups of 256 rays per CU): every copy's bits equal the first's
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = (256 * 4 * cus) // 1000 + 2
    big = np.tile(rays[:1000], reps)[: reps * 1000 - 37]
    assert len(big) > 256 * 4 * cus + 256
    d_rays = to_device(big)
    out = torch.full((len(big), 4), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.shade_into(d_rays.data_ptr(), len(big), out.data_ptr())
    first = torch.from_numpy(bits(got[:1000]).astype(np.int32)).to("cuda:0")
    words = torch.cat([out.view(torch.int32), first[963:]]).reshape(reps, 1000, 4)   # (the cut tail filled in)
    assert bool((words == first[None]).all()), (name, "grid-stride")
    r.cleanup_update()


# ---- derived rays outside the tables' proven range ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", [False, True])
def test_hit_point_beyond_the_proven_range(pkg, oracle, mirror):
    """The 1e104 plane of tests/test_shade_host.py: the caller's ray is inside the proven range, its hit point is not, and every test
    of the shadow and bounce rays is NaN in the reference: the hit is lit, the mirror blends the background."""
    osc = far_plane(oracle, mirror)
    rays = rays_ref.make_rays(*FAR_RAY)
    want, want_rec = shade_ref.shade(osc, rays, hits=True)
    r = pkg.Renderer(R.desc(pkg, osc), device=0)
    got, rec = shade_dev(r, rays, hits=True)
    r.cleanup_update()
    assert_colours(got, want)
    assert_records(rec, want_rec)
    lit = [FAR_LIT] * 3 if not mirror else [(F(1.0) - F(0.5)) * FAR_LIT + F(0.5) * F(b) for b in (0.5, 0.25, 1.0)]
    assert got[0].tolist() == lit + [1.0] and rec["object"][0] == 1


def cone_scene(oracle, mirror):
    """The cone x^2 + y^2 - z^2 = 0 (its gradient vanishes at the apex), a sphere behind it and two lights."""
    q = np.zeros(20)
    q[10], q[11], q[12] = 1.0, 1.0, -1.0
    return scene_of(oracle, [(list(q), (0.8, 0.7, 0.6), 0.5 if mirror else 0.0), (R.sphere((0.5, 0.2, 6), 1.5), (0.2, 0.9, 0.3), 0.0)],
                    [R.stored_light(0, R.unit((0.2, 1.0, -0.5)), (0.9, 0.8, 0.7)), R.stored_light(1, (2.0, 3.0, -1.0), (30.0, 30.0, 30.0))])


CONE_RAYS = ([[0.0, 0.0, -2.0], [0.3, 0.1, -2.0], [0.0, 0.0, -2.0]], [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.5]])


@pytest.mark.parametrize("mirror", [False, True])
def test_hit_where_the_gradient_vanishes(pkg, oracle, mirror):
    osc = cone_scene(oracle, mirror)
    rays = rays_ref.make_rays(*CONE_RAYS)
    want, want_rec = shade_ref.shade(osc, rays, hits=True)
    assert np.isnan(want_rec["normal"][0]).all() and want_rec["point"][0].tolist() == [0.0, 0.0, 0.0] and not np.isnan(want_rec["normal"][1]).any()
    r = pkg.Renderer(R.desc(pkg, osc), device=0)
    got, rec = shade_dev(r, rays, hits=True)
    assert_records(rec, trace_dev(r, rays))
    r.cleanup_update()
    assert_colours(got, want, mirror)
    assert_records_as_composer(rec, want_rec, mirror)


# ---- reflections ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_refl", [0, 1, 5])
def test_reflection_depths(pkg, oracle, max_refl):
    sc = random_scene(pkg, 3100, 9, 2, w=40, h=30, with_plane=True, mirrors=True).set_max_reflections(max_refl)
    osc = oracle_from(pkg, oracle, sc)
    cam = pkg.camera_matrix((0.5, 1.0, -2.0), 88.0, -6.0)
    rays = rays_ref.primary_rays(osc, cam)
    seg = np.zeros(len(rays), dtype=np.int64)
    want = shade_ref.shade(osc, rays, segments=seg)
    r, frame = frame_of(pkg, sc, cam)
    got, _ = shade_dev(r, rays)
    r.cleanup_update()
    assert_colours(got, want, max_refl)
    assert_same_bits(got, frame.reshape(-1, 4), max_refl)
    assert seg.max() == max_refl + 1 if max_refl < 5 else seg.max() > 2


def test_facing_mirrors_and_ratio_boundaries(pkg, oracle):
    rays = rays_ref.make_rays([[0.0, 0.0, 0.0], [0.1, -0.2, 1.0]], [[0.0, 0.0, 1.0], [0.0, 0.0, -3.0]])
    for max_refl, value in ((0, 0.5), (2, 0.125), (5, 0.015625)):
        osc = facing_mirrors(oracle, max_refl)
        r = pkg.Renderer(R.desc(pkg, osc), device=0)
        got, _ = shade_dev(r, rays)
        r.cleanup_update()
        assert_colours(got, shade_ref.shade(osc, rays), max_refl)
        assert got.tolist() == [[value, value, value, 1.0]] * 2
    for ratio, value in ((RATIO_ABOVE, [RATIO_ABOVE * F(0.5), RATIO_ABOVE * F(0.25), RATIO_ABOVE * F(1.0), 1.0]), (RATIO_BELOW, [0.0, 0.0, 0.0, 1.0])):
        osc = ratio_scene(oracle, ratio)
        r = pkg.Renderer(R.desc(pkg, osc), device=0)
        got, _ = shade_dev(r, rays[:1])
        r.cleanup_update()
        assert_colours(got, shade_ref.shade(osc, rays[:1]), ratio)
        assert got[0].tolist() == value


def mirror_scene(pkg):
    """The mirror scene of test_rays_gpu.py::test_through_a_mirror: a mirror plane ahead, a sphere behind the camera."""
    s = pkg.Scene.new(W, H, 50.0, 4, (0.1, 0.1, 0.1))
    s.add_object(pkg.surface_make("plane", [0, 0, 12], [0, 0, -1]), (0.9, 0.9, 0.9), 0.9)
    s.add_object(pkg.surface_make("sphere", [0, 0, -6], [2.0]), (0.9, 0.1, 0.1))
    s.add_light("directional", [0, -1, 1])
    return s


@pytest.mark.parametrize("scale", [0.5, 2.0])
def test_unnormalised_direction_through_a_mirror(pkg, oracle, scale):
    sc = mirror_scene(pkg)
    osc = oracle_from(pkg, oracle, sc).with_size(40, 30)
    rays = rays_ref.primary_rays(osc)
    rays["d"] *= scale
    seg = np.zeros(len(rays), dtype=np.int64)
    want, want_rec = shade_ref.shade(osc, rays, hits=True, segments=seg)
    assert np.all(want_rec["object"] == 0) and np.all(seg == 2) and len(np.unique(bits(want[:, 0]))) > 2   # the sphere shows in the mirror
    r = pkg.Renderer(sc, device=0)
    got, rec = shade_dev(r, rays, hits=True)
    r.cleanup_update()
    assert_colours(got, want, scale)
    assert_records(rec, want_rec, scale)


# ---- lights --------------------------------------------------------------------------------------------------------------------------
def test_without_lights_hits_are_black(pkg, oracle):
    sc = random_scene(pkg, 3200, 10, 0, w=40, h=30, with_plane=False, mirrors=False)
    osc = oracle_from(pkg, oracle, sc)
    rays = rays_ref.primary_rays(osc)
    want, want_rec = shade_ref.shade(osc, rays, hits=True)
    r, frame = frame_of(pkg, sc)
    got, rec = shade_dev(r, rays, hits=True)
    r.cleanup_update()
    assert_colours(got, want)
    assert_same_bits(got, frame.reshape(-1, 4))
    hit = rec["object"] >= 0
    assert hit.any() and (~hit).any() and not got[hit, :3].any() and np.array_equal(got[~hit, :3], np.broadcast_to(osc.bg_color, ((~hit).sum(), 3)))


ODD = R.FAMILIES + ["mirror-many-dir_nan_inf_color", "gq-many-pcol_nan", "lean-many-dir_eps_above"]


@pytest.mark.parametrize("name", ODD)
def test_odd_lights_and_colours_of_raw_descriptors(pkg, oracle, name):
    """Light vectors that are short, zero, long, NaN or inf, colours / albedos / backgrounds that are not finite (tests/tools/
    raw_desc_scenes.py), handed over as raw descriptors: the composer's colours, and the frame's."""
    osc, _, cams = R.named(name)
    osc = osc.with_size(32, 24)
    cam = cams[1]
    rays = rays_ref.primary_rays(osc, cam)
    want = shade_ref.shade(osc, rays)
    r, frame = frame_of(pkg, R.desc(pkg, osc), cam)
    got, _ = shade_dev(r, rays)
    r.cleanup_update()
    n = np.isnan(want)
    assert np.array_equal(np.isnan(got), n) and np.array_equal(bits(got)[~n], bits(want)[~n]), (name, shade_ref.describe_difference(got, want))
    assert_same_bits(got, frame.reshape(-1, 4), name)


# ---- degree 3 ------------------------------------------------------------------------------------------------------------------------
def cubic_check(pkg, oracle, sc, osc, rays, what):
    """The composer under the device's cbrt / acos / cos is the reference; conftest.compare; bad pixels <= max(3, int(0.002 * w * h)),
    the bound tests/test_cubic_gpu.py applies to frames with cubics and mirrors.  The composer under glibc is compared first, so that
    the share of the bound that libm alone takes is on record."""
    r = pkg.Renderer(sc, device=0)
    got, _ = shade_dev(r, rays)
    r.cleanup_update()
    glibc = shade_ref.shade(osc, rays)
    ref, _, rounds = oracle.under_libm(lambda: shade_ref.shade(osc, rays), D.evaluator(D.lib(pkg)))
    c_libm = compare(glibc[:, :3], ref[:, :3])
    c = compare(got[:, :3], ref[:, :3])
    print(f"{what}: glibc composer vs device-libm composer {c_libm['n_bad_pixels']} bad pixels; rt_shade_rays vs device-libm composer {c['n_bad_pixels']} bad of {len(rays)} "
          f"(max rel {c['max_rel']:.3e}), libm rounds {rounds}")
    assert c["n_bad_pixels"] <= max(3, int(0.002 * W * H)), (what, c)
    assert np.all(bits(got[:, 3]) == bits(F(1.0))) and (bits(got[:, :3]) != bits(got[0, :3])).any()


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


# ---- contexts, frames, graphs ----------------------------------------------------------------------------------------------------------
def test_every_context_kind_answers_alike(pkg, oracle):
    for sc in (pkg.Scene.load_from_file(scene_path("20spheres")).set_size(97, 61), mixed_scene(pkg, 3, w=97, h=61)):
        rays = arbitrary_rays(oracle_from(pkg, oracle, sc), 500, 21)
        r = pkg.Renderer(sc, device=0)
        ref, ref_rec = shade_dev(r, rays, hits=True)
        r.cleanup_update()
        assert (ref_rec["object"] >= 0).any()
        kinds = [dict(flags=pkg.RT_FLAG_SSAA2), dict(flags=pkg.RT_FLAG_SSAA4 | pkg.RT_FLAG_SSAA_ADAPTIVE),
                 dict(flags=pkg.RT_FLAG_SSAA4 | pkg.RT_FLAG_SSAA_ADAPTIVE | pkg.RT_FLAG_SSAA_GEOMETRY), dict(rank=1, world=2, band_rows=5), dict(fmt=pkg.RT_FMT_RGBA8),
                 dict(flags=pkg.RT_FLAG_NOCULL | pkg.RT_FLAG_SIMPLE), dict(flags=pkg.RT_FLAG_STREAM)]
        for kw in kinds:
            r = pkg.Renderer(sc, device=0, **kw)
            got, rec = shade_dev(r, rays, hits=True)
            assert_same_bits(got, ref, kw)
            assert_records(rec, ref_rec, kw)
            assert_same_bits(r.shade(rays["o"], rays["d"]), ref, (kw, "host"))
            r.cleanup_update()


def booked(counters):
    """The counters a frame defines.  tests_executed is left out: in a view without hits it counts the tests of workgroups that start
    before the tile scan has declared their tile empty, and differs between two identical frame sequences of fresh contexts (3136 ..
    5120 in four runs of the sequence below without any shade call)."""
    return {k: v for k, v in counters.items() if k != "tests_executed"}


def test_shading_is_invisible_to_the_frames(pkg, oracle):
    import torch
    w, h = 320, 180
    sc = random_scene(pkg, 4242, 40, 4, w=w, h=h, with_plane=False, mirrors=True)
    views = [pkg.camera_matrix((0.0, 0.0, 0.0), 90.0, 0.0), pkg.camera_matrix((0.0, 0.0, 0.0), -90.0, 0.0), pkg.camera_matrix((14.0, 2.0, 20.0), 160.0, -5.0)]
    rays = arbitrary_rays(oracle_from(pkg, oracle, sc), 2000, 8)
    want, want_cnt = [], []
    fresh = pkg.Renderer(sc, device=0)
    for cam in views:
        fresh.update(cam)
        want.append(fresh.download().copy())
    ref, _ = shade_dev(fresh, rays)
    fresh.cleanup_update()
    fresh = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_STRICT | pkg.RT_FLAG_COUNT)
    for cam in views:
        fresh.update(cam)
        want_cnt.append(fresh.counters())
    fresh.cleanup_update()
    s2 = torch.cuda.Stream()
    r = pkg.Renderer(sc, device=0)
    frames = []
    for k, cam in enumerate(views):
        r.update(cam)
        frames.append(r.download().copy())
        got, _ = shade_dev(r, rays, stream=s2.cuda_stream if k == 1 else None, timed=k != 1)
        assert_same_bits(got, ref, k)
    r.update(views[0])
    assert np.array_equal(bits(r.download()), bits(want[0]))
    r.cleanup_update()
    for a, b in zip(frames, want):
        assert np.array_equal(bits(a), bits(b))
    r = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_STRICT | pkg.RT_FLAG_COUNT)
    for cam, cnt in zip(views, want_cnt):
        assert_same_bits(shade_dev(r, rays)[0], ref, "counting context")
        r.update(cam)
        assert_same_bits(shade_dev(r, rays)[0], ref, "counting context")
        assert booked(r.counters()) == booked(cnt)   # RT_FLAG_COUNT books none of the shaded rays
    r.cleanup_update()
    assert want_cnt[0]["primary_rays"] == w * h


def test_three_calls_captured_into_one_graph(pkg, oracle):
    import torch
    sc = mixed_scene(pkg, 2, w=W, h=H)
    rays = arbitrary_rays(oracle_from(pkg, oracle, sc), 3000, 4)
    parts = [rays[:1000], rays[1000:1900], rays[1900:]]
    r = pkg.Renderer(sc, device=0)
    plain = [shade_dev(r, p, hits=True) for p in parts]
    s = torch.cuda.Stream()
    d_rays = [to_device(p) for p in parts]
    outs = [torch.zeros((len(p), 4), dtype=torch.float32, device="cuda:0") for p in parts]
    recs = [torch.zeros((len(p), 6), dtype=torch.float64, device="cuda:0") for p in parts]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):   # one stream: the three kernels form a single chain
        for k in range(3):
            r.shade_into(d_rays[k].data_ptr(), len(parts[k]), outs[k].data_ptr(), recs[k].data_ptr() if k != 1 else None, stream=s.cuda_stream, timed=False)
    for _ in range(2):
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for k in range(3):
            assert_same_bits(outs[k].cpu().numpy(), plain[k][0], k)
            if k != 1:
                assert_records(hits_of(recs[k]), plain[k][1], k)
    r.cleanup_update()


# ---- host entry points, refusals, the FAST build -----------------------------------------------------------------------------------------
def test_host_entry_points(pkg, oracle):
    """rt_shade_rays_host equals the device entry point; mi355rt_update_shade of libmi355rt_update.so (ctypes: init_update receives the
    loaded scene's Scene object, the first member of the rt_scene handle) equals both, and refuses before init_update and after
    cleanup_update."""
    sc = pkg.Scene.load_from_file(scene_path("reflection_test")).set_size(W, H)
    rays = arbitrary_rays(oracle_from(pkg, oracle, sc), 700, 3)
    r = pkg.Renderer(sc, device=0)
    dev, rec = shade_dev(r, rays, hits=True)
    host = r.shade(rays["o"], rays["d"])
    assert host.shape == (700, 4) and host.dtype == np.float32
    assert_same_bits(host, dev)
    assert_same_bits(r.shade(rays["o"][:3], rays["d"][:3]), dev[:3])   # (the staging buffers do not shrink)
    assert_same_bits(r.shade(np.tile(rays["o"], (3, 1)), np.tile(rays["d"], (3, 1))), np.tile(dev, (3, 1)))   # (... and grow)
    assert_records(r.trace(rays["o"], rays["d"]), rec)   # (... and are shared with rt_trace_rays_host)
    r.cleanup_update()
    assert (rec["object"] >= 0).any()
    upd = C.CDLL(pkg.UPDATE_LIB_PATH)
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
    cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
    init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
    upd.mi355rt_update_shade.argtypes = [C.POINTER(pkg.Ray), C.c_uint, C.POINTER(C.c_float)]
    out = np.zeros((len(rays), 4), dtype=np.float32)
    args = (rays.ctypes.data_as(C.POINTER(pkg.Ray)), len(rays), out.ctypes.data_as(C.POINTER(C.c_float)))
    assert upd.mi355rt_update_shade(*args) == -1 and b"init_update" in pkg.lib().rt_last_error()
    init(42, sc._h)
    try:
        assert upd.mi355rt_update_shade(*args) == 0, pkg.lib().rt_last_error()   # (no update() call needed: no camera is involved)
    finally:
        cleanup()
    assert_same_bits(out, dev)
    assert upd.mi355rt_update_shade(*args) == -1


def test_refusals(pkg):
    import torch
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(W, H)
    r = pkg.Renderer(sc, device=0)
    buf = torch.zeros((64, 6), dtype=torch.float64, device="cuda:0")
    px = torch.zeros((64, 6), dtype=torch.float64, device="cuda:0")
    hit = torch.zeros((64, 6), dtype=torch.float64, device="cuda:0")
    p, q, h = buf.data_ptr(), px.data_ptr(), hit.data_ptr()

    def refused(call, *words):
        with pytest.raises(pkg.RtError) as e:
            call()
        assert e.value.code == -1 and any(w in str(e.value) for w in words) and "rt_shade_rays" in str(e.value), str(e.value)
    refused(lambda: r.shade_into(None, 4, q), "null")
    refused(lambda: r.shade_into(p, 4, None), "null")
    refused(lambda: r.shade_into(p, 0, q), "n is 0")
    refused(lambda: r.shade(np.zeros((0, 3)), np.zeros((0, 3))), "n is 0")
    refused(lambda: r.shade_into(p + 8, 4, q), "aligned")
    refused(lambda: r.shade_into(p, 4, q + 8), "aligned")
    refused(lambda: r.shade_into(p, 4, q, h + 8), "aligned")
    refused(lambda: r.shade_into(p, 8, p), "overlap")
    refused(lambda: r.shade_into(p, 8, p + 48 * 7), "overlap")          # rgba inside the rays
    refused(lambda: r.shade_into(p + 16 * 7, 8, p), "overlap")          # rays begin inside the rgba
    refused(lambda: r.shade_into(p, 8, q, p + 48 * 7), "overlap")       # hits over the rays
    refused(lambda: r.shade_into(p + 48 * 7, 8, q, p), "overlap")
    refused(lambda: r.shade_into(p, 8, q, q + 16 * 7), "overlap")       # hits over the rgba
    refused(lambda: r.shade_into(p, 8, q + 48 * 7, q), "overlap")
    assert pkg.lib().rt_shade_rays_host(r._h, None, 4, None, None) == -1 and b"null" in pkg.lib().rt_last_error()
    assert pkg.lib().rt_shade_rays(None, p, 4, q, None, None, None) == -1 and b"null" in pkg.lib().rt_last_error()
    r.shade_into(p, 8, p + 48 * 8, p + 48 * 8 + 16 * 8)   # adjacent ranges are fine
    r.cleanup_update()


def test_fast_build_statistics(pkg, oracle):
    """FAST against strict on the primary rays of three scenes: only what holds by construction is asserted -- a ray that misses in
    both builds is exactly the background with alpha 1.0f -- and the share of differing colours is printed."""
    for name in ("20spheres", "reflection_test", "clebsch"):
        w, h = 160, 90
        sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
        osc = oracle.load_scene(scene_path(name)).with_size(w, h)
        rays = rays_ref.primary_rays(osc)
        ra, rb = pkg.Renderer(sc, device=0), pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_FAST)
        (a, arec), (b, brec) = shade_dev(ra, rays, hits=True), shade_dev(rb, rays, hits=True)
        ra.cleanup_update()
        rb.cleanup_update()
        miss = brec["object"] < 0
        bg = np.append(np.asarray(osc.bg_color, dtype=np.float32), F(1.0))
        assert miss.any() and np.all(bits(b[miss]) == bits(bg)) and np.all(bits(b[:, 3]) == bits(F(1.0)))
        differ = (bits(a) != bits(b)).any(axis=-1)
        print(f"FAST vs strict rt_shade_rays, {name} {w}x{h}: colour differs at {int(differ.sum())} of {len(rays)} rays ({100.0 * differ.mean():.3f} %), "
              f"largest channel difference {float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))):.3e}, object differs at {int((arec['object'] != brec['object']).sum())}")
