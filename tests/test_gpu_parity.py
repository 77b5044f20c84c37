"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on identical scene / camera.

Bar (BASELINE.json north_star): every channel within 1e-5 relative of update-cpu.cpp's value.  The strict
kernel computes the same IEEE operations in the same order as the oracle for surfaces of degree <= 2, so
there the frames are expected to be BIT-IDENTICAL (asserted); degree-3 surfaces go through device cbrt /
acos / cos, which differ from glibc's in the last ulp, so they are held to the 1e-5 bar -- with a few flipped pixels
against the plain oracle, with none against the oracle under the device's cbrt / acos / cos
(tests/tools/cubic_device_lab.py).
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, compare, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cubic_device_lab as D  # noqa: E402  (the oracle under the device's cbrt / acos / cos)

pytestmark = pytest.mark.gpu

QUADRIC = ["quadratic", "20spheres", "reflection_test"]
CUBIC = ["clebsch", "cubic", "cayley", "dingdong", "monkey_saddle"]


def render_gpu(pkg, name, w, h, max_refl=None, cam=None, **kw):
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
    if max_refl is not None:
        sc.set_max_reflections(max_refl)
    r = pkg.Renderer(sc, device=0, **kw)
    ms = r.update(cam)
    img = r.download()
    cnt = r.counters() if kw.get("flags", 0) & pkg.RT_FLAG_COUNT else None
    r.cleanup_update()
    return img, ms, cnt


def render_cpu(oracle, name, w, h, max_refl=None, cam=None, counters=False):
    s = oracle.load_scene(scene_path(name)).with_size(w, h, max_refl)
    return s.render(cam=cam, counters=counters, nthreads=8)


@pytest.mark.parametrize("name", QUADRIC)
def test_quadric_scenes_bit_identical(pkg, oracle, name):
    w, h = 320, 240
    got, _, _ = render_gpu(pkg, name, w, h, 4)
    want = render_cpu(oracle, name, w, h, 4)
    assert np.all(got[..., 3] == 1.0)
    c = compare(got[..., :3], want)
    assert c["identical"], c


@pytest.mark.parametrize("name", CUBIC)
def test_cubic_scenes_within_tolerance(pkg, oracle, name):
    w, h = 320, 240
    got, _, _ = render_gpu(pkg, name, w, h)
    want = render_cpu(oracle, name, w, h)
    c = compare(got[..., :3], want)
    # pixels sitting on a solver discontinuity may flip on a last-ulp difference of cbrt/acos/cos; the
    # bound is what SURVEY.md section 7 measured between two CPU builds of the reference itself (<= 0.04 % of pixels)
    assert c["n_bad_pixels"] <= max(2, int(0.0004 * w * h)), c
    # with the device's cbrt / acos / cos in the oracle's solver nothing is left to flip: no pixel beyond 1e-5
    c = D.compare_device_libm(pkg, got[..., :3], oracle.load_scene(scene_path(name)).with_size(w, h))
    assert c["n_bad_pixels"] == 0, c


def test_counters_match_oracle(pkg, oracle):
    w, h = 480, 270
    for name, mr in (("20spheres", None), ("reflection_test", 4), ("clebsch", None)):
        _, _, cnt = render_gpu(pkg, name, w, h, mr, flags=pkg.RT_FLAG_COUNT)
        _, ocnt = render_cpu(oracle, name, w, h, mr, counters=True)
        for k in ("primary_rays", "shadow_rays", "reflect_rays"):
            assert cnt[k] == ocnt[k], (name, k, cnt, ocnt)
        if name != "clebsch":
            assert cnt["tests"] == ocnt["tests"], (name, cnt, ocnt)
            assert cnt["hits"] == ocnt["normals"], (name, cnt, ocnt)


def test_moved_camera(pkg, oracle):
    cam = oracle.camera_matrix(pos=(1.5, 2.0, -3.0), yaw_deg=78.0, pitch_deg=9.0)
    w, h = 256, 192
    got, _, _ = render_gpu(pkg, "20spheres", w, h, cam=cam)
    want = render_cpu(oracle, "20spheres", w, h, cam=cam)
    assert compare(got[..., :3], want)["identical"]


def test_band_sharding_reassembles_bit_identical(pkg):
    """world=3 contexts on one GPU + rt_assemble == the world=1 frame (ragged height: 250 rows, bands of 8)."""
    import torch
    w, h, world = 200, 250, 3
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(w, h)
    full = pkg.Renderer(sc, device=0)
    full.update()
    want = full.download()
    rs = [pkg.Renderer(sc, device=0, rank=r, world=world, band_rows=8) for r in range(world)]
    mx = rs[0].max_local_rows
    gathered = torch.zeros((world, mx, w, 4), dtype=torch.float32, device="cuda:0")
    for r, ren in enumerate(rs):
        assert ren.local_rows == len(pkg.band_rows_of_rank(h, 8, world, r))
        assert np.array_equal(ren.row_map(), pkg.band_rows_of_rank(h, 8, world, r))
        ren.update(dev_fb=gathered[r].data_ptr())
    out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    rs[0].assemble(gathered.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


def test_rgba8_within_one_lsb(pkg, oracle):
    """The quantisation is defined exactly -- (unsigned char) (int) (v * 255.0f + 0.5f) in FP32 -- so the RGBA8 frame is held to
    that rule applied to the RGBA32F frame of the same configuration and to the oracle's frame, not to one LSB."""
    from test_raw_descriptor_gpu import check_rgba8, rgba8_of
    w, h = 320, 240
    got, _, _ = render_gpu(pkg, "20spheres", w, h, fmt=pkg.RT_FMT_RGBA8)
    v32, _, _ = render_gpu(pkg, "20spheres", w, h)
    want = render_cpu(oracle, "20spheres", w, h)
    assert got.dtype == np.uint8 and np.all(got[..., 3] == 255)
    check_rgba8(got, v32, "20spheres against its RGBA32F frame")
    q, ok = rgba8_of(want)
    assert ok.all() and np.array_equal(got, q)
    assert np.abs(got[..., :3].astype(np.int32) - np.floor(want * 255.0 + 0.5).astype(np.int32)).max() <= 1


def test_fast_variant_statistics(pkg, oracle):
    """FMA-contracted build: same algorithm, <=1 ulp per operation; report (and bound) the flips."""
    w, h = 320, 240
    for name in QUADRIC + CUBIC:
        got, _, _ = render_gpu(pkg, name, w, h, flags=pkg.RT_FLAG_FAST)
        want = render_cpu(oracle, name, w, h)
        c = compare(got[..., :3], want)
        assert c["n_bad_pixels"] <= max(2, int(0.002 * w * h)), (name, c)


def test_full_size_properties(pkg, oracle):
    """BASELINE config 2 at full size: ray counts equal SURVEY.md's table, frame is deterministic, and a
    sample of rows is bit-identical to the oracle."""
    w, h = 1920, 1080
    a, _, cnt = render_gpu(pkg, "20spheres", w, h, flags=pkg.RT_FLAG_COUNT)
    b, _, _ = render_gpu(pkg, "20spheres", w, h)
    assert np.array_equal(a, b)
    assert cnt["rays_total"] == 6754877 and cnt["tests"] == 121254919
    rows = np.arange(0, h, 37, dtype=np.uint32)
    want = oracle.load_scene(scene_path("20spheres")).with_size(w, h).render(rows=rows, nthreads=8)
    assert np.array_equal(a[rows][..., :3], want)
    # checksum anchor of SURVEY.md 8 work table (sum of all RGB channels in double)
    assert abs(float(a[..., :3].astype(np.float64).sum()) - 645483.747) < 0.01


def test_golden_frames(pkg):
    """HIP path against the committed oracle-rendered fixtures (tests/golden/frames_96x72.npz, two cameras)."""
    import os
    from conftest import ROOT
    g = np.load(os.path.join(ROOT, "tests", "golden", "frames_96x72.npz"))
    for key in g.files:
        if key.startswith("cam_"):
            continue
        name, cam = key.split("__")
        got, _, _ = render_gpu(pkg, name, 96, 72, cam=g["cam_" + cam])
        c = compare(got[..., :3], g[key])
        if name in QUADRIC:
            assert c["identical"], (key, c)
        else:
            assert c["n_bad_pixels"] <= 3, (key, c)


@pytest.mark.parametrize("depth", [0, 1, 3, 5])
def test_reflection_depth_limit(pkg, oracle, depth):
    """Two facing mirrors: every pixel bounces exactly max_reflections times; none of the
    reference's scenes reaches the limit, so this one is synthetic."""
    from test_oracle_units import two_mirror_scene
    osc = two_mirror_scene(oracle, depth)
    want, ocnt = osc.render(counters=True)
    d = pkg.desc_from_arrays(osc.width, osc.height, osc.vertical_fov, osc.bg_color, osc.max_reflections, osc.coefs,
                             osc.reflection, osc.albedo, osc.light_is_spherical, osc.light_p, osc.light_color)
    r = pkg.Renderer(d, device=0, flags=pkg.RT_FLAG_COUNT)
    r.update()
    got, cnt = r.download(), r.counters()
    r.cleanup_update()
    assert cnt["reflect_rays"] == ocnt["reflect_rays"] == depth * osc.width * osc.height
    assert cnt["tests"] == ocnt["tests"]
    assert np.array_equal(got[..., :3], want)


def test_update_h_drop_in_boundary(pkg, oracle, tmp_path):
    """A host written only against the reference's update.h / scene.h (tests/host_driver/update_driver.cpp),
    linked against libmi355rt_update.so, produces the oracle's frame."""
    import os
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "tests", "host_driver", "update_driver")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    cam = oracle.camera_matrix(pos=(0.5, 1.0, -2.0), yaw_deg=85.0, pitch_deg=5.0)
    out = str(tmp_path / "frame.f32")
    w, h = 200, 150
    p = subprocess.run([exe, scene_path("reflection_test"), str(w), str(h), "4", out] + [repr(float(v)) for v in cam],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert float(p.stdout.strip()) > 0.0
    got = np.fromfile(out, dtype=np.float32).reshape(h, w, 4)
    want = render_cpu(oracle, "reflection_test", w, h, 4, cam=cam)
    assert np.array_equal(got[..., :3], want) and np.all(got[..., 3] == 1.0)
    # loader errors surface as the reference's SceneException text on stderr, exit code 1 (src/ray-tracer.cpp:151-158)
    p = subprocess.run([exe, "/nonexistent.yml", "8", "8", "-1", out], capture_output=True, text=True)
    assert p.returncode == 1 and "Cannot read the file /nonexistent.yml" in p.stderr


def random_scene(pkg, seed, n_spheres, n_lights, w=160, h=120, with_plane=True, mirrors=False):
    """Synthetic stress scene: random spheres (some overlapping), a floor plane, directional + point lights."""
    rng = np.random.default_rng(seed)
    s = pkg.Scene.new(w, h, float(rng.uniform(30, 80)), 3, (0.1, 0.2, 0.3))
    for i in range(n_spheres):
        c = rng.uniform([-12, -6, 6], [12, 8, 40])
        r = float(rng.uniform(0.3, 3.0))
        s.add_object(pkg.surface_make("sphere", c, [r]), rng.uniform(0, 1, 3), float(rng.uniform(0.2, 0.8)) if (mirrors and i % 3 == 0) else 0.0)
    if with_plane:
        s.add_object(pkg.surface_make("plane", [0, -7, 0], [0.05, 1, 0.02]), (0.5, 0.5, 0.5), 0.4 if mirrors else 0.0)
    for i in range(n_lights):
        if i % 2 == 0:
            s.add_light("directional", rng.normal(size=3) + np.array([0, -1.5, 0]), rng.uniform(0, 1, 3), float(rng.uniform(0.2, 1.5)))
        else:
            s.add_light("spherical", rng.uniform([-15, 0, 0], [15, 20, 40]), rng.uniform(0, 1, 3), float(rng.uniform(100, 900)))
    return s


def render_desc(pkg, sc, cam=None, **kw):
    """Three frames from one context: the first runs the tiles in index order, the later ones in the launch order fed
    back by the frame before (rt_wavefront.hip, "launch order from the previous frame"); the image must not notice."""
    r = pkg.Renderer(sc, device=0, **kw)
    r.update(cam)
    first = r.download().copy()
    r.update(cam)
    second = r.download().copy()
    r.update(cam)
    img = r.download()
    r.cleanup_update()
    assert np.array_equal(first, second) and np.array_equal(first, img), "frame changed with the launch order"
    return img


def oracle_from(pkg, oracle, sc):
    a = sc.arrays()
    o = oracle.Scene(a["width"], a["height"], 0.0, a["max_reflections"], a["bg_color"])
    o.vertical_fov = a["vertical_fov"]
    for i in range(len(a["reflection"])):
        o.add_object(a["coefs"][i], a["albedo"][i], a["reflection"][i])
    for i in range(len(a["light_is_spherical"])):
        l = oracle.OrcLight()
        l.is_spherical = int(a["light_is_spherical"][i])
        for k in range(3):
            l.p[k] = float(a["light_p"][i][k])
            l.color[k] = float(a["light_color"][i][k])
        o.lights.append(l)
    return o


@pytest.mark.parametrize("seed", range(12))
def test_culling_and_kernel_variants_agree_on_random_scenes(pkg, oracle, seed):
    """Wavefront kernel with culling == without culling == simple kernel == oracle, bit for bit, on random sphere
    fields (up to 70 objects: more than one 64-object chunk) with mixed light kinds, mirrors and moved cameras."""
    n_s = [3, 8, 20, 40, 70, 12][seed % 6]
    sc = random_scene(pkg, seed, n_s, 1 + seed % 7, mirrors=seed % 2 == 1)
    cam = oracle.camera_matrix(pos=(seed * 0.3 - 1.0, 0.5, -4.0), yaw_deg=90.0 + 2 * seed, pitch_deg=-3.0 + seed) if seed % 3 else None
    a = render_desc(pkg, sc, cam)
    b = render_desc(pkg, sc, cam, flags=pkg.RT_FLAG_NOCULL)
    c = render_desc(pkg, sc, cam, flags=pkg.RT_FLAG_SIMPLE)
    assert np.array_equal(a, b), "culling changed pixels"
    assert np.array_equal(a, c), "default path and simple kernel disagree"
    want = oracle_from(pkg, oracle, sc).render(cam=cam, nthreads=8)
    assert np.array_equal(a[..., :3], want)


def test_kernel_variants_agree_on_reference_scenes(pkg):
    for name in QUADRIC + CUBIC:
        sc = pkg.Scene.load_from_file(scene_path(name)).set_size(256, 192)
        a = render_desc(pkg, sc)
        assert np.array_equal(a, render_desc(pkg, sc, flags=pkg.RT_FLAG_SIMPLE)), name
        assert np.array_equal(a, render_desc(pkg, sc, flags=pkg.RT_FLAG_NOCULL)), name


def test_counters_identical_across_kernels(pkg):
    """Reference-equivalent ray / test counts do not depend on the kernel or on culling."""
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(480, 270)
    out = []
    for fl in (0, pkg.RT_FLAG_NOCULL, pkg.RT_FLAG_SIMPLE):
        r = pkg.Renderer(sc, device=0, flags=fl | pkg.RT_FLAG_COUNT)
        r.update()
        out.append(r.counters())
        r.cleanup_update()
    for k in ("primary_rays", "shadow_rays", "reflect_rays", "tests", "hits"):
        assert out[0][k] == out[1][k] == out[2][k], (k, out)
    assert out[0]["tests_executed"] < out[1]["tests_executed"]  # culling removes work


def _check_against_oracle(pkg, oracle, sc, cam=None, exact=True):
    got = render_desc(pkg, sc, cam)
    assert np.array_equal(got, render_desc(pkg, sc, cam, flags=pkg.RT_FLAG_SIMPLE))
    assert np.array_equal(got, render_desc(pkg, sc, cam, flags=pkg.RT_FLAG_NOCULL))
    want = oracle_from(pkg, oracle, sc).render(cam=cam, nthreads=4)
    if exact:
        assert np.array_equal(got[..., :3], want)
    else:
        assert compare(got[..., :3], want)["n_bad_pixels"] <= 2
    return got


def test_edge_cases(pkg, oracle):
    """Empty and ragged inputs: no objects, no lights, 1x1 and odd-sized images, more than 32 lights (two shadow
    words), more than 64 spheres (two table groups), a camera inside a sphere, a point light inside a sphere."""
    # no objects at all: every pixel is background
    s = pkg.Scene.new(37, 19, 50.0, 2, (0.3, 0.6, 0.9))
    s.add_light("directional", [0, -1, 0])
    g = _check_against_oracle(pkg, oracle, s)
    assert np.allclose(g[..., :3], [0.3, 0.6, 0.9])
    # objects but no lights: hits are black (src/update-cpu.cpp:58,77)
    s = pkg.Scene.new(33, 17, 50.0, 2, (0.3, 0.6, 0.9))
    s.add_object(pkg.surface_make("sphere", [0, 0, 10], [3.0]), (1, 1, 1))
    g = _check_against_oracle(pkg, oracle, s)
    assert g[8, 16, 0] == 0.0 and g[0, 0, 2] == np.float32(0.9)
    # 1x1 image, 3x1 image
    for w, h in ((1, 1), (3, 1), (1, 5)):
        s = random_scene(pkg, 5, 6, 3, w=w, h=h)
        _check_against_oracle(pkg, oracle, s)
    # 40 lights (two 32-bit shadow words per hit), 70 + 1 objects (two 64-entry table groups), mirrors on
    s = random_scene(pkg, 21, 70, 40, w=96, h=64, mirrors=True)
    _check_against_oracle(pkg, oracle, s)
    # camera inside a big sphere (every primary ray hits from inside; normals are not flipped)
    s = pkg.Scene.new(64, 48, 60.0, 2, (0.1, 0.1, 0.1))
    s.add_object(pkg.surface_make("sphere", [0, 0, 0], [50.0]), (0.9, 0.8, 0.7))
    s.add_object(pkg.surface_make("sphere", [1, 0, 8], [1.0]), (0.2, 0.9, 0.2), 0.5)
    s.add_light("spherical", [0, 5, 4], (1, 1, 1), 500.0)
    s.add_light("directional", [0.2, -1, 0.3], (1, 1, 1), 1.0)
    _check_against_oracle(pkg, oracle, s)
    # point light inside one of the spheres, spheres touching / overlapping
    s = pkg.Scene.new(80, 60, 45.0, 3, (0.0, 0.0, 0.0))
    for c, r in (([0, 0, 10], 2.0), ([2.0, 0, 10], 2.0), ([4.0, 0, 10], 2.0), ([0, 4.0, 10], 2.0), ([0, -4, 12], 2.5), ([8, 1, 14], 3.0)):
        s.add_object(pkg.surface_make("sphere", c, [r]), (0.8, 0.8, 0.8), 0.3)
    s.add_light("spherical", [0, 0, 10], (1, 1, 1), 300.0)
    s.add_light("spherical", [3, 6, 2], (1, 0.5, 0.5), 600.0)
    _check_against_oracle(pkg, oracle, s)


def test_huge_coordinates_do_not_break_culling(pkg, oracle):
    """The culling margins carry a term for the cancellation error of the reference's own t0 at large coordinates:
    a sphere field translated by 1e6 still renders exactly like the simple kernel and the oracle."""
    rng = np.random.default_rng(3)
    off = np.array([1.0e6, -2.0e6, 3.0e6])
    s = pkg.Scene.new(96, 72, 50.0, 2, (0.1, 0.2, 0.3))
    for i in range(12):
        c = rng.uniform([-8, -5, 8], [8, 5, 30]) + off
        s.add_object(pkg.surface_make("sphere", c, [float(rng.uniform(0.5, 2.5))]), rng.uniform(0, 1, 3))
    s.add_light("directional", [0.3, -1.0, 0.4], (1, 1, 1), 1.0)
    s.add_light("spherical", np.array([0.0, 12.0, 5.0]) + off, (1, 1, 1), 800.0)
    cam = np.eye(4).reshape(16).copy()
    cam[12:15] = off  # camera translated with the scene (column-major: last column)
    _check_against_oracle(pkg, oracle, s, cam=cam)


def test_general_quadrics_and_planes(pkg, oracle):
    """Ellipsoid, hyperboloid (negative leading coefficient: Q5 quirk), paraboloid, cross terms, planes: the GQ / LIN
    table paths of the wavefront kernel."""
    s = pkg.Scene.new(120, 90, 55.0, 3, (0.2, 0.3, 0.4))
    q = np.zeros(20); q[10], q[11], q[12], q[19] = 1.0, 4.0, 0.5, -9.0; q[18] = -6.0       # ellipsoid-ish, shifted in z
    s.add_object(q, (0.9, 0.3, 0.3))
    q = np.zeros(20); q[10], q[11], q[12], q[19] = -1.0, 1.0, -1.0, 1.0; q[16], q[18] = 0.5, 12.0  # hyperboloid, t2 < 0 on many rays
    s.add_object(q, (0.3, 0.9, 0.3), 0.4)
    q = np.zeros(20); q[10], q[12], q[17], q[19] = 0.1, 0.1, 1.0, 20.0                     # the paraboloid of quadratic.yml
    s.add_object(q, (0.8, 0.8, 0.0))
    q = np.zeros(20); q[10], q[11], q[12], q[13], q[14], q[15], q[19] = 1.0, 2.0, 1.5, 0.5, -0.3, 0.2, -30.0; q[18] = -10.0
    s.add_object(q, (0.3, 0.3, 0.9))                                                        # cross terms
    s.add_object(pkg.surface_make("plane", [0, -6, 0], [0, 1, 0.05]), (0.5, 0.5, 0.5), 0.3)
    s.add_object(pkg.surface_make("sphere", [3, 1, 9], [1.2]), (0.9, 0.9, 0.9))
    s.add_light("directional", [0.4, -1.0, 0.3], (1, 1, 1), 1.2)
    s.add_light("spherical", [-4, 6, 2], (1, 0.8, 0.6), 500.0)
    for cam in (None, oracle.camera_matrix(pos=(1.0, 1.0, -3.0), yaw_deg=95.0, pitch_deg=4.0)):
        _check_against_oracle(pkg, oracle, s, cam=cam)


def test_fly_through_sequence(pkg, oracle):
    """A moving-camera sequence (the host loop of src/ray-tracer.cpp:220-233, headless): every frame equals the
    oracle's frame for the same pose; one context renders the whole sequence (state does not leak between frames)."""
    w, h = 192, 108
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(w, h)
    osc = oracle.load_scene(scene_path("20spheres")).with_size(w, h)
    r = pkg.Renderer(sc, device=0)
    for i in range(8):
        cam = pkg.camera_matrix(pos=(0.4 * i - 1.0, 0.2 * i, -0.5 * i), yaw_deg=90.0 + 3.0 * i, pitch_deg=-2.0 + 1.5 * i)
        r.update(cam)
        assert np.array_equal(r.download()[..., :3], osc.render(cam=cam, nthreads=8)), i
    r.cleanup_update()


def _orbit_pose(pkg, i, n=24):
    a = 2.0 * np.pi * i / n
    pos = (5.0 + 14.0 * np.sin(a), 2.0 + 2.0 * np.sin(2 * a), 15.0 - 14.0 * np.cos(a))
    return pkg.camera_matrix(pos, float(np.degrees(np.arctan2(15.0 - pos[2], 5.0 - pos[0]))), float(-np.degrees(np.arctan2(pos[1] - 2.0, 14.0))))


@pytest.mark.parametrize("pose", [3, 5, 6, 19])
def test_box_stage_culling_on_orbit_poses(pkg, oracle, pose):
    """Views along the rows of 20spheres.yml: tiles whose 64-hit chunks span a near and a far sphere (long thin bounding box, fat
    bounding ball), where the shadow phase's second culling stage (crec_in_box_shadow, rt_wavefront_math.hpp) runs.  The frame
    must equal the oracle's and the frames of the kernels without that stage."""
    w, h = 480, 270
    cam = _orbit_pose(pkg, pose)
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(w, h)
    got = render_desc(pkg, sc, cam)
    assert np.array_equal(got, render_desc(pkg, sc, cam, flags=pkg.RT_FLAG_NOCULL))
    assert np.array_equal(got, render_desc(pkg, sc, cam, flags=pkg.RT_FLAG_SIMPLE))
    assert np.array_equal(got[..., :3], oracle.load_scene(scene_path("20spheres")).with_size(w, h).render(cam=cam, nthreads=8))


@pytest.mark.parametrize("seed", range(6))
def test_box_stage_culling_on_sphere_rows(pkg, oracle, seed):
    """Constructed for the box stage: rows of spheres receding from the camera (every tile on a silhouette sees a near and a far
    one) and directional lights, some of them along the rows, so that many spheres lie near every chunk's axis."""
    rng = np.random.default_rng(7000 + seed)
    s = pkg.Scene.new(256, 160, 55.0, 0, (0.05, 0.1, 0.2))
    for row in range(3):
        x0, y0 = float(rng.uniform(-3, 3)), float(rng.uniform(-2, 2))
        for k in range(int(rng.integers(6, 10))):
            z = 6.0 + 3.2 * k
            s.add_object(pkg.surface_make("sphere", [x0 + 0.35 * k * (row - 1) + float(rng.normal(0, 0.1)), y0 + 0.25 * k, z], [float(rng.uniform(0.8, 1.4))]),
                         rng.uniform(0.2, 1, 3), 0.0)
    for i in range(12):
        d = np.array([0.1 * (i - 6), -0.3 - 0.05 * i, -1.0 + 0.15 * i]) if i % 2 == 0 else rng.normal(size=3) + np.array([0, -1.0, 0])
        s.add_light("directional", d, rng.uniform(0.2, 1, 3), float(rng.uniform(0.2, 0.8)))
    s.add_light("spherical", [0.0, 12.0, 10.0], (1, 1, 1), 300.0)
    _check_against_oracle(pkg, oracle, s)
    # the stage really ran: a counting render books its evaluations as directional decisions, three each (rt_wavefront.hip)
    r = pkg.Renderer(s, device=0, flags=pkg.RT_FLAG_COUNT)
    r.update()
    d = r.counters_detail()
    r.cleanup_update()
    assert d["cull_by_kind"]["shadow_directional"] > 0


@pytest.mark.parametrize("pose", [-1, 5, 6, 16])
def test_half_tiles_do_not_change_the_frame(pkg, oracle, pose):
    """The costliest tiles of the previous frame are rendered by two workgroups, rows 0-7 and rows 8-15 (rt_wavefront.hip, "half
    tiles"), while the GPU has workgroup slots to spare -- which at these sizes it always has.  Frames with and without
    (RT_FLAG_NOSPLIT) must be identical, frame after frame, and equal the oracle's."""
    w, h = 640, 360
    cam = None if pose < 0 else _orbit_pose(pkg, pose)
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(w, h)
    want = oracle.load_scene(scene_path("20spheres")).with_size(w, h).render(cam=cam, nthreads=8)
    ra, rb = pkg.Renderer(sc, device=0), pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_NOSPLIT)
    for frame in range(6):   # the split starts with the second frame (it needs the first one's costs) and feeds back into the third ...
        ra.update(cam)
        rb.update(cam)
        a, b = ra.download(), rb.download()
        assert np.array_equal(a, b), frame
        assert np.array_equal(a[..., :3], want), frame
    ra.cleanup_update()
    rb.cleanup_update()


@pytest.mark.parametrize("name,depth", [("reflection_test", 4), ("quadratic", None), ("clebsch", None)])
def test_half_tiles_on_the_other_surface_classes(pkg, name, depth):
    """Mirrors, general quadrics, the cubic: the same frames with and without half tiles."""
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(512, 288)
    if depth is not None:
        sc.set_max_reflections(depth)
    ra, rb = pkg.Renderer(sc, device=0), pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_NOSPLIT)
    for frame in range(5):
        ra.update()
        rb.update()
        assert np.array_equal(ra.download(), rb.download()), frame
    ra.cleanup_update()
    rb.cleanup_update()


def mixed_scene(pkg, seed, w=128, h=96):
    """Random mix of every degree <= 2 class: spheres, ellipsoids / hyperboloids / paraboloids with cross terms, planes;
    directional and point lights; some mirrors."""
    rng = np.random.default_rng(1000 + seed)
    s = pkg.Scene.new(w, h, float(rng.uniform(35, 75)), int(rng.integers(0, 4)), rng.uniform(0, 1, 3))
    for i in range(int(rng.integers(2, 14))):
        kind = rng.integers(0, 4)
        refl = float(rng.uniform(0.1, 0.9)) if rng.random() < 0.3 else 0.0
        col = rng.uniform(0, 1, 3)
        if kind <= 1:
            s.add_object(pkg.surface_make("sphere", rng.uniform([-10, -6, 5], [10, 8, 35]), [float(rng.uniform(0.3, 3.0))]), col, refl)
        elif kind == 2:
            q = np.zeros(20)
            q[10:13] = rng.uniform(-1.5, 2.0, 3)
            if rng.random() < 0.5:
                q[13:16] = rng.uniform(-0.5, 0.5, 3)
            c = rng.uniform([-6, -4, 8], [6, 4, 25])
            q[16:19] = -2.0 * q[10:13] * c
            q[19] = float(np.dot(q[10:13], c * c) - rng.uniform(0.5, 6.0))
            s.add_object(q, col, refl)
        else:
            n = rng.normal(size=3)
            s.add_object(pkg.surface_make("plane", rng.uniform([-5, -8, 0], [5, -3, 30]), n / np.linalg.norm(n) + np.array([0, 1.5, 0])), col, refl)
    for i in range(int(rng.integers(1, 6))):
        if rng.random() < 0.5:
            s.add_light("directional", rng.normal(size=3) + np.array([0, -1.2, 0]), rng.uniform(0, 1, 3), float(rng.uniform(0.3, 1.5)))
        else:
            s.add_light("spherical", rng.uniform([-12, -2, -5], [12, 15, 35]), rng.uniform(0, 1, 3), float(rng.uniform(100, 900)))
    return s


@pytest.mark.parametrize("seed", range(24))
def test_random_mixed_class_scenes_bit_identical(pkg, oracle, seed):
    """Every kernel instantiation for degree <= 2 (with / without general quadrics, with / without mirrors) against the
    simple kernel and the oracle on random mixed scenes -- bit for bit."""
    sc = mixed_scene(pkg, seed)
    cam = pkg.camera_matrix(pos=(0.3 * (seed % 5) - 0.6, 0.2 * (seed % 3), -1.0 * (seed % 4)), yaw_deg=90.0 + (seed % 7) - 3, pitch_deg=(seed % 5) - 2.0)
    a = render_desc(pkg, sc, cam)
    assert np.array_equal(a, render_desc(pkg, sc, cam, flags=pkg.RT_FLAG_SIMPLE)), "wavefront vs simple"
    want = oracle_from(pkg, oracle, sc).render(cam=cam, nthreads=8)
    assert np.array_equal(a[..., :3], want)


def random_cubic_scene(pkg, seed, w=128, h=96):
    """A random degree-3 surface next to a sphere and a plane, two lights; returns (scene, camera)."""
    rng = np.random.default_rng(500 + seed)
    s = pkg.Scene.new(w, h, 40.0, 2, (0.05, 0.1, 0.15))
    q = np.zeros(20)
    q[:10] = rng.uniform(-1, 1, 10) * (rng.random(10) < 0.6)
    q[10:16] = rng.uniform(-1, 1, 6)
    q[16:19] = rng.uniform(-2, 2, 3)
    q[19] = rng.uniform(-4, 4)
    # move it in front of the camera: substitute z -> z - 12 by sampling the translated polynomial is overkill; use the
    # camera instead (the camera matrix is an input of the path)
    s.add_object(q, (0.8, 0.8, 0.8), 0.3 if seed % 2 else 0.0)
    s.add_object(pkg.surface_make("sphere", [1.5, 0.5, 2.0], [0.7]), (0.9, 0.3, 0.2))
    s.add_object(pkg.surface_make("plane", [0, -3, 0], [0, 1, 0]), (0.4, 0.5, 0.4))
    s.add_light("directional", [0.3, -1.0, 0.5], (1, 1, 1), 1.5)
    s.add_light("spherical", [2.0, 4.0, -6.0], (1, 0.9, 0.8), 300.0)
    return s, pkg.camera_matrix(pos=(0.5, 1.0, -9.0), yaw_deg=92.0, pitch_deg=-4.0)


@pytest.mark.parametrize("seed", range(6))
def test_random_cubic_scenes_within_tolerance(pkg, oracle, seed):
    """Random degree-3 surfaces next to spheres and a plane (the cubic + mixed instantiations).  Device cbrt / acos / cos
    differ from glibc's in the last ulp, so the bar is 1e-5 relative with at most 0.2 % of the pixels flipping at solver
    discontinuities; wavefront and simple kernels must still agree exactly (same device functions)."""
    w, h = 128, 96
    s, cam = random_cubic_scene(pkg, seed, w, h)
    a = render_desc(pkg, s, cam)
    assert np.array_equal(a, render_desc(pkg, s, cam, flags=pkg.RT_FLAG_SIMPLE))
    osc = oracle_from(pkg, oracle, s)
    want = osc.render(cam=cam, nthreads=8)
    c = compare(a[..., :3], want)
    assert c["n_bad_pixels"] <= max(3, int(0.002 * w * h)), c
    c = D.compare_device_libm(pkg, a[..., :3], osc, cam=cam)   # (the oracle under the device's cbrt / acos / cos: no pixel beyond 1e-5)
    assert c["n_bad_pixels"] == 0, c


@pytest.mark.parametrize("seed", [158, 534] + list(range(2000, 2040)))
def test_fuzz_regressions_and_sample(pkg, oracle, seed):
    """tests/tools/fuzz_parity.py scenes: odd image sizes (down to 1 pixel), scene scales 0.1 .. 100, huge / tiny /
    imaginary spheres, random quadrics, planes, mirrors, both light kinds, random cameras.  Seeds 158 and 534 are the
    two scenes (106x2 and 71x3 pixels, cones wider than a half-space) on which the fuzzer caught the primary cone
    culling before it was guarded."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tests", "tools", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    s, cam = fz.scene(seed)
    a = render_desc(pkg, s, cam)
    assert np.array_equal(a, render_desc(pkg, s, cam, flags=pkg.RT_FLAG_NOCULL))
    assert np.array_equal(a, render_desc(pkg, s, cam, flags=pkg.RT_FLAG_SIMPLE))
    assert np.array_equal(a[..., :3], oracle_from(pkg, oracle, s).render(cam=cam, nthreads=4), equal_nan=True)


@pytest.mark.parametrize("h,band,world", [(37, 1, 2), (50, 3, 4), (64, 5, 3), (129, 16, 8), (100, 33, 2), (16, 8, 5), (7, 2, 6)])
def test_row_band_ownership_variants(pkg, h, band, world):
    """Any band height / rank count (bands that do not divide the tile height make a wave's four rows non-contiguous in
    the image): every rank's local rows equal the corresponding rows of the single-context frame."""
    w = 150
    sc = random_scene(pkg, 99, 14, 5, w=w, h=h, mirrors=True)
    full = render_desc(pkg, sc)
    seen = np.zeros(h, dtype=bool)
    for r in range(world):
        ren = pkg.Renderer(sc, device=0, rank=r, world=world, band_rows=band)
        rows = ren.row_map()
        assert np.array_equal(rows, pkg.band_rows_of_rank(h, band, world, r))
        ren.update()
        if len(rows):
            assert np.array_equal(ren.download(), full[rows]), (r, rows[:4])
            seen[rows] = True
        ren.cleanup_update()
    assert seen.all()


def camera_cut_sequence(pkg, mirrors=False):
    """(scene, views, (away, front, side)): cuts between an empty view, a full view and a partial one, so that the launch-order
    lists are stale, too short (truncated) and too long in turn."""
    sc = random_scene(pkg, 4242, 40, 6, w=640, h=360, with_plane=False, mirrors=mirrors)
    away = pkg.camera_matrix((0.0, 0.0, 0.0), -90.0, 0.0)
    front = pkg.camera_matrix((0.0, 0.0, 0.0), 90.0, 0.0)
    side = pkg.camera_matrix((14.0, 2.0, 20.0), 160.0, -5.0)
    return sc, [away, away, front, front, front, front, side, front, away, side, side, front], (away, front, side)


def test_launch_order_feedback_survives_camera_cuts(pkg, oracle):
    """The launch order comes from the previous frame and the number of list slots from an even older one: cut between
    an empty view, a full view and a partial one so that the lists are stale, too short (truncated) and too long in
    turn.  Every frame equals the one an index-order context renders, and the first full one equals the oracle."""
    sc, seq, (away, front, side) = camera_cut_sequence(pkg)
    r = pkg.Renderer(sc, device=0)
    ref = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_STATIC_ORDER)
    seen = {}
    for i, cam in enumerate(seq):
        r.update(cam)
        got = r.download().copy()
        key = cam.tobytes()
        if key not in seen:
            ref.update(cam)
            seen[key] = ref.download().copy()
        assert np.array_equal(got, seen[key]), f"frame {i}"
    want = oracle_from(pkg, oracle, sc).render(cam=front, nthreads=8)
    assert np.array_equal(seen[front.tobytes()][..., :3], want)
    bg = np.asarray(sc.arrays()["bg_color"], dtype=np.float32)
    assert np.all(seen[away.tobytes()][..., :3] == bg)          # the cuts really go through an empty frame
    assert np.any(seen[front.tobytes()][..., :3] != bg)


@pytest.mark.parametrize("name,flags", [("quadratic", 1), ("reflection_test", 0), ("20spheres", 1), ("reflection_test", 3)])
def test_first_kernel_of_a_fresh_process(pkg, name, flags):
    """A frame must not depend on what earlier launches left in scratch memory (tools/check_spills.py): render in a
    fresh process, where this kernel is the first GPU work at all, and compare with the simple kernel there."""
    import os
    import subprocess
    import sys
    tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "first_in_process.py")
    out = subprocess.run([sys.executable, tool, name, str(flags)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == "OK", out.stdout


def random_walk(pkg, seed, frames=14):
    """(scene, cameras): a sparse random sphere field (few tiles with hits, so the launch-order lists stay in use; mirrors on odd
    seeds) and a camera that drifts, jumps, looks away for a frame (the lists go stale) and stands still."""
    rng = np.random.default_rng(7000 + seed)
    w, h = int(rng.integers(300, 700)), int(rng.integers(200, 420))
    s = pkg.Scene.new(w, h, float(rng.uniform(40, 75)), 3, (0.2, 0.3, 0.4))
    n = int(rng.integers(3, 12))
    for i in range(n):
        c = rng.uniform([-14, -8, 10], [14, 8, 45])
        s.add_object(pkg.surface_make("sphere", c, [float(rng.uniform(0.4, 2.2))]), rng.uniform(0, 1, 3),
                     float(rng.uniform(0.2, 0.7)) if (seed % 2 and i % 3 == 0) else 0.0)
    for i in range(int(rng.integers(1, 6))):
        if i % 2:
            s.add_light("spherical", rng.uniform([-20, 5, -5], [20, 25, 30]), rng.uniform(0, 1, 3), float(rng.uniform(50, 400)))
        else:
            s.add_light("directional", rng.normal(size=3) + np.array([0, -1.5, 0]), rng.uniform(0, 1, 3), float(rng.uniform(0.3, 1.2)))
    pos, yaw, pitch = np.array([0.0, 0.0, 0.0]), 90.0, 0.0
    cams = []
    for frame in range(frames):
        kind = rng.integers(0, 4)
        if kind == 0:      # drift
            pos = pos + rng.normal(scale=0.3, size=3); yaw += float(rng.normal(scale=2.0))
        elif kind == 1:    # jump
            pos = rng.uniform([-10, -4, -5], [10, 6, 8]); yaw = float(rng.uniform(40, 140)); pitch = float(rng.uniform(-15, 15))
        # kind == 2: look away for one frame (empty frame, the lists go stale); kind == 3: stand still
        cams.append(pkg.camera_matrix(tuple(pos), -90.0 if kind == 2 else yaw, pitch))
    return s, cams


@pytest.mark.parametrize("seed", range(8))
def test_launch_order_feedback_random_walks(pkg, seed):
    """Sparse random sphere fields (few tiles with hits, so the launch-order lists stay in use) under a camera that
    drifts, jumps and comes back: every frame must equal the frame of an index-order context, bit for bit."""
    s, cams = random_walk(pkg, seed)
    r = pkg.Renderer(s, device=0)
    ref = pkg.Renderer(s, device=0, flags=pkg.RT_FLAG_STATIC_ORDER)
    hits_seen = 0
    for frame, cam in enumerate(cams):
        r.update(cam)
        ref.update(cam)
        a, b = r.download(), ref.download()
        assert np.array_equal(a, b), f"seed {seed} frame {frame}"
        hits_seen += int(np.any(a[..., :3] != np.asarray((0.2, 0.3, 0.4), dtype=np.float32)))
    assert hits_seen >= 2, "the walk never saw the scene"


def general_camera_case(pkg, seed, max_w=None, max_h=None):
    """(scene, camera): an all-sphere field under a scaled and sheared camera matrix, mirrored on every third seed; max_w / max_h
    cap the frame size (the matrix and the spheres stay the same)."""
    rng = np.random.default_rng(9100 + seed)
    n, lights, w, h = int(rng.integers(4, 30)), int(rng.integers(1, 7)), int(rng.integers(150, 400)), int(rng.integers(100, 300))
    sc = random_scene(pkg, 9100 + seed, n, lights, w=w if max_w is None else min(w, max_w), h=h if max_h is None else min(h, max_h),
                      with_plane=False, mirrors=bool(seed % 2))
    base = pkg.camera_matrix((float(rng.uniform(-3, 3)), float(rng.uniform(-2, 2)), float(rng.uniform(-4, 2))),
                             float(rng.uniform(70, 110)), float(rng.uniform(-10, 10))).reshape(4, 4).T.copy()   # row-major view
    lin = np.eye(3) + rng.normal(scale=0.25, size=(3, 3))          # shear + anisotropic scale
    if seed % 3 == 0:
        lin[:, 0] *= -1.0                                           # mirrored
    m = base.copy()
    m[:3, :3] = base[:3, :3] @ lin
    return sc, np.ascontiguousarray(m.T).reshape(16)                # back to column-major


@pytest.mark.parametrize("seed", range(6))
def test_general_camera_matrices_on_sphere_fields(pkg, oracle, seed):
    """update() takes any dmat4, not only the rigid ones the reference's host builds: scaled, sheared and mirrored
    camera matrices on all-sphere scenes (where the tile-level pyramid test uses the inverse transpose of the 3x3 part)
    must still match the oracle bit for bit."""
    sc, cam = general_camera_case(pkg, seed)
    got = render_desc(pkg, sc, cam)
    want = oracle_from(pkg, oracle, sc).render(cam=cam, nthreads=8)
    assert np.array_equal(got[..., :3], want)
    assert np.array_equal(got, render_desc(pkg, sc, cam, flags=pkg.RT_FLAG_SIMPLE))


@pytest.mark.parametrize("n", [65, 130, 200])
def test_many_spheres_without_a_plane(pkg, oracle, n):
    """All-sphere scenes with more than one 64-sphere group: the tile-level pyramid test, the per-wave cone and the
    shadow-phase culling all loop over groups; frames must match the oracle and the un-culled kernels bit for bit."""
    sc = random_scene(pkg, 31000 + n, n, 5, w=200, h=150, with_plane=False, mirrors=(n == 130))
    cam = pkg.camera_matrix((0.5, 1.0, -6.0), 88.0, -3.0)
    got = render_desc(pkg, sc, cam)
    assert np.array_equal(got[..., :3], oracle_from(pkg, oracle, sc).render(cam=cam, nthreads=8))
    assert np.array_equal(got, render_desc(pkg, sc, cam, flags=pkg.RT_FLAG_NOCULL))
    assert np.array_equal(got, render_desc(pkg, sc, cam, flags=pkg.RT_FLAG_SIMPLE))


@pytest.mark.parametrize("w,h,world,band,name", [(200, 250, 3, 8, "20spheres"), (333, 97, 2, 16, "20spheres"), (256, 160, 4, 5, "reflection_test"),
                                                 (64, 48, 1, 16, "quadratic")])
def test_sparse_transport_rebuilds_the_frame(pkg, w, h, world, band, name):
    """rt_pack_sparse + rt_assemble_sparse (tiles with content + ids, fixed-size messages) == the single-context RGBA8
    frame, for ragged sizes, widths that are not multiples of 4 or 16, bands that cut through tiles, and a frame where
    every tile has content; a capacity that is too small raises the overflow flag instead of writing out of bounds."""
    import torch
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
    full = pkg.Renderer(sc, device=0, fmt=pkg.RT_FMT_RGBA8)
    full.update()
    want = full.download()
    rs = [pkg.Renderer(sc, device=0, rank=r, world=world, band_rows=band, fmt=pkg.RT_FMT_RGBA8) for r in range(world)]
    n_tiles = max(((w + 15) // 16) * ((ren.local_rows + 15) // 16) for ren in rs)
    for cap in (n_tiles, max(1, n_tiles // 7)):
        nbytes = pkg.Renderer.sparse_bytes(cap)
        assert nbytes % 16 == 0
        msgs = torch.full((world, nbytes), 0xAB, dtype=torch.uint8, device="cuda:0")
        for r, ren in enumerate(rs):
            ren.update()
            ren.pack_sparse(msgs[r].data_ptr(), cap)
        out = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda:0")
        rs[0].assemble_sparse(msgs.data_ptr(), cap, out.data_ptr())
        torch.cuda.synchronize()
        hdr = msgs.cpu().numpy().view(np.uint32)[:, :2]
        if cap == n_tiles:
            assert not hdr[:, 1].any()
            assert np.array_equal(out.cpu().numpy(), want)
            # the device messages hold the same (id -> tile) pairs as the host-side mirror (the order is free) and the
            # mirror rebuilds the same frame from them
            bgw = pkg.bg_rgba8(sc.arrays()["bg_color"])
            words = msgs.cpu().numpy().view(np.uint32)
            off = (4 + cap + 3) & ~3
            for r, ren in enumerate(rs):
                ref = pkg.pack_sparse_numpy(ren.download(), ren.local_rows, bgw, cap)
                assert words[r][0] == ref[0]
                dev = {int(words[r][4 + j]): words[r][off + j * 256: off + (j + 1) * 256].tobytes() for j in range(int(words[r][0]))}
                host = {int(ref[4 + j]): ref[off + j * 256: off + (j + 1) * 256].tobytes() for j in range(int(ref[0]))}
                assert dev == host
            assert np.array_equal(pkg.assemble_sparse_numpy(words, w, h, band, world, bgw, cap), want)
        else:
            overflowed = hdr[:, 0] > cap
            assert np.array_equal(hdr[:, 1] != 0, overflowed)
            if not overflowed.any():
                assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("w,h,world,band,name", [(200, 250, 3, 8, "20spheres"), (333, 97, 2, 16, "20spheres"), (256, 160, 4, 5, "reflection_test"),
                                                 (640, 360, 1, 16, "20spheres")])
def test_render_sparse_equals_render_plus_pack(pkg, w, h, world, band, name):
    """rt_render_sparse writes the message itself (no framebuffer, no pack kernel): rebuilt on the root it must equal
    the dense RGBA8 frame, three frames in a row (launch-order feedback active), and a capacity that is too small must
    only raise the overflow flag."""
    import torch
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
    full = pkg.Renderer(sc, device=0, fmt=pkg.RT_FMT_RGBA8)
    full.update()
    want = full.download()
    rs = [pkg.Renderer(sc, device=0, rank=r, world=world, band_rows=band, fmt=pkg.RT_FMT_RGBA8) for r in range(world)]
    n_tiles = max(((w + 15) // 16) * ((ren.local_rows + 15) // 16) for ren in rs)
    for cap in (n_tiles, max(1, n_tiles // 9)):
        nbytes = pkg.Renderer.sparse_bytes(cap)
        for frame in range(3):
            msgs = torch.full((world, nbytes), 0xCD, dtype=torch.uint8, device="cuda:0")
            for r, ren in enumerate(rs):
                ren.update_sparse(msgs[r].data_ptr(), cap)
            out = torch.full((h, w, 4), 9, dtype=torch.uint8, device="cuda:0")
            rs[0].assemble_sparse(msgs.data_ptr(), cap, out.data_ptr())
            torch.cuda.synchronize()
            hdr = msgs.cpu().numpy().view(np.uint32)[:, :2]
            overflowed = hdr[:, 0] > cap
            assert np.array_equal(hdr[:, 1] != 0, overflowed), (cap, frame)
            if not overflowed.any():
                assert np.array_equal(out.cpu().numpy(), want), (cap, frame)
        if cap == n_tiles:
            assert not overflowed.any()


def test_incremental_sparse_assembly_follows_a_moving_camera(pkg):
    """rt_assemble_sparse_incremental keeps the frame buffer between frames and only repaints tiles that lost their content:
    cut between views (content appears, moves, disappears entirely, comes back) and compare every frame with the dense
    single-context frame."""
    import torch
    w, h, world, band = 400, 300, 3, 16
    sc = random_scene(pkg, 777, 9, 4, w=w, h=h, with_plane=False)
    sc2 = sc  # same scene for the RGBA8 contexts
    ref = pkg.Renderer(sc, device=0, fmt=pkg.RT_FMT_RGBA8)
    rs = [pkg.Renderer(sc2, device=0, rank=r, world=world, band_rows=band, fmt=pkg.RT_FMT_RGBA8) for r in range(world)]
    cap = max(((w + 15) // 16) * ((ren.local_rows + 15) // 16) for ren in rs)
    nbytes = pkg.Renderer.sparse_bytes(cap)
    msgs = torch.zeros((world, nbytes), dtype=torch.uint8, device="cuda:0")
    full = torch.full((h, w, 4), 3, dtype=torch.uint8, device="cuda:0")
    stamps = torch.full((rs[0].sparse_stamp_bytes(),), 0x5A, dtype=torch.uint8, device="cuda:0")   # garbage: tag 0 must clear it
    cams = [pkg.camera_matrix((0.0, 0.0, 0.0), 90.0, 0.0), pkg.camera_matrix((2.0, 0.5, 1.0), 80.0, 3.0), pkg.camera_matrix((0.0, 0.0, 0.0), -90.0, 0.0),
            pkg.camera_matrix((0.0, 0.0, 0.0), -90.0, 0.0), pkg.camera_matrix((-3.0, 1.0, 4.0), 100.0, -5.0), pkg.camera_matrix((0.0, 0.0, 0.0), 90.0, 0.0)]
    saw_content = 0
    for k, cam in enumerate(cams):
        for r, ren in enumerate(rs):
            ren.update_sparse(msgs[r].data_ptr(), cap, cam)
        rs[0].assemble_sparse_incremental(msgs.data_ptr(), cap, full.data_ptr(), stamps.data_ptr(), k)   # tag 0 first, then 1, 2, ...
        ref.update(cam)
        torch.cuda.synchronize()
        want = ref.download()
        assert np.array_equal(full.cpu().numpy(), want), f"frame {k}"
        saw_content += int(msgs.cpu().numpy().view(np.uint32)[:, 0].sum() > 0)
    assert 3 <= saw_content < len(cams)   # the sequence really has frames with and without content


def test_frames_issued_on_alternating_streams(pkg):
    """A context's frames depend on each other on the device (launch-order generations, tile words): rt_render orders a frame
    behind the previous one when the caller switches streams.  Eight frames of a moving camera, alternately on two streams,
    no host synchronisation in between; every frame equals an index-order context's frame."""
    import torch
    w, h = 640, 360
    sc = random_scene(pkg, 4242, 40, 6, w=w, h=h, with_plane=False)
    r = pkg.Renderer(sc, device=0)
    ref = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_STATIC_ORDER | pkg.RT_FLAG_NOSCAN)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(8)]
    cams = [pkg.camera_matrix((0.3 * k, 0.1 * k, -0.5 * k), 90.0 + 5.0 * (k % 3) - (180.0 if k == 4 else 0.0), 1.0 * k) for k in range(8)]
    for k, cam in enumerate(cams):
        r.update(cam, dev_fb=bufs[k].data_ptr(), stream=streams[k & 1].cuda_stream, timed=False)
    torch.cuda.synchronize()
    for k, cam in enumerate(cams):
        ref.update(cam)
        assert np.array_equal(bufs[k].cpu().numpy(), ref.download()), k
