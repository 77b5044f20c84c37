"""The kernels held to a build of the reference's own CPU path directly: no restatement in between.

Every other GPU module compares a kernel with oracle/rt_oracle.c; tests/test_oracle_vs_reference.py compares that oracle with the
programs oracle/Makefile.ref compiles from the reference's unmodified sources into oracle/_ref/.  Here the frame a kernel renders
through the C ABI is compared with the frame the reference's update() renders for the same scene and camera (tests/tools/ref_binary.py
runs the program: a CPU child process, one at a time, before the device work; it reads its scene from the test, never from a tree
outside the repository).

Bars: degree <= 2, strict build: the same bits (array_equal; a NaN only has to be a NaN on both sides).  Degree 3: DESIGN.md
section 3's bar as test_gpu_parity.test_cubic_scenes_within_tolerance states it -- conftest.compare's 1e-5 relative with the 1e-7
absolute floor per channel, at most max(2, 0.04 % of the pixels) beyond it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, compare, scene_path
from test_gpu_parity import CUBIC, QUADRIC
from test_oracle_vs_reference import OWN_EDGES, _own_edge_scenes, built_scene

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ref_binary as R  # noqa: E402

pytestmark = pytest.mark.gpu

MOVED = ((0.3, 0.2, -0.5), 80.0, 10.0)


@pytest.fixture(scope="module", autouse=True)
def ref_programs():
    return R.require()


def cubic_bound(w, h):
    return max(2, int(0.0004 * w * h))   # test_gpu_parity.test_cubic_scenes_within_tolerance


def variants(pkg):
    return {"wavefront": 0, "simple": pkg.RT_FLAG_SIMPLE, "nocull": pkg.RT_FLAG_NOCULL, "nolean": pkg.RT_FLAG_NOLEAN}


def frame(pkg, sc, cam, flags=0):
    """Two frames of one context (the second runs the tiles in the launch order the first fed back); both must be the same."""
    r = pkg.Renderer(sc, device=0, flags=flags)
    try:
        r.update(cam)
        first = r.download().copy()
        r.update(cam)
        img = r.download().copy()
    finally:
        r.cleanup_update()
    assert np.array_equal(first, img, equal_nan=True), "the frame changed with the launch order"
    assert np.all(img[..., 3] == 1.0)
    return img[..., :3]


def desc_of(pkg, osc):
    return pkg.desc_from_arrays(osc.width, osc.height, osc.vertical_fov, osc.bg_color, osc.max_reflections, osc.coefs, osc.reflection,
                                osc.albedo, osc.light_is_spherical, osc.light_p, osc.light_color)


def is_cubic(osc):
    return bool(np.any(np.asarray(osc.coefs, dtype=np.float64).reshape(-1, 20)[:, :10] != 0))


def lean_eligible(osc):
    """Unit spheres only, no mirrors: what the wave-per-block instantiation renders (rt_wavefront.hip, "the lean path")."""
    c = np.asarray(osc.coefs, dtype=np.float64).reshape(-1, 20)
    return len(c) > 0 and not c[:, :10].any() and not c[:, 13:16].any() and bool(np.all(c[:, 10:13] == 1.0)) and not np.any(np.asarray(osc.reflection) > 1e-7)


def hold_to_reference(pkg, sc, want, cam, cubic, what):
    """Every kernel variant's frame of `sc` against the reference's frame `want`.  Returns the number of frames compared."""
    h, w = want.shape[:2]
    n = 0
    for vname, flags in variants(pkg).items():
        got = frame(pkg, sc, cam, flags)
        if cubic:
            c = compare(got, want)
            assert c["n_bad_pixels"] <= cubic_bound(w, h), (what, vname, c)
        else:
            assert np.array_equal(got, want, equal_nan=True), (what, vname, int((got != want).any(-1).sum()))
        n += 1
    return n


def report(n):
    print(f"frames compared with the reference's: {n}")   # (pytest -s: summed up for DESIGN.md's test section)


@pytest.mark.parametrize("name", QUADRIC + CUBIC)
def test_shipped_scenes(pkg, monkeypatch, name):
    """The repository's scenes through the product's loader on one side and through the reference's factories on the other."""
    cubic = name in CUBIC
    w, h = (320, 240) if cubic else (96, 72)   # degree 3 at the size the 0.04 % bound was stated for
    cams = [None, pkg.camera_matrix(*MOVED)]
    want = R.RefScene.from_yaml(scene_path(name)).render(cams, w, h, 4)
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h).set_max_reflections(4)
    n = sum(hold_to_reference(pkg, sc, ref, cam, cubic, name) for cam, ref in zip(cams, want))
    if name == "20spheres":   # the lean instantiation on every frame (small frames otherwise leave it after the first)
        monkeypatch.setenv("MI355RT_LEAN", "always")
        for cam, ref in zip(cams, want):
            assert np.array_equal(frame(pkg, sc, cam), ref), "lean instantiation"
            n += 1
    report(n)


def _keys():
    from test_counters_fuzz_gpu import RANDOM, SHEAR
    from test_ssaa_adaptive_fuzz_gpu import EDGE
    keys = [("fuzz_spheres", s) for s in range(6)] + [("fuzz_parity", s) for s in [158, 534] + list(range(2000, 2006))]
    keys += [("fuzz_cubic", s) for s in range(3)] + [("random_cubic", s) for s in range(3)] + [("mixed", s, 96, 72) for s in range(6)]
    keys += RANDOM[::3] + SHEAR[:2] + [("edge", n) for n in EDGE]
    return keys


@pytest.mark.parametrize("key", _keys(), ids=lambda k: "-".join(str(v) for v in k[:3]))
def test_random_and_edge_scenes(pkg, oracle, monkeypatch, key):
    """A sample of the scenes of tests/test_oracle_vs_reference.py, from the same builders."""
    osc, cam = built_scene(pkg, oracle, key)
    want = R.render(osc, [cam])[0]
    sc = desc_of(pkg, osc)
    n = hold_to_reference(pkg, sc, want, cam, is_cubic(osc), key)
    if lean_eligible(osc):
        monkeypatch.setenv("MI355RT_LEAN", "always")
        assert np.array_equal(frame(pkg, sc, cam), want, equal_nan=True), (key, "lean instantiation")
        n += 1
    report(n)


@pytest.mark.parametrize("name", OWN_EDGES)
def test_constructed_edge_scenes(pkg, oracle, name):
    """Lights behind and on the surface, reflection_ratio at and around EPS, coincident objects, an empty scene, hits at EPS and MAX_T."""
    osc = _own_edge_scenes(oracle)[name]
    cams = [None, oracle.camera_matrix((0.4, 0.5, -1.0), 86.0, 3.0)] if osc.width > 1 else [None]
    want = R.render(osc, cams)
    sc = desc_of(pkg, osc)
    report(sum(hold_to_reference(pkg, sc, ref, cam, False, name) for cam, ref in zip(cams, want)))


@pytest.mark.parametrize("name", ["20spheres", "quadratic"])
def test_gbuffer_object_and_depth(pkg, oracle, name):
    """Renderer.gbuffer's object and depth planes against the nearest hit assembled from the REFERENCE's intersect_ray, one call per
    pixel and object (update-cpu.cpp:50-56: t >= EPS, t < MAX_T, t < best_t in object order).  The primary directions are the
    oracle's (the reference has no entry point for them; its frames pin them)."""
    w, h = 48, 36
    cam = np.ascontiguousarray(pkg.camera_matrix(*MOVED), dtype=np.float64).reshape(16)
    osc = oracle.load_scene(scene_path(name)).with_size(w, h)
    cs, d = osc.c_scene(), np.zeros(3)
    dirs = np.empty((h, w, 3))
    for y in range(h):
        for x in range(w):
            oracle.lib().orc_primary_dir(C.byref(cs), cam.ctypes.data_as(C.POINTER(C.c_double)), x, y, d.ctypes.data_as(C.POINTER(C.c_double)))
            dirs[y, x] = d
    coefs = np.asarray(osc.coefs, dtype=np.float64).reshape(-1, 20)
    rows = np.empty((len(coefs), h * w, 26))
    rows[:, :, :20], rows[:, :, 20:23], rows[:, :, 23:26] = coefs[:, None, :], cam[12:15], dirs.reshape(-1, 3)
    t = R.units("intersect_ray", rows.reshape(-1, 26)).reshape(len(coefs), h, w)
    obj, best = np.full((h, w), -1, dtype=np.int32), np.full((h, w), np.inf)
    for k in range(len(coefs)):
        with np.errstate(invalid="ignore"):
            take = (t[k] >= 1e-7) & (t[k] < 1e6) & (t[k] < best)
        obj[take], best[take] = k, t[k][take]
    r = pkg.Renderer(pkg.Scene.load_from_file(scene_path(name)).set_size(w, h), device=0)
    try:
        go, gt, _, _ = r.gbuffer(cam, normal=False)
        go, gt = go.cpu().numpy(), gt.cpu().numpy()
    finally:
        r.cleanup_update()
    assert (obj >= 0).any() and (obj < 0).any()
    assert np.array_equal(go, obj), int((go != obj).sum())
    assert np.array_equal(gt.view(np.uint64), best.view(np.uint64)), int((gt != best).sum())
