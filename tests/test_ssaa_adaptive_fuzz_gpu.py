"""Edge-adaptive supersampling (RT_FLAG_SSAA_ADAPTIVE) on the random and edge scenes that the wavefront and simple kernels are held
to.  The ray-list kernel (rt_adaptive.hip) has its own LDS staging, its own wave-wide shadow culling over 64-object chunks, its own
bounce loop and its own counters, so it meets the same scenes: random sphere fields past one and past several 64-object chunks and
past 64 KiB of LDS, mixed classes whose planes and general quadrics cannot be culled, the fuzzer's scenes, the edge cases, bands,
degree-3 surfaces, the FMA-contracted build and the reference-equivalent work counters.

For degree <= 2 every frame is compared bit for bit with ssaa_adaptive_ref.compose(P, S, k, tau) of the oracle's W x H frame P
and kW x kH frame S; tau < 0 sends every pixel through the ray-list kernel.  Counters are compared with the oracle's counters of
P plus those of the k^2 samples of every refined pixel (and of the halo rows of a band)."""
import ctypes as C
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_parity import mixed_scene, oracle_from, random_cubic_scene, random_scene
from test_ssaa_adaptive_gpu import F32, U8, ada_flags, kflag

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ssaa_adaptive_ref as ada  # noqa: E402
import ssaa_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TAUS = (-1.0, 0.0, 1.0 / 32.0, 0.2)
COUNTED = ("primary_rays", "shadow_rays", "reflect_rays", "tests", "hits")


@functools.lru_cache(maxsize=None)
def _fuzz():
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tests", "tools", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    return fz


def _pkg():
    import __graft_entry__ as graft
    return graft.load_package()


def _oracle():
    import __graft_entry__ as graft
    return graft.load_oracle()


def pose(pkg, i):
    """A few camera poses that look into the random fields from elsewhere; i < 0: the identity."""
    if i < 0:
        return None
    return pkg.camera_matrix((0.7 * i - 1.5, 0.4 * (i % 3), -1.5 * (i % 4)), 90.0 + 4.0 * (i % 5) - 8.0, 2.0 * (i % 3) - 2.0)


# ---- the edge scenes of test_gpu_parity.py / test_lean_path.py, by name (the scenes, not their assertions) --------------------
def _edge_scene(pkg, oracle, name):
    """(scene or rt_scene_desc, oracle scene or None, camera)"""
    S = pkg.surface_make
    if name == "no_objects":
        s = pkg.Scene.new(37, 19, 50.0, 2, (0.3, 0.6, 0.9))
        s.add_light("directional", [0, -1, 0])
        return s, None, None
    if name == "no_lights":
        s = pkg.Scene.new(33, 17, 50.0, 2, (0.3, 0.6, 0.9))
        s.add_object(S("sphere", [0, 0, 10], [3.0]), (1, 1, 1))
        return s, None, None
    if name in ("1x1", "3x1", "1x5"):
        w, h = (int(v) for v in name.split("x"))
        return random_scene(pkg, 5, 6, 3, w=w, h=h), None, None
    if name == "40_lights_71_objects":
        return random_scene(pkg, 21, 70, 40, w=48, h=32, mirrors=True), None, None
    if name == "camera_inside_sphere":
        s = pkg.Scene.new(64, 48, 60.0, 2, (0.1, 0.1, 0.1))
        s.add_object(S("sphere", [0, 0, 0], [50.0]), (0.9, 0.8, 0.7))
        s.add_object(S("sphere", [1, 0, 8], [1.0]), (0.2, 0.9, 0.2), 0.5)
        s.add_light("spherical", [0, 5, 4], (1, 1, 1), 500.0)
        s.add_light("directional", [0.2, -1, 0.3], (1, 1, 1), 1.0)
        return s, None, None
    if name == "light_inside_sphere":
        s = pkg.Scene.new(80, 60, 45.0, 3, (0.0, 0.0, 0.0))
        for c, r in (([0, 0, 10], 2.0), ([2.0, 0, 10], 2.0), ([4.0, 0, 10], 2.0), ([0, 4.0, 10], 2.0), ([0, -4, 12], 2.5), ([8, 1, 14], 3.0)):
            s.add_object(S("sphere", c, [r]), (0.8, 0.8, 0.8), 0.3)
        s.add_light("spherical", [0, 0, 10], (1, 1, 1), 300.0)
        s.add_light("spherical", [3, 6, 2], (1, 0.5, 0.5), 600.0)
        return s, None, None
    if name == "inside_sphere_with_four":
        s = pkg.Scene.new(80, 60, 60.0, 2, (0.2, 0.3, 0.4))
        s.add_object(S("sphere", [0, 0, 0], [50.0]), (0.9, 0.8, 0.7))
        for k in range(4):
            s.add_object(S("sphere", [3 * k - 4.5, 0.5 * k, 12], [1.0 + 0.2 * k]), (0.3, 0.9, 0.5))
        s.add_light("directional", [0.2, -1, 0.3])
        s.add_light("directional", [-1, -0.1, 0.0])
        s.add_light("spherical", [0, 5, 5], (1, 1, 1), 400.0)
        return s, None, None
    if name == "radii_1e-3_to_1e4":
        s = pkg.Scene.new(80, 60, 60.0, 2, (0.2, 0.3, 0.4))
        for k, r in enumerate([1e-3, 1e-2, 0.1, 1.0, 10.0]):
            s.add_object(S("sphere", [2.5 * k - 5, 0, 6 + 30 * r], [r * 20 if r < 1 else r]), (0.8, 0.4, 0.2))
        s.add_object(S("sphere", [0, -1e4 - 3, 0], [1e4]), (0.5, 0.5, 0.5))
        for d in ([0.3, -1, 0.2], [1, -0.02, 0], [0, -1, 0], [0, -1e-9, 1]):
            s.add_light("directional", d)
        return s, None, None
    if name.startswith("offset_"):
        off = float(name[len("offset_"):])
        s = pkg.Scene.new(48, 32, 60.0, 2, (0.2, 0.3, 0.4))
        o = np.array([off, -off, 0.5 * off])
        for k in range(6):
            s.add_object(S("sphere", o + [2.2 * k - 5.5, 0.3 * k, 14], [1.3]), (0.8, 0.4 + 0.1 * k, 0.2))
        s.add_light("directional", [0.3, -1, 0.2])
        s.add_light("directional", [-0.5, -0.2, 1])
        s.add_light("spherical", o + [0, 8, 6], (1, 1, 1), 500.0)
        return s, None, pkg.camera_matrix(tuple(o), 90.0, 0.0)
    if name == "nested_spheres":
        s = pkg.Scene.new(80, 60, 60.0, 2, (0.2, 0.3, 0.4))
        for k in range(8):
            s.add_object(S("sphere", [0.9 * k - 3, 0.2 * (k % 3), 10 + 0.5 * (k % 2)], [1.0 + 0.15 * k]), (0.2 + 0.1 * k, 0.5, 0.9 - 0.1 * k))
        s.add_object(S("sphere", [0, 0, 10], [0.3]), (1, 1, 1))
        for d in ([0.3, -1, 0.2], [-1, -0.3, 0.5], [0.1, 0.1, 1.0], [0, 1, 0]):
            s.add_light("directional", d)
        return s, None, None
    if name == "huge_coordinates":
        rng = np.random.default_rng(3)
        off = np.array([1.0e6, -2.0e6, 3.0e6])
        s = pkg.Scene.new(64, 48, 50.0, 2, (0.1, 0.2, 0.3))
        for i in range(12):
            c = rng.uniform([-8, -5, 8], [8, 5, 30]) + off
            s.add_object(S("sphere", c, [float(rng.uniform(0.5, 2.5))]), rng.uniform(0, 1, 3))
        s.add_light("directional", [0.3, -1.0, 0.4], (1, 1, 1), 1.0)
        s.add_light("spherical", np.array([0.0, 12.0, 5.0]) + off, (1, 1, 1), 800.0)
        cam = np.eye(4).reshape(16).copy()
        cam[12:15] = off
        return s, None, cam
    if name.startswith("quadrics_and_planes"):
        s = pkg.Scene.new(80, 60, 55.0, 3, (0.2, 0.3, 0.4))
        q = np.zeros(20); q[10], q[11], q[12], q[19] = 1.0, 4.0, 0.5, -9.0; q[18] = -6.0
        s.add_object(q, (0.9, 0.3, 0.3))
        q = np.zeros(20); q[10], q[11], q[12], q[19] = -1.0, 1.0, -1.0, 1.0; q[16], q[18] = 0.5, 12.0
        s.add_object(q, (0.3, 0.9, 0.3), 0.4)
        q = np.zeros(20); q[10], q[12], q[17], q[19] = 0.1, 0.1, 1.0, 20.0
        s.add_object(q, (0.8, 0.8, 0.0))
        q = np.zeros(20); q[10], q[11], q[12], q[13], q[14], q[15], q[19] = 1.0, 2.0, 1.5, 0.5, -0.3, 0.2, -30.0; q[18] = -10.0
        s.add_object(q, (0.3, 0.3, 0.9))
        s.add_object(S("plane", [0, -6, 0], [0, 1, 0.05]), (0.5, 0.5, 0.5), 0.3)
        s.add_object(S("sphere", [3, 1, 9], [1.2]), (0.9, 0.9, 0.9))
        s.add_light("directional", [0.4, -1.0, 0.3], (1, 1, 1), 1.2)
        s.add_light("spherical", [-4, 6, 2], (1, 0.8, 0.6), 500.0)
        moved = name.endswith("_moved")
        return s, None, pkg.camera_matrix(pos=(0.5, 0.5, -2.0), yaw_deg=93.0, pitch_deg=2.0) if moved else None
    if name.startswith("two_mirrors_depth_"):
        from test_oracle_units import two_mirror_scene
        osc = two_mirror_scene(oracle, int(name.rsplit("_", 1)[1]))
        d = pkg.desc_from_arrays(osc.width, osc.height, osc.vertical_fov, osc.bg_color, osc.max_reflections, osc.coefs,
                                 osc.reflection, osc.albedo, osc.light_is_spherical, osc.light_p, osc.light_color)
        return d, osc, None
    raise KeyError(name)


EDGE = ["no_objects", "no_lights", "1x1", "3x1", "1x5", "40_lights_71_objects", "camera_inside_sphere", "light_inside_sphere",
        "inside_sphere_with_four", "radii_1e-3_to_1e4", "offset_1e4", "offset_1e6", "offset_3e7", "nested_spheres", "huge_coordinates",
        "quadrics_and_planes", "quadrics_and_planes_moved", "two_mirrors_depth_0", "two_mirrors_depth_1", "two_mirrors_depth_5"]


def build(key):
    """key -> (scene or desc, oracle scene, camera).  Keys: ("random", seed, n, lights, plane, mirrors, w, h, pose),
    ("mixed", seed, w, h), ("fuzz", seed), ("edge", name)."""
    pkg, oracle = _pkg(), _oracle()
    kind = key[0]
    if kind == "random":
        _, seed, n, lights, plane, mirrors, w, h, p = key
        sc, osc, cam = random_scene(pkg, seed, n, lights, w=w, h=h, with_plane=plane, mirrors=mirrors), None, pose(pkg, p)
    elif kind == "mixed":
        _, seed, w, h = key
        sc, osc = mixed_scene(pkg, seed, w, h), None
        cam = pkg.camera_matrix(pos=(0.3 * (seed % 5) - 0.6, 0.2 * (seed % 3), -1.0 * (seed % 4)), yaw_deg=90.0 + (seed % 7) - 3, pitch_deg=(seed % 5) - 2.0)
    elif kind == "fuzz":
        (sc, cam), osc = _fuzz().scene(key[1]), None
    else:
        sc, osc, cam = _edge_scene(pkg, oracle, key[1])
    return sc, (oracle_from(pkg, oracle, sc) if osc is None else osc), cam


@functools.lru_cache(maxsize=None)
def oracle_frame(key, k=1, counters=False):
    """The oracle's frame of scene `key` at k times its size (and its counters)."""
    _, osc, cam = build(key)
    return osc.with_size(k * osc.width, k * osc.height).render(cam=cam, counters=counters, nthreads=8)


def identical(got, want):
    """Bit for bit, except that a NaN channel only has to be NaN on both sides (the device and glibc spell NaN differently)."""
    if got.shape != want.shape:
        return False
    if got.dtype == np.uint8 or want.dtype == np.uint8:
        return got.dtype == want.dtype and np.array_equal(got, want)
    nan = np.isnan(got)
    return np.array_equal(nan, np.isnan(want)) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def mismatch(got, want):
    with np.errstate(invalid="ignore"):
        return int((got != want).any(axis=-1).sum())


def adaptive(pkg, sc, cam, k, tau, fmt=F32, extra=0, **kw):
    """(frame, refined pixels, counters or None) of one adaptive frame."""
    r = pkg.Renderer(sc, device=0, flags=ada_flags(pkg, k, extra), fmt=fmt, ssaa_threshold=tau, **kw)
    try:
        r.update(cam)
        cnt = r.counters() if extra & pkg.RT_FLAG_COUNT else None
        return r.download(), r.refined, cnt
    finally:
        r.cleanup_update()


def plain(pkg, sc, cam, flags=0):
    r = pkg.Renderer(sc, device=0, flags=flags)
    try:
        r.update(cam)
        return r.download()
    finally:
        r.cleanup_update()


def expect(p, s, k, tau, fmt):
    out = ada.compose(p, s, k, tau)
    return ssaa_ref.quantise(out) if fmt == U8 else out


def check_against_oracle(pkg, key, k, fmt=F32, taus=TAUS, extra=0):
    """Every tau: the adaptive frame == compose(P, S, k, tau) bit for bit and Renderer.refined == refine_mask(P, tau).sum()."""
    sc, _, cam = build(key)
    p, s = oracle_frame(key), oracle_frame(key, k)
    for tau in taus:
        got, n, _ = adaptive(pkg, sc, cam, k, tau, fmt, extra)
        want = expect(p, s, k, tau, fmt)
        assert identical(got, want), (key, k, fmt, tau, mismatch(got, want))
        assert n == int(ada.refine_mask(p, tau).sum()), (key, k, tau, n)


# 1. random sphere fields: 3 .. 568 spheres, one to nine lights, with and without mirrors and the floor plane, moved cameras
RANDOM = [  # (seed, spheres, lights, plane, mirrors, w, h, pose, k, fmt)
    (1, 3, 1, True, False, 64, 48, -1, 2, F32),
    (2, 12, 4, True, True, 64, 48, 1, 4, U8),
    (3, 40, 9, False, False, 80, 60, 2, 2, F32),
    (4, 64, 3, False, True, 48, 36, 3, 4, F32),
    (5, 65, 5, False, True, 48, 36, 4, 4, F32),
    (6, 65, 3, True, False, 80, 60, -1, 2, U8),
    (7, 130, 6, True, True, 80, 60, 5, 2, F32),
    (8, 130, 2, False, False, 48, 36, 6, 4, U8),
    (9, 200, 5, False, True, 80, 60, 7, 2, F32),
    (10, 200, 7, True, False, 40, 30, -1, 4, F32),
    (11, 300, 4, True, True, 64, 48, 8, 2, F32),     # 301 objects: 86.7 KB of dynamic LDS on the ray-list launch
    (12, 567, 3, True, False, 24, 16, 9, 2, F32),    # 568 objects: the most rt_create accepts for an adaptive context (160 KiB)
]


@pytest.mark.parametrize("case", RANDOM, ids=[f"seed{c[0]}-n{c[1]}-k{c[8]}" for c in RANDOM])
def test_random_sphere_fields(pkg, case):
    seed, n, lights, plane, mirrors, w, h, p, k, fmt = case
    check_against_oracle(pkg, ("random", 9300 + seed, n, lights, plane, mirrors, w, h, p), k, fmt)


def test_lds_limit_of_an_adaptive_context(pkg):
    """One object past 160 KiB of staged LDS (569 x 288 bytes): rt_create refuses the context instead of launching it."""
    sc = random_scene(pkg, 9313, 568, 2, w=16, h=8)
    for extra in (0, pkg.RT_FLAG_SIMPLE):
        with pytest.raises(pkg.RtError, match="adaptive supersampling stages 163872 bytes"):
            pkg.Renderer(sc, device=0, flags=ada_flags(pkg, 2, extra))


# 2. mixed classes (planes and general quadrics: culling entries that cannot be culled) and the fuzzer's scenes
@pytest.mark.parametrize("seed", range(8))
def test_mixed_class_scenes(pkg, seed):
    check_against_oracle(pkg, ("mixed", seed, 80, 60), 2 if seed % 2 else 4, U8 if seed % 4 == 1 else F32)


@pytest.mark.parametrize("seed", [158, 534, 2000, 2007, 2009, 2018, 2021, 2023, 2028, 2041, 2043, 2045, 2047, 2048])
def test_fuzz_scenes(pkg, seed):
    check_against_oracle(pkg, ("fuzz", seed), 4 if seed % 3 == 0 else 2)


# 3. the edge scenes
@pytest.mark.parametrize("name", EDGE)
def test_edge_scenes(pkg, name):
    k = 2 if name in ("40_lights_71_objects", "huge_coordinates") else 4
    check_against_oracle(pkg, ("edge", name), k, U8 if name.startswith("offset") else F32)
    if k == 4:
        check_against_oracle(pkg, ("edge", name), 2, F32, taus=(-1.0, 1.0 / 32.0))


# 4. bands on random scenes: the halo rows (K = 1) away from reflection_test, heights that are not a multiple of world x band
@pytest.mark.parametrize("band", [1, 3, 16])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_bands_on_random_scenes(pkg, world, band):
    key = ("random", 9400 + world * band, 30, 5, True, True, 72, 67, world % 5)
    i = [1, 3, 16].index(band) + world
    k, fmt = (2, 4)[i % 2], (F32, U8)[(i // 2) % 2]
    sc, _, cam = build(key)
    h = sc.desc().height
    p, s = oracle_frame(key), oracle_frame(key, k)
    for tau in (0.0, 1.0 / 32.0):
        want = expect(p, s, k, tau, fmt)
        single, n, _ = adaptive(pkg, sc, cam, k, tau, fmt)
        assert identical(single, want), (tau, mismatch(single, want))
        mask = ada.refine_mask(p, tau)
        seen = np.zeros(h, dtype=bool)
        for rank in range(world):
            rows = pkg.band_rows_of_rank(h, band, world, rank)
            got, n, _ = adaptive(pkg, sc, cam, k, tau, fmt, rank=rank, world=world, band_rows=band)
            assert got.shape[0] == len(rows)
            assert identical(got, single[rows]) and identical(got, want[rows]), (rank, tau, mismatch(got, want[rows]))
            assert n == int(mask[rows].sum()), (rank, tau)
            seen[rows] = True
        assert seen.all()


# 5. degree 3: the library's own renders are the reference (device cbrt / acos / cos)
@pytest.mark.parametrize("seed", range(6))
def test_random_cubic_scenes(pkg, seed):
    w, h, k = 96, 72, 2 if seed % 2 else 4
    sc, cam = random_cubic_scene(pkg, seed, w, h)
    got, n, _ = adaptive(pkg, sc, cam, k, -1.0)
    assert identical(got, plain(pkg, sc, cam, kflag(pkg, k))) and n == w * h
    p = plain(pkg, sc, cam)
    s = plain(pkg, random_cubic_scene(pkg, seed, k * w, k * h)[0], cam)
    got, n, _ = adaptive(pkg, sc, cam, k, 1.0 / 32.0)
    want = ada.compose(p, s, k, 1.0 / 32.0)
    assert identical(got, want), mismatch(got, want)
    assert n == int(ada.refine_mask(p, 1.0 / 32.0).sum())


# 6. the FMA-contracted build: every pixel refined equals the full supersampled frame of the same build
@pytest.mark.parametrize("seed,n,k", [(1, 20, 2), (2, 70, 4), (3, 130, 2)])
def test_fast_variant_on_random_scenes(pkg, seed, n, k):
    sc, _, cam = build(("random", 9500 + seed, n, 4, seed != 3, seed != 1, 80, 60, seed))
    got, _, _ = adaptive(pkg, sc, cam, k, -1.0, extra=pkg.RT_FLAG_FAST)
    assert identical(got, plain(pkg, sc, cam, kflag(pkg, k) | pkg.RT_FLAG_FAST)), (seed, n, k)


# 7. counters: reference-equivalent rays, tests and hits -- P's, plus the k^2 samples of every refined pixel, plus the halo rows
def _sum(*ds):
    return {c: sum(int(d[c]) for d in ds) for c in COUNTED}


def _oracle_counts(d):
    return dict(d, hits=d["normals"])


def sample_counts(key, k, mask):
    """The oracle's counters of the k x k samples (rays of the kW x kH frame) of the pixels where `mask` is set."""
    oracle = _oracle()
    _, osc, cam = build(key)
    big = osc.with_size(k * osc.width, k * osc.height).c_scene()
    cm = np.ascontiguousarray(oracle.IDENTITY if cam is None else cam, dtype=np.float64)
    cnt, rgb, L = oracle.OrcCounters(), (C.c_float * 3)(), oracle.lib()
    for y, x in zip(*np.nonzero(mask)):
        for j in range(k):
            for i in range(k):
                L.orc_render_pixel(C.byref(big), cm.ctypes.data_as(C.POINTER(C.c_double)), int(k * x + i), int(k * y + j), rgb, C.byref(cnt))
    return _oracle_counts(cnt.as_dict())


def rows_counts(key, rows):
    """The oracle's counters of the W x H frame's rows `rows` (repeats count again)."""
    _, osc, cam = build(key)
    if len(rows) == 0:
        return {c: 0 for c in COUNTED}
    return _oracle_counts(osc.render(cam=cam, rows=np.asarray(rows, dtype=np.uint32), counters=True, nthreads=8)[1])


COUNT_KEY = ("random", 9600, 70, 5, True, True, 48, 36, 3)   # 71 objects (two chunks, one plane that is never culled), mirrors


@pytest.mark.parametrize("nocull", [False, True], ids=["cull", "nocull"])
@pytest.mark.parametrize("kernel", ["wavefront", "simple"])
def test_counters_against_the_oracle(pkg, kernel, nocull):
    extra = pkg.RT_FLAG_COUNT | (pkg.RT_FLAG_SIMPLE if kernel == "simple" else 0) | (pkg.RT_FLAG_NOCULL if nocull else 0)
    sc, _, cam = build(COUNT_KEY)
    p, pc = oracle_frame(COUNT_KEY, 1, True)
    for k in (2, 4):
        for tau in (-1.0, 1.0 / 32.0):
            _, n, got = adaptive(pkg, sc, cam, k, tau, extra=extra)
            mask = ada.refine_mask(p, tau)
            assert n == int(mask.sum())
            samples = _oracle_counts(oracle_frame(COUNT_KEY, k, True)[1]) if tau < 0 else sample_counts(COUNT_KEY, k, mask)
            want = _sum(_oracle_counts(pc), samples)
            assert {c: got[c] for c in COUNTED} == want, (k, tau, {c: (got[c], want[c]) for c in COUNTED if got[c] != want[c]})


def test_counters_of_a_banded_frame(pkg):
    world, band, k, tau = 3, 4, 2, 1.0 / 32.0
    sc, _, cam = build(COUNT_KEY)
    h = sc.desc().height
    mask = ada.refine_mask(oracle_frame(COUNT_KEY), tau)
    for rank in range(world):
        rows = pkg.band_rows_of_rank(h, band, world, rank)
        halo = []
        for b0 in range(0, len(rows), band):   # the rows just below and just above each of the rank's bands
            g0, g1 = int(rows[b0]), int(rows[min(b0 + band, len(rows)) - 1])
            halo += [g for g in (g0 - 1, g1 + 1) if 0 <= g < h]
        lm = np.zeros_like(mask)
        lm[rows] = mask[rows]
        _, n, got = adaptive(pkg, sc, cam, k, tau, extra=pkg.RT_FLAG_COUNT, rank=rank, world=world, band_rows=band)
        assert n == int(lm.sum()), rank
        want = _sum(rows_counts(COUNT_KEY, rows), rows_counts(COUNT_KEY, halo), sample_counts(COUNT_KEY, k, lm))
        assert {c: got[c] for c in COUNTED} == want, (rank, {c: (got[c], want[c]) for c in COUNTED if got[c] != want[c]})
