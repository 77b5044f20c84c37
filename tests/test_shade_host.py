"""rt_shade_rays without a GPU: the reference composer (tests/tools/shade_ref.py) against the oracle's own frames, the boundary cases of
the definition with hand-stated values, the declarations and the build's register report (include/mi355rt.h "Ray queries", DESIGN.md
section 16)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import rays_ref  # noqa: E402
import raw_desc_scenes as R  # noqa: E402
import shade_ref  # noqa: E402
from test_gpu_parity import oracle_from, random_scene  # noqa: E402

QUADRIC = ["quadratic", "20spheres", "reflection_test"]   # the shipped scenes of degree <= 2 (reflection_test holds the mirrors)
W, H = 48, 36
PI_F = np.float32(3.14159274101257324219)
F = np.float32


def frame_equals_composer(osc, cam=None):
    want = osc.render(cam=cam)
    seg = np.zeros(W * H, dtype=np.int64)
    got, rec = shade_ref.shade(osc, rays_ref.primary_rays(osc, cam), hits=True, segments=seg)
    assert np.all(got[:, 3].view(np.uint32) == np.float32(1.0).view(np.uint32))
    assert shade_ref.same_bits(got[:, :3].reshape(H, W, 3), want), shade_ref.describe_difference(got[:, :3], want.reshape(-1, 3))
    return got, rec, seg


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("name", QUADRIC)
def test_composer_is_the_oracles_frame_on_shipped_scenes(oracle, name, moved):
    osc = oracle.load_scene(scene_path(name)).with_size(W, H)
    cam = oracle.camera_matrix((0.4, 0.3, -1.5), 84.0, -3.0) if moved else None
    _, rec, seg = frame_equals_composer(osc, cam)
    assert (rec["object"] >= 0).any() and (rec["object"] < 0).any()
    if name == "reflection_test":
        assert seg.max() > 1   # mirrors were followed


@pytest.mark.parametrize("max_refl", [0, 1, 5])
@pytest.mark.parametrize("seed", [0, 1])
def test_composer_is_the_oracles_frame_on_random_scenes(pkg, oracle, seed, max_refl):
    sc = random_scene(pkg, 3100 + seed, 9 + 4 * seed, 2 + seed, w=W, h=H, with_plane=True, mirrors=True).set_max_reflections(max_refl)
    osc = oracle_from(pkg, oracle, sc)
    assert osc.max_reflections == max_refl and (osc.reflection > 0).any()
    _, rec, seg = frame_equals_composer(osc)
    assert (rec["object"] >= 0).any() and seg.max() == min(max_refl, int(seg.max() - 1)) + 1 and (max_refl == 0 or seg.max() > 1)


def test_composer_is_the_oracles_frame_without_lights(pkg, oracle):
    osc = oracle_from(pkg, oracle, random_scene(pkg, 3200, 10, 0, w=W, h=H, with_plane=False, mirrors=False))
    got, rec, _ = frame_equals_composer(osc)
    hit = rec["object"] >= 0
    assert hit.any() and (~hit).any() and not got[hit, :3].any()   # hits are black, not the background
    assert np.array_equal(got[~hit, :3], np.broadcast_to(osc.bg_color, ((~hit).sum(), 3)))


# ---- boundary cases, each with its value stated by hand ---------------------------------------------------------------------------
def scene_of(oracle, objects, lights=(), max_refl=3, bg=(0.5, 0.25, 1.0)):
    osc = oracle.Scene(8, 8, 50.0, max_refl, bg)
    for coefs, albedo, refl in objects:
        osc.add_object(coefs, albedo, refl)
    osc.lights += list(lights)
    return osc


RATIO_ABOVE = np.float32(1e-7)                               # 1.00000001168e-7 as a double: > EPS
RATIO_BELOW = np.nextafter(np.float32(1e-7), np.float32(0))  # 9.9999994e-8: not > EPS


def ratio_scene(oracle, ratio):
    """An unlit mirror plane z = 5 facing the origin: the hit is black; where the ratio counts, the bounce leaves the scene."""
    return scene_of(oracle, [(R.plane((0, 0, 5), (0, 0, -1)), (1, 1, 1), float(ratio))])


def test_reflection_ratio_at_eps(oracle):
    assert float(RATIO_ABOVE) > 1e-7 and not float(RATIO_BELOW) > 1e-7
    rays = rays_ref.make_rays([[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]])
    seg = np.zeros(1, dtype=np.int64)
    above = shade_ref.shade(ratio_scene(oracle, RATIO_ABOVE), rays, segments=seg)
    # res = (1 - r) * 0 + r * bg: the background scaled by the ratio
    assert seg[0] == 2 and above[0].tolist() == [RATIO_ABOVE * F(0.5), RATIO_ABOVE * F(0.25), RATIO_ABOVE * F(1.0), 1.0] and above[0, 2] > 0
    below = shade_ref.shade(ratio_scene(oracle, RATIO_BELOW), rays, segments=seg)
    assert seg[0] == 1 and below[0].tolist() == [0.0, 0.0, 0.0, 1.0]


def facing_mirrors(oracle, max_refl):
    return scene_of(oracle, [(R.plane((0, 0, 5), (0, 0, -1)), (1, 1, 1), 0.5), (R.plane((0, 0, -5), (0, 0, 1)), (1, 1, 1), 0.5)], max_refl=max_refl, bg=(1, 1, 1))


def test_facing_mirrors_reach_the_cap(oracle):
    """Unlit mirrors of ratio 0.5 at z = +-5: every segment hits black, so res stays 0 until the cap blends the background (1, 1, 1) with
    cur_ratio = 0.5 ** (max_reflections + 1)."""
    rays = rays_ref.make_rays([[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]])
    for max_refl, want in ((0, 0.5), (2, 0.125), (5, 0.015625)):
        seg = np.zeros(1, dtype=np.int64)
        got = shade_ref.shade(facing_mirrors(oracle, max_refl), rays, segments=seg)
        assert seg[0] == max_refl + 1 and got[0].tolist() == [want, want, want, 1.0]


def far_plane(oracle, mirror):
    """A unit sphere at (3, 0, 5), the plane z = 1e104 facing the origin and a directional light from -z."""
    return scene_of(oracle, [(R.sphere((3, 0, 5), 1.0), (0.9, 0.1, 0.1), 0.0), (R.plane((0, 0, 1e104), (0, 0, -1)), (0.5, 0.5, 0.5), 0.5 if mirror else 0.0)],
                    [R.stored_light(0, (0, 0, -1), (2.0, 2.0, 2.0))], max_refl=5)


FAR_RAY = ([[0.0, 0.0, 0.0]], [[0.0, 0.0, 1e99]])
FAR_LIT = F(0.5) / PI_F * F(2.0) * F(1.0)   # ((albedo / pi) * colour) * max(0, n . l), n . l = 1


def test_hit_point_beyond_the_proven_range(oracle):
    osc = far_plane(oracle, False)
    rays = rays_ref.make_rays(*FAR_RAY)
    seg = np.zeros(1, dtype=np.int64)
    got, rec = shade_ref.shade(osc, rays, hits=True, segments=seg)
    assert rec["object"][0] == 1 and rec["point"][0, 2] > 1e100 and abs(rec["t"][0] - 1e5) < 1e-6 and rec["normal"][0].tolist() == [0.0, 0.0, -1.0]
    # every test of the derived rays is NaN in the reference (0 * inf in the 20-term sums): nothing blocks, nothing is hit
    dp = C.POINTER(C.c_double)
    so, sd = np.array([0.0, 0.0, 1e104]), np.array([0.0, 0.0, -1.0])
    for c in osc.coefs:
        c = np.ascontiguousarray(c)
        assert np.isnan(oracle.lib().orc_intersect_ray(c.ctypes.data_as(dp), so.ctypes.data_as(dp), sd.ctypes.data_as(dp)))
    assert seg[0] == 1 and got[0].tolist() == [FAR_LIT, FAR_LIT, FAR_LIT, 1.0] and 0.31 < FAR_LIT < 0.32   # the hit is lit
    got = shade_ref.shade(far_plane(oracle, True), rays, segments=seg)
    want = [(F(1.0) - F(0.5)) * FAR_LIT + F(0.5) * F(b) for b in (0.5, 0.25, 1.0)]   # the bounce finds nothing: the background
    assert seg[0] == 2 and got[0].tolist() == want + [1.0]


# ---- declarations, symbols, registers ---------------------------------------------------------------------------------------------
def test_declarations(pkg):
    text = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"int rt_shade_rays\(rt_ctx \*\w+, const rt_ray \*\w+, uint32_t \w+, float \*\w+, rt_hit \*\w+(?: /\*.*?\*/)?, void \*\w+, float \*\w+\);", text)
    assert re.search(r"int rt_shade_rays_host\(rt_ctx \*\w+, const rt_ray \*\w+, uint32_t \w+, float \*\w+, void \*\w+\);", text)
    assert "#define RT_ABI_VERSION 3" in text


def test_symbols_and_null_refusals(pkg):
    """Fails without the feature: the library does not export rt_shade_rays."""
    lib = pkg.lib()
    for name in ("rt_shade_rays", "rt_shade_rays_host"):
        assert hasattr(lib, name) and name in pkg.ABI_SYMBOLS
    assert hasattr(C.CDLL(pkg.UPDATE_LIB_PATH), "mi355rt_update_shade")
    for m in ("shade", "shade_into"):
        assert callable(getattr(pkg.Renderer, m))
    # refusals that need no device: NULL arguments
    assert lib.rt_shade_rays(None, None, 1, None, None, None, None) == -1 and b"null" in lib.rt_last_error() and b"rt_shade_rays" in lib.rt_last_error()
    assert lib.rt_shade_rays_host(None, None, 1, None, None) == -1 and b"null" in lib.rt_last_error()


def test_no_spill_in_the_new_kernels(pkg):
    text = open(os.path.join(os.path.dirname(pkg.UPDATE_LIB_PATH), "build", "spills.txt")).read()
    lines = [l for l in text.splitlines() if "shade_rays_kernel" in l]
    assert len(lines) == 8, lines   # <HAS_GQ, HAS_CUBIC> x strict / fast
    for l in lines:
        assert re.search(r"VGPR spills\s+0\s+scratch 0\b", l), l
