"""rt_trace_paths / rt_primary_rays / rt_pick_paths without a GPU: the reference composer (tests/tools/paths_ref.py) against
shade_ref's segment counts and, recomposed into colours, against the oracle's own frames; the boundary cases of the definition with
hand-stated values; that the cases the GPU tests use are not vacuous; the declarations and the build's register report
(include/mi355rt.h "Ray queries")."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import paths_ref  # noqa: E402
import rays_ref  # noqa: E402
import raw_desc_scenes as R  # noqa: E402
import shade_ref  # noqa: E402
from paths_ref import CAP, ESCAPED, MISS, SURFACE  # noqa: E402
from test_gpu_parity import oracle_from, random_scene  # noqa: E402
from test_shade_host import FAR_RAY, RATIO_ABOVE, RATIO_BELOW, facing_mirrors, far_plane, ratio_scene, scene_of  # noqa: E402

W, H = 40, 30
F = np.float32
F1 = np.float32(1.0)
DEPTH_CAM = ((0.5, 1.0, -2.0), 88.0, -6.0)   # the camera of tests/test_shade_gpu.py::test_reflection_depths
MOVED = ((0.4, 0.3, -1.5), 84.0, -3.0)


def depth_scene(pkg, max_refl, seed=3100, w=W, h=H):
    return random_scene(pkg, seed, 9, 2, w=w, h=h, with_plane=True, mirrors=True).set_max_reflections(max_refl)


def cone_scene(oracle, mirror):
    """The cone x^2 + y^2 - z^2 = 0 (its gradient vanishes at the apex) and a sphere behind it."""
    q = np.zeros(20)
    q[10], q[11], q[12] = 1.0, 1.0, -1.0
    return scene_of(oracle, [(list(q), (0.8, 0.7, 0.6), 0.5 if mirror else 0.0), (R.sphere((0.5, 0.2, 6), 1.5), (0.2, 0.9, 0.3), 0.0)])


CONE_RAYS = ([[0.0, 0.0, -2.0], [0.3, 0.1, -2.0], [0.0, 0.0, -2.0]], [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.5]])
MIRROR_RAYS = ([[0.0, 0.0, 0.0], [0.1, -0.2, 1.0]], [[0.0, 0.0, 1.0], [0.0, 0.0, -3.0]])


def flat_copy(osc):
    """The scene without mirrors: shade_ref.shade of a ray is then get_color_and_object's colour of that one segment."""
    flat = R.copy_scene(osc)
    for ob in flat.objects:
        ob.reflection_ratio = 0.0
    return flat


def recomposed(osc, rays):
    """The reference's colours from the composer's paths: shade_ref's colour of every segment's ray, blended with the composer's ratio
    sequence as UPDATE_COLOR does, the background where `end` says so."""
    m, n = osc.max_reflections + 1, len(rays)
    seg_rays, ratios = np.zeros((m, n), dtype=rays_ref.RAY_DTYPE), []
    seg, last, ends = paths_ref.paths(osc, rays, ratios=ratios, seg_rays=seg_rays)
    flat = flat_copy(osc)
    traced = ends["segments"] + np.isin(ends["end"], (MISS, ESCAPED))
    col = np.zeros((m, n, 3), dtype=np.float32)
    for k in range(m):
        idx = np.flatnonzero(traced > k)
        if len(idx):
            col[k, idx] = shade_ref.shade(flat, seg_rays[k, idx])[:, :3]   # (a segment that leaves the scene: the background)
    bg = [F(v) for v in np.asarray(osc.bg_color, dtype=np.float32)]
    out = np.zeros((n, 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            if ends["end"][i] == MISS:
                out[i] = bg
                continue
            res = [col[0, i, c] for c in range(3)]
            for k in range(1, int(traced[i])):
                r = ratios[i][k - 1]
                res = [(F1 - r) * res[c] + r * col[k, i, c] for c in range(3)]
            if ends["end"][i] == CAP:
                r = ratios[i][-1]
                res = [(F1 - r) * res[c] + r * bg[c] for c in range(3)]
            out[i] = res
    return out, (seg, last, ends)


def check_against_shade_and_frame(osc, cam=None):
    rays = rays_ref.primary_rays(osc, cam)
    got, (seg, last, ends) = recomposed(osc, rays)
    want = osc.render(cam=cam)
    assert shade_ref.same_bits(got.reshape(osc.height, osc.width, 3), want), shade_ref.describe_difference(got, want.reshape(-1, 3))   # (b)
    nseg = np.zeros(len(rays), dtype=np.int64)
    shade_ref.shade(osc, rays, segments=nseg)
    assert np.array_equal(ends["segments"] + np.isin(ends["end"], (MISS, ESCAPED)), nseg)   # (a)
    assert rays_ref.same_records(seg[0], rays_ref.closest(osc, rays))
    return seg, last, ends


# ---- (a), (b): the composer against shade_ref and the oracle's frames ---------------------------------------------------------------
@pytest.mark.parametrize("moved", [False, True])
def test_composer_recomposes_the_oracles_frame_on_the_shipped_mirror_scene(oracle, moved):
    osc = oracle.load_scene(scene_path("reflection_test")).with_size(W, H)
    seg, last, ends = check_against_shade_and_frame(osc, oracle.camera_matrix(*MOVED) if moved else None)
    assert ends["segments"].max() > 1


@pytest.mark.parametrize("max_refl", [0, 1, 5])
def test_composer_recomposes_the_oracles_frame_on_random_mirror_scenes(pkg, oracle, max_refl):
    osc = oracle_from(pkg, oracle, depth_scene(pkg, max_refl))
    seg, last, ends = check_against_shade_and_frame(osc, oracle.camera_matrix(*DEPTH_CAM))
    assert ends["segments"].max() == max_refl + 1 if max_refl < 5 else ends["segments"].max() > 2


# ---- (c): cases stated by hand ------------------------------------------------------------------------------------------------------
def one(osc, rays, **kw):
    seg, last, ends = paths_ref.paths(osc, rays, **kw)
    return seg, last, ends


def test_reflection_ratio_at_eps_and_nan(oracle):
    rays = rays_ref.make_rays([[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]])
    seg, last, ends = one(ratio_scene(oracle, RATIO_ABOVE), rays)
    assert ends[0].tolist() == (1, ESCAPED, RATIO_ABOVE, 0) and last["t"][0] == 5.0 and seg.shape == (4, 1) and np.all(seg["object"][1:] == -1)
    seg, last, ends = one(ratio_scene(oracle, RATIO_BELOW), rays)
    assert ends[0].tolist() == (1, SURFACE, 1.0, 0)
    seg, last, ends = one(ratio_scene(oracle, float("nan")), rays)
    assert ends[0].tolist() == (1, SURFACE, 1.0, 0)   # a NaN ratio is no mirror


def test_facing_mirrors_end_at_the_cap(oracle):
    rays = rays_ref.make_rays(*MIRROR_RAYS)
    for max_refl, value in ((0, 0.5), (2, 0.125), (5, 0.015625)):
        seg, last, ends = one(facing_mirrors(oracle, max_refl), rays)
        assert np.all(ends["segments"] == max_refl + 1) and np.all(ends["end"] == CAP) and np.all(ends["ratio"] == F(value))
        assert seg["object"][:, 0].tolist() == [k % 2 for k in range(max_refl + 1)] and np.all(last["object"] == ends["object"])
        assert rays_ref.same_records(last, seg[max_refl])
        # the second ray's direction has length 3: t is in units of |d_k|, and reflect_ray keeps the length
        assert seg["t"][0, 1] == 2.0 and np.all(np.abs(seg["t"][1:, 1] * 3.0 - 9.99) < 1e-9)


def test_hit_point_beyond_the_proven_range(oracle):
    rays = rays_ref.make_rays(*FAR_RAY)
    seg, last, ends = one(far_plane(oracle, False), rays)
    assert ends[0].tolist() == (1, SURFACE, 1.0, 1) and last["point"][0, 2] > 1e100
    seg, last, ends = one(far_plane(oracle, True), rays)
    assert ends[0].tolist() == (1, ESCAPED, 0.5, 1)   # every test of the derived ray is NaN in the reference: the bounce finds nothing


def test_hit_where_the_gradient_vanishes(oracle):
    rays = rays_ref.make_rays(*CONE_RAYS)
    seg, last, ends = one(cone_scene(oracle, False), rays)
    assert np.isnan(seg["normal"][0, 0]).all() and seg["point"][0, 0].tolist() == [0.0, 0.0, 0.0] and ends[0].tolist() == (1, SURFACE, 1.0, 0)
    seg, last, ends = one(cone_scene(oracle, True), rays)
    assert ends[0].tolist() == (1, ESCAPED, 0.5, 0)   # the bounce from the apex has a NaN origin and direction: nothing is hit
    assert not np.isnan(seg["normal"][0, 1]).any() and ends["segments"][1] >= 1


# ---- (d): the cases the GPU tests use are not vacuous -----------------------------------------------------------------------------------
def gpu_cases(pkg, oracle):
    """name -> (oracle scene, rays, the `end` values the case must show, whether a path of max_reflections + 1 segments must occur): the
    scenes, cameras and rays of tests/test_paths_gpu.py that claim to cover an ending.  (A scene without mirrors can only show MISS and
    SURFACE, so the four values are asked of the cases together and of every case what it claims.)"""
    cases = {}
    for moved in (False, True):
        osc = oracle.load_scene(scene_path("reflection_test")).with_size(W, H)
        cases[f"reflection_test moved={moved}"] = (osc, rays_ref.primary_rays(osc, oracle.camera_matrix(*MOVED) if moved else None), {MISS, SURFACE, ESCAPED}, False)
    for max_refl in (0, 1, 5):
        osc = oracle_from(pkg, oracle, depth_scene(pkg, max_refl))
        cases[f"depth {max_refl}"] = (osc, rays_ref.primary_rays(osc, oracle.camera_matrix(*DEPTH_CAM)), {MISS, SURFACE} | ({ESCAPED} if max_refl else set()) | ({CAP} if max_refl < 5 else set()), max_refl < 5)
    for max_refl in (0, 2, 5):
        cases[f"facing mirrors {max_refl}"] = (facing_mirrors(oracle, max_refl), rays_ref.make_rays(*MIRROR_RAYS), {CAP}, True)
    cases["ratio above"] = (ratio_scene(oracle, RATIO_ABOVE), rays_ref.make_rays(*MIRROR_RAYS)[:1], {ESCAPED}, False)
    cases["ratio below"] = (ratio_scene(oracle, RATIO_BELOW), rays_ref.make_rays(*MIRROR_RAYS)[:1], {SURFACE}, False)
    return cases


def test_the_gpu_cases_are_not_vacuous(pkg, oracle):
    seen = set()
    for name, (osc, rays, claims, full) in gpu_cases(pkg, oracle).items():
        seg, last, ends = paths_ref.paths(osc, rays)
        have = set(int(e) for e in np.unique(ends["end"]))
        assert claims <= have, (name, have)
        assert not full or (ends["segments"] == osc.max_reflections + 1).any(), name
        seen |= have
    assert seen == {MISS, SURFACE, ESCAPED, CAP}


# ---- (e): declarations, symbols, refusals before a device, registers ---------------------------------------------------------------------
def test_declarations(pkg):
    text = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "int rt_trace_paths(rt_ctx *ctx, const rt_ray *dev_rays, uint32_t n, uint32_t max_segments, rt_hit *dev_segments , rt_hit *dev_last , rt_path_end *dev_ends , void *stream, float *ms);" in flat
    assert "int rt_trace_paths_host(rt_ctx *ctx, const rt_ray *rays, uint32_t n, uint32_t max_segments, rt_hit *segments_out, rt_hit *last_out , rt_path_end *ends_out, void *stream);" in flat
    assert "int rt_primary_rays(rt_ctx *ctx, const double cam[16], const uint32_t rect[4] , rt_ray *dev_rays , void *stream, float *ms);" in flat
    assert "int rt_pick_paths(rt_ctx *ctx, const double cam[16], const uint32_t *xy, uint32_t n, uint32_t max_segments, rt_hit *segments_host , rt_path_end *ends_host, void *stream);" in flat
    for name, value in (("RT_PATH_MISS", "0u"), ("RT_PATH_SURFACE", "1u"), ("RT_PATH_ESCAPED", "2u"), ("RT_PATH_CAP", "3u"), ("RT_PATH_MAX_SEGMENTS", "64u"), ("RT_ABI_VERSION", "3")):
        assert re.search(rf"#define {name} {value}\b", text), name
    assert C.sizeof(pkg.PathEnd) == 16 and pkg.PATH_END_DTYPE.itemsize == 16 and paths_ref.END_DTYPE == pkg.PATH_END_DTYPE
    assert (pkg.RT_PATH_MISS, pkg.RT_PATH_SURFACE, pkg.RT_PATH_ESCAPED, pkg.RT_PATH_CAP, pkg.RT_PATH_MAX_SEGMENTS) == (MISS, SURFACE, ESCAPED, CAP, paths_ref.MAX_SEGMENTS)


def test_symbols_and_refusals_before_a_device(pkg):
    """Fails without the feature: the library does not export rt_trace_paths."""
    lib = pkg.lib()
    for name in ("rt_trace_paths", "rt_trace_paths_host", "rt_primary_rays", "rt_pick_paths"):
        assert hasattr(lib, name) and name in pkg.ABI_SYMBOLS
    assert hasattr(C.CDLL(pkg.UPDATE_LIB_PATH), "mi355rt_update_pick_path")
    for m in ("paths", "paths_into", "primary_rays", "primary_rays_into", "pick_paths"):
        assert callable(getattr(pkg.Renderer, m))

    def refused(rc, word, who):
        assert rc == -1 and word in lib.rt_last_error() and who in lib.rt_last_error(), lib.rt_last_error()
    ends = np.zeros(4, dtype=pkg.PATH_END_DTYPE)
    rays = np.zeros(4, dtype=pkg.RAY_DTYPE)
    rp, ep = rays.ctypes.data_as(C.POINTER(pkg.Ray)), ends.ctypes.data_as(C.POINTER(pkg.PathEnd))
    refused(lib.rt_trace_paths(None, rays.ctypes.data, 4, 0, None, None, ends.ctypes.data, None, None), b"null", b"rt_trace_paths")
    refused(lib.rt_trace_paths_host(None, rp, 4, 0, None, None, ep, None), b"null", b"rt_trace_paths_host")
    refused(lib.rt_primary_rays(None, None, None, None, None, None), b"null", b"rt_primary_rays")
    refused(lib.rt_pick_paths(None, None, None, 1, 0, None, ep, None), b"null", b"rt_pick_paths")
    hit = pkg.Hit()
    refused(C.CDLL(pkg.UPDATE_LIB_PATH).mi355rt_update_pick_path(0, 0, C.byref(hit), 1, ep), b"update", b"mi355rt_update_pick_path")


def test_no_spill_in_the_new_kernels(pkg):
    text = open(os.path.join(os.path.dirname(pkg.UPDATE_LIB_PATH), "build", "spills.txt")).read()
    lines = [l for l in text.splitlines() if "path_query_kernel" in l]
    assert len(lines) == 8, lines   # <HAS_GQ, HAS_CUBIC> x strict / fast
    lines += [l for l in text.splitlines() if "primary_rays_kernel" in l]
    assert len(lines) == 10, lines
    for l in lines:
        assert re.search(r"VGPR spills\s+0\s+scratch 0\b", l), l
