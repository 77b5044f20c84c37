"""Ray queries without a GPU: the reference composer (tests/tools/rays_ref.py) against the G-buffer composer and against the oracle's
own frames, the two boundary cases of the definitions, and the declarations (include/mi355rt.h "Ray queries")."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gbuffer_ref  # noqa: E402
import rays_ref  # noqa: E402

QUADRIC = ["quadratic", "20spheres", "reflection_test"]   # the shipped scenes of degree <= 2


@pytest.mark.parametrize("name", QUADRIC)
def test_closest_on_primary_rays_is_the_gbuffer_composer(oracle, name):
    osc = oracle.load_scene(scene_path(name)).with_size(48, 36)
    cam = oracle.camera_matrix((0.4, 0.3, -1.5), 84.0, -3.0) if name != "quadratic" else None
    ref = gbuffer_ref.compose(osc, cam)
    rays = rays_ref.primary_rays(osc, cam)
    assert np.array_equal(rays["d"].view(np.uint64), ref["dir"].reshape(-1, 3).view(np.uint64))
    got = rays_ref.closest(osc, rays)
    assert np.array_equal(got["object"], ref["object"].reshape(-1)) and (got["object"] >= 0).any() and (got["object"] < 0).any()
    assert np.array_equal(got["t"].view(np.uint64), ref["t"].reshape(-1).view(np.uint64))
    assert np.array_equal(got["point"].view(np.uint64), ref["point"].reshape(-1, 3).view(np.uint64))
    assert np.array_equal(got["normal"].view(np.uint32), ref["normal"].reshape(-1, 4)[:, :3].view(np.uint32))


@pytest.mark.parametrize("name", ["20spheres", "quadratic"])   # (no mirrors: with max_reflections = 0 a mirror blends in the background)
def test_a_frame_composed_from_the_queries_is_the_oracles_frame(oracle, name):
    """max_reflections = 0: closest on the primary rays, occluded on the reference's shadow rays (bias, float direction,
    orc_shadow_ray's max_t), orc_surface_color of the unblocked lights summed in float32 in light order, one clamp: bit for bit
    orc_render_rows.  Pins both acceptance rules to the reference's loops."""
    w, h = 48, 36
    osc = oracle.load_scene(scene_path(name)).with_size(w, h, 0)
    L = oracle.lib()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    rays = rays_ref.primary_rays(osc)
    n64 = np.zeros((len(rays), 3))
    hits = rays_ref.closest(osc, rays, normals64=n64)
    srays, tmax, hit_of, light_of = rays_ref.shadow_rays(osc, hits, n64)
    blocked = rays_ref.occluded(osc, srays, tmax)
    assert not blocked.all() and (blocked.any() or name != "20spheres")
    img = np.broadcast_to(np.asarray(osc.bg_color, dtype=np.float32), (w * h, 3)).copy()
    acc = np.zeros((w * h, 3), dtype=np.float32)
    c = np.zeros(3, dtype=np.float32)
    for j in np.flatnonzero(blocked == 0).tolist():   # (hit-major, light order within a hit)
        i = int(hit_of[j])
        sp, sn = np.ascontiguousarray(hits["point"][i]), np.ascontiguousarray(n64[i])
        albedo = np.asarray(list(osc.objects[int(hits["object"][i])].color), dtype=np.float32)
        L.orc_surface_color(C.byref(osc.lights[int(light_of[j])]), sp.ctypes.data_as(dp), sn.ctypes.data_as(dp), albedo.ctypes.data_as(fp), c.ctypes.data_as(fp))
        acc[i] = acc[i] + c
    hit = hits["object"] >= 0
    img[hit] = np.where(acc[hit] < np.float32(1.0), acc[hit], np.float32(1.0))
    want, cnt = osc.render(counters=True)
    assert int((blocked == 0).sum()) == cnt["surface_colors"] and len(srays) == cnt["shadow_rays"]
    assert np.array_equal(img.reshape(h, w, 3).view(np.uint32), want.view(np.uint32))


def plane_scene(oracle, origin_z):
    """One plane z = origin_z with normal +z: coefficients z - origin_z = 0 (src/surface.cpp:18-25 gives exactly K_Z = 1, K_C = -origin_z)."""
    osc = oracle.Scene(8, 8, 50.0, 0)
    q = np.zeros(20)
    L = oracle.lib()
    dp = C.POINTER(C.c_double)
    o, nv = np.array([0.0, 0.0, origin_z]), np.array([0.0, 0.0, 1.0])
    L.orc_surface_plane(o.ctypes.data_as(dp), nv.ctypes.data_as(dp), q.ctypes.data_as(dp))
    osc.add_object(q, (1, 1, 1))
    return osc


def test_eps_boundary(oracle):
    """The plane z + 1e-7 = 0 from the origin along -z: t is exactly 1e-7 = EPS.  The closest hit accepts it (>=), occlusion does not (>)."""
    osc = plane_scene(oracle, -1e-7)
    assert osc.coefs[0][18] == 1.0 and osc.coefs[0][19] == 1e-7
    rays = rays_ref.make_rays([[0.0, 0.0, 0.0]], [[0.0, 0.0, -1.0]])
    hit = rays_ref.closest(osc, rays)
    assert hit["object"][0] == 0 and hit["t"][0] == 1e-7
    assert rays_ref.occluded(osc, rays)[0] == 0
    assert rays_ref.occluded(osc, rays_ref.make_rays([[0.0, 0.0, 0.0]], [[0.0, 0.0, -0.5]]))[0] == 1   # (t = 2e-7)


def test_t_max_boundary(oracle):
    """A plane at t = 2: not blocked with t_max = 2, blocked with the next double; a NaN t_max blocks nothing."""
    osc = plane_scene(oracle, 2.0)
    rays = rays_ref.make_rays([[0.0, 0.0, 0.0]] * 4, [[0.0, 0.0, 1.0]] * 4)
    assert rays_ref.closest(osc, rays)["t"][0] == 2.0
    got = rays_ref.occluded(osc, rays, [2.0, np.nextafter(2.0, 3.0), np.nan, np.inf])
    assert got.tolist() == [0, 1, 0, 1]
    assert rays_ref.occluded(osc, rays)[0] == 1


def test_declarations(pkg):
    text = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"int rt_trace_rays\(rt_ctx \*\w*, const rt_ray \*\w+, uint32_t \w+, rt_hit \*\w+, void \*\w+, float \*\w+\);", text)
    assert re.search(r"int rt_occluded_rays\(rt_ctx \*\w*, const rt_ray \*\w+, const double \*\w+, uint32_t \w+, int32_t \*\w+, void \*\w+, float \*\w+\);", text)
    assert re.search(r"int rt_trace_rays_host\(rt_ctx \*\w*, const rt_ray \*\w+, uint32_t \w+, rt_hit \*\w+, void \*\w+\);", text)
    assert "#define RT_ABI_VERSION 3" in text and re.search(r"typedef struct rt_ray \{\s*double o\[3\];.*?double d\[3\];", text, flags=re.S)
    lib = pkg.lib()
    for name in ("rt_trace_rays", "rt_occluded_rays", "rt_trace_rays_host"):
        assert hasattr(lib, name) and name in pkg.ABI_SYMBOLS
    assert pkg.RAY_DTYPE.itemsize == 48 and C.sizeof(pkg.Ray) == 48 and pkg.RAY_DTYPE == rays_ref.RAY_DTYPE and pkg.HIT_DTYPE == rays_ref.HIT_DTYPE
    for m in ("trace", "trace_into", "occluded", "occluded_into"):
        assert callable(getattr(pkg.Renderer, m))
    # refusals that need no device: NULL arguments
    assert lib.rt_trace_rays(None, None, 1, None, None, None) == -1 and b"null" in lib.rt_last_error()
    assert lib.rt_occluded_rays(None, None, None, 1, None, None, None) == -1 and b"null" in lib.rt_last_error()
    assert lib.rt_trace_rays_host(None, None, 1, None, None) == -1 and b"null" in lib.rt_last_error()
    upd = C.CDLL(pkg.UPDATE_LIB_PATH)
    assert hasattr(upd, "mi355rt_update_trace")
