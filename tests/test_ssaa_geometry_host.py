"""Geometric edges for adaptive supersampling (RT_FLAG_SSAA_GEOMETRY), host side: the ABI constants and entry points, the refusals
rt_create / rt_set_ssaa_geometry / update() make without a device, the numpy statement the GPU tests compare against
(tests/tools/ssaa_geometry_ref.py) held to a scalar loop and to oracle data, and the build report of the new kernel."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_gpu_parity import oracle_from

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gbuffer_ref  # noqa: E402
import ssaa_adaptive_ref as ada  # noqa: E402
import ssaa_geometry_ref as geo  # noqa: E402
import ssaa_ref  # noqa: E402

INF = float("inf")


# ---- header, binding, refusals ----------------------------------------------------------------------------
def test_flag_and_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"#define RT_FLAG_SSAA_GEOMETRY 4096u\b", hdr)
    assert "#define RT_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", hdr)
    sig = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int rt_set_ssaa_geometry(rt_ctx *ctx, float min_cos);" in sig
    assert "int rt_multi_set_ssaa_geometry(rt_multi *m, float min_cos);" in sig
    assert pkg.RT_FLAG_SSAA_GEOMETRY == 4096
    assert "rt_set_ssaa_geometry" in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), "rt_set_ssaa_geometry")
    assert "rt_multi_set_ssaa_geometry" in pkg.MULTI_ABI_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.MULTI_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rt_multi_set_ssaa_geometry\b", out)
    assert pkg.lib().rt_abi_version() & 0xFFF == 3


def _create_rc(pkg, flags, w=64, h=48):
    sc = pkg.Scene.load_from_file(scene_path("quadratic")).set_size(w, h)
    d = sc.desc()
    cfg = pkg.Config(-1, 0, 1, 8, int(flags), pkg.RT_FMT_RGBA32F)
    ctx = C.c_void_p()
    rc = pkg.lib().rt_create(C.byref(ctx), C.byref(d), C.byref(cfg))
    if rc == 0:
        pkg.lib().rt_destroy(ctx)
    return rc, pkg.lib().rt_last_error().decode()


def test_flag_refused_without_adaptive(pkg):
    g = pkg.RT_FLAG_SSAA_GEOMETRY
    rc, msg = _create_rc(pkg, g)
    assert rc == -1 and "RT_FLAG_SSAA_GEOMETRY" in msg, (rc, msg)   # RT_ERR_INVALID before the device query
    rc, msg = _create_rc(pkg, g | pkg.RT_FLAG_SSAA2)
    assert rc == -1 and "RT_FLAG_SSAA_GEOMETRY" in msg, (rc, msg)
    rc, msg = _create_rc(pkg, g | pkg.RT_FLAG_SSAA_ADAPTIVE)        # (no factor: the adaptive flag's own refusal)
    assert rc == -1, (rc, msg)


def test_all_three_flags_reach_the_device_query(pkg):
    import torch
    rc, msg = _create_rc(pkg, pkg.RT_FLAG_SSAA_GEOMETRY | pkg.RT_FLAG_SSAA_ADAPTIVE | pkg.RT_FLAG_SSAA2)
    if torch.cuda.is_available():
        assert rc == 0, (rc, msg)
    else:
        assert rc == pkg.RT_ERR_NO_DEVICE, (rc, msg)


def test_setter_refuses_null(pkg):
    lib = pkg.lib()
    assert lib.rt_set_ssaa_geometry(None, C.c_float(0.5)) == -1
    assert b"rt_set_ssaa_geometry" in lib.rt_last_error()
    assert lib.rt_set_ssaa_geometry(None, C.c_float(float("nan"))) == -1


def test_update_driver_refuses_geometry_without_adaptive(pkg, tmp_path):
    exe = os.path.join(ROOT, "tests", "host_driver", "update_driver")
    env = {k: v for k, v in os.environ.items() if k not in ("MI355RT_SSAA", "MI355RT_SSAA_ADAPTIVE")}
    for ssaa in (None, "4"):
        for val in ("", "0.9"):
            e = dict(env, MI355RT_SSAA_GEOMETRY=val)
            if ssaa:
                e["MI355RT_SSAA"] = ssaa
            p = subprocess.run([exe, scene_path("20spheres"), "64", "48", "-1", str(tmp_path / "f.f32")], capture_output=True, text=True, env=e, timeout=600)
            assert p.returncode != 0 and "MI355RT_SSAA_GEOMETRY: needs MI355RT_SSAA_ADAPTIVE" in p.stderr, (ssaa, val, p.returncode, p.stderr[-500:])
    e = dict(env, MI355RT_SSAA="2", MI355RT_SSAA_ADAPTIVE="", MI355RT_SSAA_GEOMETRY="nan")
    p = subprocess.run([exe, scene_path("20spheres"), "64", "48", "-1", str(tmp_path / "f.f32")], capture_output=True, text=True, env=e, timeout=600)
    assert p.returncode != 0 and "MI355RT_SSAA_GEOMETRY" in p.stderr, p.stderr[-500:]


# ---- geo_mask against a scalar double loop ------------------------------------------------------------------
def _scalar_dot(a, b):
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        return f(f(f(a[0]) * f(b[0])) + f(f(a[1]) * f(b[1]))) + f(f(a[2]) * f(b[2]))


def _scalar_geo(obj, nrm, c, halo=None):
    h, w = obj.shape
    below, above = halo if halo is not None else (None, None)
    out = np.zeros((h, w), dtype=bool)

    def at(y, x):
        if y == -1:
            return int(below[0][x]), below[1][x]
        if y == h:
            return int(above[0][x]), above[1][x]
        return int(obj[y, x]), nrm[y, x]

    for y in range(h):
        for x in range(w):
            o0, n0 = at(y, x)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ny, nx = y + dy, x + dx
                    if (dy, dx) == (0, 0) or not 0 <= nx < w:
                        continue
                    if (ny < 0 and below is None) or (ny >= h and above is None):
                        continue
                    o1, n1 = at(ny, nx)
                    if o1 != o0:
                        out[y, x] = True
                    elif o0 >= 0 and not (_scalar_dot(n0, n1) >= np.float32(c)):
                        out[y, x] = True
    return out


def _random_planes(rng, h, w, nan=True):
    obj = rng.integers(-1, 3, size=(h, w)).astype(np.int32)
    obj[rng.random((h, w)) < 0.5] = 1                       # patches of one object
    n = rng.normal(size=(h, w, 4)).astype(np.float32)
    n[..., :3] /= np.linalg.norm(n[..., :3], axis=-1, keepdims=True)
    n[rng.random((h, w)) < 0.5, :3] = np.float32([0.0, 0.6, 0.8])   # ... with one normal
    n[..., 3] = 0.0
    n[obj < 0] = 0.0
    if nan and h * w > 2:
        obj[h // 2, w // 2] = 1
        n[h // 2, w // 2, 1] = np.nan                        # a NaN normal refines itself and its neighbours of the same object
    return obj, n


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (7, 1), (5, 6), (9, 4), (11, 13)])
@pytest.mark.parametrize("c", [-INF, 0.0, 0.9, 1.0])
def test_geo_mask_matches_a_scalar_loop(h, w, c):
    rng = np.random.default_rng(h * 31 + w)
    obj, n = _random_planes(rng, h, w)
    assert np.array_equal(geo.geo_mask(obj, n, c), _scalar_geo(obj, n, c))


@pytest.mark.parametrize("c", [-INF, 0.0, 0.9, 1.0])
def test_geo_mask_with_halo_rows(c):
    rng = np.random.default_rng(5)
    obj, n = _random_planes(rng, 4, 6)
    (bo, bn), (ao, an) = _random_planes(rng, 1, 6, nan=False), _random_planes(rng, 1, 6, nan=False)
    below, above = (bo[0], bn[0]), (ao[0], an[0])
    for halo in [(below, above), (None, above), (below, None), (None, None)]:
        assert np.array_equal(geo.geo_mask(obj, n, c, halo), _scalar_geo(obj, n, c, halo)), halo


def test_geo_mask_limits():
    h, w = 7, 9
    miss_o, miss_n = np.full((h, w), -1, np.int32), np.zeros((h, w, 4), np.float32)
    for c in (-INF, 0.0, 1.0, INF):
        assert not geo.geo_mask(miss_o, miss_n, c).any()     # an all-miss image: no normal term on misses, whatever c
    one = miss_o.copy()
    one[3, 4] = 0
    n = miss_n.copy()
    n[3, 4, :3] = (0.0, 0.0, -1.0)
    m = geo.geo_mask(one, n, -INF)
    assert m.sum() == 9 and m[2:5, 3:6].all()                # a one-pixel object: its 3 x 3 block
    # one object everywhere with one normal: nothing at c <= 1, everything above; a NaN normal at c = -inf: its 3 x 3 block
    flat_o = np.zeros((h, w), np.int32)
    flat_n = np.zeros((h, w, 4), np.float32)
    flat_n[..., 2] = -1.0
    assert not geo.geo_mask(flat_o, flat_n, 1.0).any() and geo.geo_mask(flat_o, flat_n, 1.5).all()
    flat_n[3, 4, 0] = np.nan
    m = geo.geo_mask(flat_o, flat_n, -INF)
    assert m.sum() == 9 and m[2:5, 3:6].all()
    # a band edge is not an image edge: the halo row's other object marks the top row
    m = geo.geo_mask(flat_o[:2], np.nan_to_num(flat_n[:2]), -INF, (None, (np.full(w, 1, np.int32), flat_n[0])))
    assert m[1].all() and not m[0].any()


# ---- the compose on oracle data ----------------------------------------------------------------------------
def lightless_scene(pkg, w=40, h=30):
    """Three overlapping spheres and a plane behind them, no lights, black background: every pixel of P is black."""
    s = pkg.Scene.new(w, h, 50.0, 2, (0.0, 0.0, 0.0))
    s.add_object(pkg.surface_make("sphere", [-1.5, 0.2, 10], [2.0]), (0.9, 0.2, 0.2))
    s.add_object(pkg.surface_make("sphere", [1.0, -0.3, 9], [1.5]), (0.9, 0.2, 0.2))
    s.add_object(pkg.surface_make("sphere", [3.5, 2.0, 14], [1.0]), (0.2, 0.9, 0.2), 0.5)
    s.add_object(pkg.surface_make("plane", [0, -2.5, 0], [0, 1, 0.1]), (0.5, 0.5, 0.5))
    return s


def test_compose_on_a_lightless_scene(pkg, oracle):
    k = 2
    osc = oracle_from(pkg, oracle, lightless_scene(pkg))
    p = osc.render(nthreads=8)
    s = osc.with_size(k * osc.width, k * osc.height).render(nthreads=8)
    assert not p[..., :3].any() and not s[..., :3].any()
    g = gbuffer_ref.compose(osc)
    obj, nrm = g["object"], g["normal"]
    for tau in (0.0, 1.0 / 32.0, INF):
        assert not ada.refine_mask(p, tau).any()              # the colour term sees nothing at all
    m = geo.geo_mask(obj, nrm, -INF)
    # exactly the silhouettes: the pixels with a neighbour of another object
    sil = np.zeros_like(m)
    h, w = obj.shape
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, xs = slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx))
            yn, xn = slice(max(0, dy), h - max(0, -dy)), slice(max(0, dx), w - max(0, -dx))
            sil[ys, xs] |= obj[ys, xs] != obj[yn, xn]
    assert np.array_equal(m, sil) and 0 < m.sum() < m.size and len(np.unique(obj)) == 5
    out = geo.compose(p, s, k, 1.0 / 32.0, obj, nrm, -INF)
    r = ssaa_ref.resolve(s, k)
    assert np.array_equal(out[m].view(np.uint32), r[m].view(np.uint32))
    assert np.array_equal(out[~m][:, :3].view(np.uint32), p[~m][:, :3].view(np.uint32)) and np.all(out[..., 3] == 1.0)
    # a finite threshold adds the curved interiors but never a miss next to misses
    m9 = geo.geo_mask(obj, nrm, 0.999)
    assert (m9 & ~m).any() and (m9 | ~m).all()


@pytest.mark.parametrize("k", [2, 4])
def test_compose_with_one_object_everywhere_is_the_adaptive_compose(oracle, k):
    osc = oracle.load_scene(scene_path("20spheres")).with_size(32, 24, 2)
    p = osc.render(nthreads=8)
    s = osc.with_size(k * 32, k * 24).render(nthreads=8)
    obj = np.full((24, 32), 7, np.int32)
    nrm = np.random.default_rng(k).normal(size=(24, 32, 4)).astype(np.float32)
    for tau in (-1.0, 0.0, 1.0 / 32.0, INF):
        a, b = geo.compose(p, s, k, tau, obj, nrm, -INF), ada.compose(p, s, k, tau)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), tau


# ---- build report ------------------------------------------------------------------------------------------
def test_build_report_lists_the_new_kernel_without_spills():
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    lines = [l for l in open(report).read().splitlines() if "classify_geometry_k" in l]   # (the report cuts mangled names at 40 characters)
    for variant in ("strict", "fast"):
        mine = [l for l in lines if l.startswith(f"rt_adaptive_{variant}.o")]
        assert len(mine) == 2, mine                            # <RGBA8> instantiations
    for l in lines:
        assert re.search(r"VGPR spills +0 +scratch 0$", l.rstrip()), l
