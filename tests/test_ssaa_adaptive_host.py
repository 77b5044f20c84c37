"""Edge-adaptive supersampling (RT_FLAG_SSAA_ADAPTIVE), host side: the ABI constants, the refusals rt_create and
rt_set_ssaa_threshold make without a device, update()'s refusal, and the numpy statement the GPU tests compare against
(tests/tools/ssaa_adaptive_ref.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ssaa_adaptive_ref as ada  # noqa: E402
import ssaa_ref  # noqa: E402


def test_flag_and_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"#define RT_FLAG_SSAA_ADAPTIVE 2048u\b", hdr)
    assert pkg.RT_FLAG_SSAA_ADAPTIVE == 2048
    for name in ("rt_set_ssaa_threshold", "rt_get_ssaa_refined"):
        assert name in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), name)
    assert "rt_multi_set_ssaa_threshold" in pkg.MULTI_ABI_SYMBOLS


def _create_rc(pkg, flags, w=64, h=48):
    sc = pkg.Scene.load_from_file(scene_path("quadratic")).set_size(w, h)
    d = sc.desc()
    cfg = pkg.Config(-1, 0, 1, 8, int(flags), pkg.RT_FMT_RGBA32F)
    ctx = C.c_void_p()
    rc = pkg.lib().rt_create(C.byref(ctx), C.byref(d), C.byref(cfg))
    if rc == 0:
        pkg.lib().rt_destroy(ctx)
    return rc, pkg.lib().rt_last_error().decode()


def test_flag_refused_alone_and_with_both_factors(pkg):
    a = pkg.RT_FLAG_SSAA_ADAPTIVE
    rc, msg = _create_rc(pkg, a)
    assert rc == -1 and "RT_FLAG_SSAA_ADAPTIVE" in msg, (rc, msg)   # RT_ERR_INVALID before the device query
    rc, msg = _create_rc(pkg, a | pkg.RT_FLAG_FAST | pkg.RT_FLAG_COUNT)
    assert rc == -1, (rc, msg)
    rc, msg = _create_rc(pkg, a | pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA4)
    assert rc == -1 and "SSAA" in msg, (rc, msg)
    rc, msg = _create_rc(pkg, a | pkg.RT_FLAG_SSAA4, w=16385, h=8)
    assert rc == -1 and "65536" in msg, (rc, msg)


def test_threshold_refusals_without_a_context(pkg):
    lib = pkg.lib()
    assert lib.rt_set_ssaa_threshold(None, C.c_float(0.1)) == -1
    n = C.c_uint64()
    assert lib.rt_get_ssaa_refined(None, C.byref(n)) == -1


def test_nan_threshold_refused(pkg):
    """A NaN tau is refused (on a live adaptive context when there is a GPU; the check precedes everything else either way)."""
    import torch
    if not torch.cuda.is_available():
        assert pkg.lib().rt_set_ssaa_threshold(None, C.c_float(float("nan"))) == -1
        return
    sc = pkg.Scene.load_from_file(scene_path("quadratic")).set_size(32, 24)
    r = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA_ADAPTIVE)
    with pytest.raises(pkg.RtError):
        r.set_ssaa_threshold(float("nan"))
    r.cleanup_update()


def _scalar_mask(p, tau, halo=None):
    h, w = p.shape[:2]
    below, above = halo if halo is not None else (None, None)
    f = np.float32
    out = np.zeros((h, w), dtype=bool)

    def px(y, x):
        if y == -1:
            return below[x]
        if y == h:
            return above[x]
        return p[y, x]

    for y in range(h):
        for x in range(w):
            if f(tau) < 0:
                out[y, x] = True
                continue
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ny, nx = y + dy, x + dx
                    if (dy, dx) == (0, 0) or not 0 <= nx < w:
                        continue
                    if (ny < 0 and below is None) or (ny >= h and above is None) or ny < -1 or ny > h:
                        continue
                    for c in range(3):
                        with np.errstate(invalid="ignore"):
                            d = abs(f(p[y, x, c]) - f(px(ny, nx)[c]))
                        if not (d <= f(tau)):
                            out[y, x] = True
    return out


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (7, 1), (5, 6), (9, 4)])
@pytest.mark.parametrize("tau", [1.0 / 32.0, 0.0, -1.0, float("inf"), 0.3])
def test_mask_matches_a_scalar_loop(h, w, tau):
    rng = np.random.default_rng(h * 31 + w)
    p = rng.random((h, w, 4), dtype=np.float32)
    p[rng.random((h, w)) < 0.4] = p[0, 0]                # flat patches
    if h * w > 2:
        p[h // 2, w // 2, 1] = np.nan                     # NaN colours refine themselves and their neighbours
    assert np.array_equal(ada.refine_mask(p, tau), _scalar_mask(p, tau))


def test_mask_with_halo_rows():
    rng = np.random.default_rng(3)
    p = rng.random((4, 6, 3), dtype=np.float32).round(1).astype(np.float32)
    below, above = rng.random((6, 3), dtype=np.float32), rng.random((6, 3), dtype=np.float32)
    for halo in [(below, above), (None, above), (below, None), (None, None)]:
        assert np.array_equal(ada.refine_mask(p, 0.05, halo), _scalar_mask(p, 0.05, halo))


@pytest.mark.parametrize("k", [2, 4])
def test_limits_of_compose(k):
    rng = np.random.default_rng(k)
    h, w = 6, 9
    s = rng.random((k * h, k * w, 4), dtype=np.float32)
    p = s[::k, ::k].copy()
    assert np.array_equal(ada.compose(p, s, k, -1.0).view(np.uint32), ssaa_ref.resolve(s, k).view(np.uint32))
    want = p.copy()
    want[..., 3] = 1.0
    assert np.array_equal(ada.compose(p, s, k, float("inf")).view(np.uint32), want.view(np.uint32))
    # a flat frame refines nothing at the default tau; one changed pixel refines its 3x3 block
    flat = np.full((h, w, 4), 0.25, dtype=np.float32)
    assert not ada.refine_mask(flat, 1.0 / 32.0).any()
    flat[2, 3, 0] = 0.5
    m = ada.refine_mask(flat, 1.0 / 32.0)
    assert m.sum() == 9 and m[1:4, 2:5].all()


def test_update_driver_refuses_adaptive_without_ssaa(pkg, tmp_path):
    exe = os.path.join(ROOT, "tests", "host_driver", "update_driver")
    env = {k: v for k, v in os.environ.items() if k != "MI355RT_SSAA"}
    for val in ("", "0.05"):
        env["MI355RT_SSAA_ADAPTIVE"] = val
        p = subprocess.run([exe, scene_path("20spheres"), "64", "48", "-1", str(tmp_path / "f.f32")], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode != 0 and "MI355RT_SSAA_ADAPTIVE: needs MI355RT_SSAA=2 or 4" in p.stderr, (val, p.returncode, p.stderr[-500:])
    env.update(MI355RT_SSAA="2", MI355RT_SSAA_ADAPTIVE="nan")
    p = subprocess.run([exe, scene_path("20spheres"), "64", "48", "-1", str(tmp_path / "f.f32")], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode != 0 and "MI355RT_SSAA_ADAPTIVE" in p.stderr, p.stderr[-500:]
