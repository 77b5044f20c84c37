"""Supersampling (RT_FLAG_SSAA2 / RT_FLAG_SSAA4), host side: the ABI constants, the refusals rt_create makes before it looks for a
device (so they hold with or without a GPU), and the numpy statement of the resolve the GPU tests compare against
(tests/tools/ssaa_ref.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ssaa_ref  # noqa: E402


def test_flags_in_header_and_binding(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"#define RT_FLAG_SSAA2 512u\b", hdr) and re.search(r"#define RT_FLAG_SSAA4 1024u\b", hdr)
    assert "#define RT_ABI_VERSION 3" in hdr
    assert pkg.RT_FLAG_SSAA2 == 512 and pkg.RT_FLAG_SSAA4 == 1024
    # no bit shared with the other flags or the multi layer's
    others = (pkg.RT_FLAG_FAST | pkg.RT_FLAG_COUNT | pkg.RT_FLAG_SIMPLE | pkg.RT_FLAG_NOCULL | pkg.RT_FLAG_STATIC_ORDER | pkg.RT_FLAG_NOSCAN
              | pkg.RT_FLAG_PLAIN_ORDER | pkg.RT_FLAG_NOSPLIT | pkg.RT_FLAG_NOLEAN | pkg.RT_MULTI_SELF_EXCHANGE | pkg.RT_MULTI_BANDWISE | pkg.RT_MULTI_SPARSE)
    assert not (others & (pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA4))


def _create_rc(pkg, w, h, flags):
    import ctypes as C
    sc = pkg.Scene.load_from_file(scene_path("quadratic")).set_size(w, h)
    d = sc.desc()
    cfg = pkg.Config(-1, 0, 1, 8, int(flags), pkg.RT_FMT_RGBA32F)
    ctx = C.c_void_p()
    rc = pkg.lib().rt_create(C.byref(ctx), C.byref(d), C.byref(cfg))
    if rc == 0:
        pkg.lib().rt_destroy(ctx)
    return rc, pkg.lib().rt_last_error().decode()


def test_both_factors_refused_before_the_device_query(pkg):
    rc, msg = _create_rc(pkg, 64, 48, pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA4)
    assert rc == -1 and "SSAA" in msg, (rc, msg)   # RT_ERR_INVALID, not RT_ERR_NO_DEVICE
    rc, _ = _create_rc(pkg, 64, 48, pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA4 | pkg.RT_FLAG_FAST)
    assert rc == -1


@pytest.mark.parametrize("k,w,h", [(2, 32769, 100), (2, 100, 32769), (4, 16385, 64), (4, 64, 16385)])
def test_oversized_sample_grid_refused(pkg, k, w, h):
    rc, msg = _create_rc(pkg, w, h, pkg.RT_FLAG_SSAA2 if k == 2 else pkg.RT_FLAG_SSAA4)
    assert rc == -1 and "65536" in msg, (rc, msg)


def test_sizes_at_the_limit_get_past_the_checks(pkg):
    """k*W = 65536 is allowed: without a GPU rt_create gets as far as the device query, with one it creates the context."""
    import torch
    rc, msg = _create_rc(pkg, 16384, 8, pkg.RT_FLAG_SSAA4)
    assert rc in (0, -4), (rc, msg)
    if not torch.cuda.is_available():
        assert rc == -4


@pytest.mark.parametrize("k", [2, 4])
def test_resolve_of_identical_samples_is_exact(k):
    """Power-of-two trees and 1/k^2: a block of k x k equal values resolves to exactly that value (so a pure background pixel
    stays bit-equal to the background), for random float32 colours including subnormals and values above 1."""
    rng = np.random.default_rng(7 + k)
    h, w = 9, 13
    v = rng.random((h, w, 3), dtype=np.float32)
    v[0, 0] = np.float32(1e-40)   # subnormal
    v[1, 1] = np.float32(3.5)
    v[2, 2] = 0.0
    s = np.repeat(np.repeat(v, k, axis=0), k, axis=1)
    out = ssaa_ref.resolve(s, k)
    assert out.shape == (h, w, 4) and out.dtype == np.float32
    assert np.array_equal(out[..., :3].view(np.uint32), v.view(np.uint32))
    assert np.all(out[..., 3] == 1.0)


@pytest.mark.parametrize("k", [2, 4])
def test_resolve_matches_a_scalar_statement(k):
    """The vectorised helper against a scalar loop over the contract's order, float32 at every step; RGBA8 against the kernels'
    (unsigned char)(int)(v * 255 + 0.5)."""
    rng = np.random.default_rng(100 + k)
    h, w = 5, 7
    s = rng.random((k * h, k * w, 4), dtype=np.float32)
    out = ssaa_ref.resolve(s, k)
    q = ssaa_ref.resolve_rgba8(s, k)
    f = np.float32
    for y in range(h):
        for x in range(w):
            for c in range(3):
                def sub(j):
                    e = [s[k * y + j, k * x + i, c] for i in range(k)]
                    return f(e[0] + e[1]) if k == 2 else f(f(e[0] + e[1]) + f(e[2] + e[3]))
                r = [sub(j) for j in range(k)]
                tot = f(r[0] + r[1]) if k == 2 else f(f(r[0] + r[1]) + f(r[2] + r[3]))
                want = f(tot * f(1.0 / (k * k)))
                assert out[y, x, c].view(np.uint32) == want.view(np.uint32), (y, x, c)
                assert q[y, x, c] == int(f(f(want * f(255.0)) + f(0.5))) & 0xFF, (y, x, c)
            assert q[y, x, 3] == 255 and out[y, x, 3] == 1.0


def test_resolve_order_is_not_a_plain_sum():
    """The tree order is observable: samples chosen so that ((a + b) + (c + d)) differs from a left-to-right sum."""
    a, b, c, d = np.float32(1.0), np.float32(0.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24)
    s = np.array([[[a, a, a, 1], [b, b, b, 1]], [[c, c, c, 1], [d, d, d, 1]]], dtype=np.float32)
    got = ssaa_ref.resolve(s, 2)[0, 0, 0]
    tree = np.float32(np.float32(a + b) + np.float32(c + d)) * np.float32(0.25)
    seq = np.float32(np.float32(np.float32(a + b) + c) + d) * np.float32(0.25)
    assert got == tree and tree != seq


def test_quantise_matches_the_kernel_expression():
    vals = np.array([0.0, 1.0, 0.5, 1.0 / 255.0, 0.00196078, 0.998, np.nextafter(np.float32(0.5 / 255.0), np.float32(0))], dtype=np.float32)
    img = np.stack([vals, vals, vals], axis=-1)[None]
    q = ssaa_ref.quantise(img)
    for i, v in enumerate(vals):
        t = np.float32(np.float32(v * np.float32(255.0)) + np.float32(0.5))
        assert q[0, i, 0] == int(t) and q[0, i, 3] == 255


def test_update_driver_rejects_other_factors(pkg, tmp_path):
    """MI355RT_SSAA accepts 2 and 4; init_update refuses anything else through die_text before it looks for a device."""
    exe = os.path.join(ROOT, "tests", "host_driver", "update_driver")
    for bad in ("3", "1", "x"):
        env = dict(os.environ, MI355RT_SSAA=bad)
        p = subprocess.run([exe, scene_path("20spheres"), "64", "48", "-1", str(tmp_path / "f.f32")], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode != 0 and "MI355RT_SSAA: expected 2 or 4" in p.stderr, (bad, p.returncode, p.stderr[-500:])
