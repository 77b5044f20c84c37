"""The primary-hit G-buffer without a GPU: the reference composer (tests/tools/gbuffer_ref.py) against the oracle itself, and the
entry points, record layout and build report of rt_render_gbuffer / rt_pick (include/mi355rt.h)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gbuffer_ref  # noqa: E402


@pytest.mark.parametrize("name,hits", [("20spheres", 283), ("quadratic", 864), ("reflection_test", 876), ("clebsch", 1569)])
def test_composer_agrees_with_the_oracle_render(oracle, name, hits):
    """With max_reflections = 0 the oracle computes one normal per primary hit, so its `normals` counter is the number of pixels
    with an object; and where the composer sees nothing the oracle's pixel is the background, bit for bit."""
    osc = oracle.load_scene(scene_path(name)).with_size(48, 36, 0)
    ref = gbuffer_ref.compose(osc)
    img, cnt = osc.render(counters=True)
    n = int((ref["object"] >= 0).sum())
    assert n == cnt["normals"] == hits
    miss = ref["object"] < 0
    bg = np.asarray(osc.bg_color, dtype=np.float32)
    assert np.array_equal(img[miss].view(np.uint32), np.broadcast_to(bg, img[miss].shape).copy().view(np.uint32))
    assert np.all(np.isinf(ref["t"][miss])) and not ref["normal"][miss].any() and np.all(ref["object"][miss] == -1)
    hit = ~miss
    assert np.all((ref["t"][hit] >= gbuffer_ref.K_EPS) & (ref["t"][hit] < gbuffer_ref.K_MAX_T))
    ln = np.linalg.norm(ref["normal"][hit][:, :3].astype(np.float64), axis=-1)
    assert np.all(np.abs(ln - 1.0) < 1e-6) and not ref["normal"][..., 3].any()


def test_entry_points_are_exported_and_refuse_null(pkg):
    lib = pkg.lib()
    for name in ("rt_render_gbuffer", "rt_pick"):
        assert hasattr(lib, name) and name in pkg.ABI_SYMBOLS
    assert lib.rt_render_gbuffer(None, None, None, None, None, None, None) == -1
    assert b"rt_render_gbuffer" in lib.rt_last_error() and b"null" in lib.rt_last_error()
    assert lib.rt_pick(None, None, None, 0, None, None) == -1
    assert b"rt_pick" in lib.rt_last_error() and b"null" in lib.rt_last_error()
    cam = np.eye(4).reshape(16).copy()
    assert lib.rt_render_gbuffer(None, cam.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None, None) == -1


def test_hit_record_layout_agrees_with_the_header(pkg):
    text = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    m = re.search(r"typedef struct rt_hit \{(.*?)\} rt_hit;", text, flags=re.S)
    assert m, "rt_hit is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields == ["double t", "double point[3]", "float normal[3]", "int32_t object"]
    assert C.sizeof(pkg.Hit) == 48 == pkg.HIT_DTYPE.itemsize
    assert [(n, getattr(pkg.Hit, n).offset) for n, _ in pkg.Hit._fields_] == [("t", 0), ("point", 8), ("normal", 32), ("object", 44)]
    assert [pkg.HIT_DTYPE.fields[n][1] for n in ("t", "point", "normal", "object")] == [0, 8, 32, 44]
    sig = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "int rt_render_gbuffer(rt_ctx *ctx, const double cam[16], int32_t *dev_object, double *dev_t, float *dev_normal, void *stream, float *ms);" in sig
    assert "int rt_pick(rt_ctx *ctx, const double cam[16], const uint32_t *xy, uint32_t n, rt_hit *out_host, void *stream);" in sig
    assert "#define RT_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", text)


def test_update_backend_exports_pick(pkg):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT mi355rt_update_pick\b", out)
    assert os.path.exists(pkg.PICK_DRIVER_PATH)


def test_build_report_lists_the_new_kernels_without_spills():
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    lines = [l for l in open(report).read().splitlines() if l.startswith("rt_gbuffer_")]
    for variant in ("strict", "fast"):
        mine = [l for l in lines if l.startswith(f"rt_gbuffer_{variant}.o")]
        assert sum("gbuffer_kernel" in l for l in mine) == 4, mine   # <gq, cubic> instantiations (picking is a launch mode of the same kernels)
    for l in lines:
        assert re.search(r"VGPR spills +0 +scratch 0$", l.rstrip()), l
