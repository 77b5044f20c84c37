"""rt_object_extents without a GPU (include/mi355rt.h, "Object extents"): the reference composer
(tests/tools/extents_ref.py) against a plain double loop over the pixels, the identities, the merge of ranks, and the declarations, record
layout, refusals and build report of the entry points.  Of the refusals only those that are decided before the context is read can be
driven here (NULL arguments, a misaligned device output, x0 > x1, y0 > y1): x1 >= W, y1 >= H and the supersampling flags are properties of
a context, and rt_create makes none without a device -- behind its argument checks it asks hipGetDeviceCount and returns
RT_ERR_NO_DEVICE before the frame geometry or the supersampling factor of the context exist (csrc/rt_capi.cpp, rt_create) --, so
tests/test_extents_gpu.py holds them (test_rectangles)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import extents_ref  # noqa: E402
import gbuffer_ref  # noqa: E402
import launch_table as LT  # noqa: E402

INF_BITS = 0x7FF0000000000000


def plain_loop(planes, n, xs, ys, rect):
    """The definition read aloud: one pass over the pixels, Python scalars only."""
    rec = [dict(pixels=0, x_min=0xFFFFFFFF, y_min=0xFFFFFFFF, x_max=0, y_max=0, t_min=float("inf"), t_max=0.0) for _ in range(n)]
    for j, y in enumerate(ys):
        for i, x in enumerate(xs):
            if rect is not None and not (rect[0] <= x <= rect[2] and rect[1] <= y <= rect[3]):
                continue
            o, t = int(planes["object"][j, i]), float(planes["t"][j, i])
            if o < 0:
                continue
            r = rec[o]
            r["pixels"] += 1
            r["x_min"], r["x_max"] = min(r["x_min"], x), max(r["x_max"], x)
            r["y_min"], r["y_max"] = min(r["y_min"], y), max(r["y_max"], y)
            r["t_min"], r["t_max"] = min(r["t_min"], t), max(r["t_max"], t)
    out = np.zeros(n, dtype=extents_ref.DTYPE)
    for k, r in enumerate(rec):
        out[k] = tuple(r[f] for f in extents_ref.DTYPE.names)
    return out


@pytest.mark.parametrize("name", ["20spheres", "quadratic"])
def test_composer_equals_a_plain_loop_over_the_pixels(oracle, name):
    w, h = 40, 30
    osc = oracle.load_scene(scene_path(name)).with_size(w, h, 0)
    cam = oracle.camera_matrix(pos=(0.4, 0.3, -1.5), yaw_deg=84.0, pitch_deg=-3.0)
    planes = gbuffer_ref.compose(osc, cam)
    n = len(osc.objects)
    seen = 0
    for rect in (None, (0, 0, w - 1, h - 1), (7, 5, 29, 21), (20, 15, 20, 15), (0, 0, 15, 15)):
        got = extents_ref.compose(osc, cam, rect)
        assert extents_ref.same(got, plain_loop(planes, n, range(w), range(h), rect)), (name, rect)
        seen += int((got["pixels"] > 0).sum())
    full = extents_ref.compose(osc, cam)
    assert seen > 0 and int(full["pixels"].sum()) == int((planes["object"] >= 0).sum())
    # rows given out of a rank's hands: only they count
    rows = np.array([3, 4, 5, 16, 17, 29])
    assert extents_ref.same(extents_ref.compose(osc, cam, (2, 4, 37, 20), rows=rows),
                            plain_loop({k: planes[k][[4, 5, 16, 17]] for k in ("object", "t")}, n, range(w), [4, 5, 16, 17], (2, 4, 37, 20)))


def test_an_unseen_object_gets_the_identities(oracle):
    """A sphere in front of the camera, one behind it and one far off to the side: records 1 and 2 are the identities, value by value."""
    osc = oracle.Scene(32, 24, 50.0, 0, (0.0, 0.0, 0.0))
    for c, r in (((0.0, 0.0, 10.0), 2.0), ((0.0, 0.0, -10.0), 2.0), ((500.0, 0.0, 10.0), 2.0)):
        coefs = np.zeros(20)
        coefs[10:13] = 1.0                      # x2, y2, z2
        coefs[16:19] = [-2.0 * v for v in c]    # x, y, z
        coefs[19] = sum(v * v for v in c) - r * r
        osc.add_object(coefs, (1.0, 1.0, 1.0))
    got = extents_ref.compose(osc)
    assert got["pixels"][0] > 0 and got["x_min"][0] <= got["x_max"][0] < 32 and got["y_min"][0] <= got["y_max"][0] < 24
    assert 8.0 - 1e-9 <= got["t_min"][0] <= got["t_max"][0] < 10.0
    for k in (1, 2):
        r = got[k]
        assert (int(r["pixels"]), int(r["x_min"]), int(r["y_min"]), int(r["x_max"]), int(r["y_max"])) == (0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0)
        assert r["t_min"].view(np.uint64) == INF_BITS and r["t_max"].view(np.uint64) == 0   # +inf and +0.0, on the bits
    assert extents_ref.same(got[1:], extents_ref.identity(2))
    assert extents_ref.same(extents_ref.compose(osc, rect=(0, 0, 3, 3)), extents_ref.identity(3))   # a rectangle on background


def test_ranks_merge_to_the_whole_frame(pkg, oracle):
    w, h, band = 40, 30, 8
    osc = oracle.load_scene(scene_path("20spheres")).with_size(w, h, 0)
    for rect in (None, (5, 3, 33, 27), (0, 8, 39, 15)):
        whole = extents_ref.compose(osc, rect=rect)
        parts = [extents_ref.compose(osc, rect=rect, rows=pkg.band_rows_of_rank(h, band, 2, rank)) for rank in range(2)]
        assert extents_ref.same(extents_ref.merge(parts[0], parts[1]), whole), rect
        assert (whole["pixels"] > 0).any()
    assert extents_ref.same(parts[0], extents_ref.identity(len(osc.objects)))   # rows 8 .. 15 are rank 1's alone
    assert extents_ref.same(extents_ref.merge(extents_ref.identity(4), extents_ref.identity(4)), extents_ref.identity(4))


def test_entry_points_record_and_kernels_member_are_declared(pkg, tmp_path):
    lib = pkg.lib()
    for name in ("rt_object_extents", "rt_object_extents_host"):
        assert hasattr(lib, name) and name in pkg.ABI_SYMBOLS
    assert lib.rt_abi_version() == 3
    text = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    sig = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "int rt_object_extents(rt_ctx *ctx, const double cam[16], const uint32_t rect[4] , rt_object_extent *dev_out , void *stream, float *ms);" in sig
    assert "int rt_object_extents_host(rt_ctx *ctx, const double cam[16], const uint32_t rect[4], rt_object_extent *out_host, void *stream);" in sig
    assert "#define RT_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", text)
    assert "rt_object_extents" in re.search(r"The passes that READ the scene --(.*?)need no ordering", text, flags=re.S).group(1)
    src = tmp_path / "size.c"
    src.write_text('#include "mi355rt.h"\n#include <stddef.h>\n_Static_assert(sizeof(rt_object_extent) == 40 && _Alignof(rt_object_extent) == 8, "size");\n'
                   '_Static_assert(offsetof(rt_object_extent, x_min) == 8 && offsetof(rt_object_extent, y_max) == 20, "box");\n'
                   '_Static_assert(offsetof(rt_object_extent, t_min) == 24 && offsetof(rt_object_extent, t_max) == 32, "t");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")], check=True)
    assert pkg.EXTENT_DTYPE.itemsize == 40 and pkg.EXTENT_DTYPE == extents_ref.DTYPE
    assert [pkg.EXTENT_DTYPE.fields[n][1] for n in pkg.EXTENT_DTYPE.names] == [0, 8, 12, 16, 20, 24, 32]
    launch = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc", "rt_launch.h")).read()
    # the member of the launcher table (struct QueryLaunchers, one per path in struct Kernels), and the staged path's slot names this launcher
    kernels = re.search(r"struct QueryLaunchers \{(.*?)\};", launch, flags=re.S).group(1)
    assert "decltype(&rt_launch_object_extents_strict) object_extents;" in kernels
    assert "QueryLaunchers query[3];" in re.search(r"struct Kernels \{(.*?)\};", launch, flags=re.S).group(1)
    assert LT.slot_of("rt_launch_object_extents") == "query[PATH_STAGED].object_extents"
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("rt_launch_object_extents_strict", "rt_launch_object_extents_fast", "rt_extents_lds_accumulators_strict"):
        assert re.search(rf"\bT {sym}\b", out), sym
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT mi355rt_update_extents\b", out)


def test_refusals_that_need_no_device(pkg):
    lib = pkg.lib()
    err = lib.rt_last_error
    cam = np.eye(4).reshape(16).copy()
    camp = cam.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros(64, dtype=np.uint64)
    # nothing below reads the context (a rectangle with x0 > x1 or y0 > y1 is refused before the image size is looked at): any non-NULL handle
    # will do; it still gets 64 KiB of zeroes, more than any rt_ctx, so that a mistake here would read zeroes and not foreign memory
    keep = C.create_string_buffer(1 << 16)
    handle = C.c_void_p(C.addressof(keep))
    for name, tail in (("rt_object_extents", (None, None)), ("rt_object_extents_host", (None,))):
        fn = getattr(lib, name)
        for args in ((None, camp, None, C.c_void_p(out.ctypes.data)), (handle, None, None, C.c_void_p(out.ctypes.data)), (handle, camp, None, None)):
            assert fn(*args, *tail) == -1
            assert name.encode() + b": null argument" in err(), err()
        for off in (1, 2, 4, 7, 12) if name == "rt_object_extents" else ():   # (device memory only: a host array is merely copied into)
            assert fn(handle, camp, None, C.c_void_p(out.ctypes.data + off), *tail) == -1
            assert name.encode() + b":" in err() and b"8-byte aligned" in err(), err()
        for rect in ((5, 0, 4, 3), (0, 9, 7, 8), (0xFFFFFFFF, 0, 0, 0), (3, 2, 1, 0)):
            r = np.array(rect, dtype=np.uint32)
            assert fn(handle, camp, r.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_void_p(out.ctypes.data), *tail) == -1
            assert name.encode() + b": rect" in err() and b"not a rectangle" in err(), err()
    upd = C.CDLL(pkg.UPDATE_LIB_PATH)
    upd.mi355rt_update_extents.argtypes = [C.POINTER(C.c_uint32), C.c_void_p, C.c_uint]
    assert upd.mi355rt_update_extents(None, C.c_void_p(out.ctypes.data), 1) == -1 and b"mi355rt_update_extents" in err()


def test_the_size_function_switches_where_160_kib_are_full(pkg):
    """Sphere scenes stage 64 bytes of class table per object (rt_scene_dev.h: UsEntry) and accumulate in 40: 104 n <= 163840."""
    fn = pkg.lib().rt_extents_lds_accumulators_strict
    fn.argtypes = [C.c_size_t, C.c_uint32]
    assert fn(0, 0) == 1 and fn(64 * 1575, 1575) == 1 and fn(64 * 1576, 1576) == 0
    assert fn(160 * 1024, 0) == 1 and fn(160 * 1024 - 39, 1) == 0
    fast = pkg.lib().rt_extents_lds_accumulators_fast
    fast.argtypes = [C.c_size_t, C.c_uint32]
    assert all(fast(64 * n, n) == fn(64 * n, n) for n in (1, 1575, 1576, 4000))


# build/spills.txt of the parent commit: the instantiations of rt_gbuffer.hip, which gains the new kernels (file, kernel, VGPRs, occupancy)
PARENT_GBUFFER = [
    ("rt_gbuffer_fast.o", "_ZN8rtk_fast14gbuffer_kernelILb1ELb1EEEv", 132, 3), ("rt_gbuffer_fast.o", "_ZN8rtk_fast14gbuffer_kernelILb0ELb1EEEv", 132, 3),
    ("rt_gbuffer_fast.o", "_ZN8rtk_fast14gbuffer_kernelILb1ELb0EEEv", 84, 5), ("rt_gbuffer_fast.o", "_ZN8rtk_fast14gbuffer_kernelILb0ELb0EEEv", 56, 8),
    ("rt_gbuffer_strict.o", "_ZN10rtk_strict14gbuffer_kernelILb1ELb1E", 152, 3), ("rt_gbuffer_strict.o", "_ZN10rtk_strict14gbuffer_kernelILb0ELb1E", 152, 3),
    ("rt_gbuffer_strict.o", "_ZN10rtk_strict14gbuffer_kernelILb1ELb0E", 90, 5), ("rt_gbuffer_strict.o", "_ZN10rtk_strict14gbuffer_kernelILb0ELb0E", 56, 8),
]


def test_build_report_lists_the_new_kernels_without_spills_and_keeps_the_old_lines():
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    lines = [l.rstrip() for l in open(report).read().splitlines() if l.startswith("rt_gbuffer_")]
    for variant in ("strict", "fast"):
        mine = [l for l in lines if l.startswith(f"rt_gbuffer_{variant}.o") and "extents_kernel" in l]
        assert len(mine) == 4, mine   # <gq, cubic>
        assert sum("extents_init_kernel" in l for l in lines if l.startswith(f"rt_gbuffer_{variant}.o")) == 1
        for l in mine:
            assert re.search(r"VGPR spills +0 +scratch 0$", l), l
    old = [l for l in lines if "extents" not in l]
    got = []
    for l in old:
        m = re.match(r"(\S+) +(\S+) VGPRs +(\d+) +occupancy +(\d+) +SGPR spills +0 +VGPR spills +0 +scratch 0$", l)
        assert m, l
        got.append((m.group(1), m.group(2), int(m.group(3)), int(m.group(4))))
    assert sorted(got) == sorted(PARENT_GBUFFER)
