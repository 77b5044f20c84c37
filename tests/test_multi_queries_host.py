"""The multi-GPU layer's scene updates, G-buffer, extents and query context without a GPU (include/mi355rt.h, "Several GPUs"; DESIGN.md
section 21): the prototypes, the symbol lists and the library each symbol lives in, the refusals that are decided before a device is
looked for, the build's register report for csrc/rt_planes.hip, and the numpy restatements the GPU file
(tests/test_multi_queries_gpu.py) compares the two root-side kernels with."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import extents_ref  # noqa: E402

BASE_NEW = ("rt_assemble_planes", "rt_merge_object_extents")
MULTI_NEW = ("rt_set_scene_multi", "rt_multi_set_scene_status", "rt_multi_query_ctx", "rt_render_gbuffer_multi", "rt_object_extents_multi",
             "rt_object_extents_multi_host")
PROTOTYPES = (
    "int rt_assemble_planes(rt_ctx *ctx, const void *gathered, size_t slot_stride_bytes, void *full, uint32_t elem_bytes, void *stream);",
    "int rt_merge_object_extents(rt_ctx *ctx, const rt_object_extent *dev_parts, uint32_t n_parts, rt_object_extent *dev_out, void *stream);",
    "int rt_set_scene_multi(rt_multi *m, const rt_scene_update *host);",
    "int rt_multi_set_scene_status(rt_multi *m, uint64_t *applied, uint64_t *rejected, uint32_t *reason, uint32_t *index);",
    "rt_ctx *rt_multi_query_ctx(rt_multi *m);",
    "int rt_render_gbuffer_multi(rt_multi *m, const double cam[16], int32_t *root_object, double *root_t, float *root_normal, float *ms);",
    "int rt_object_extents_multi(rt_multi *m, const double cam[16], const uint32_t rect[4], rt_object_extent *root_dev_out, float *ms);",
    "int rt_object_extents_multi_host(rt_multi *m, const double cam[16], const uint32_t rect[4], rt_object_extent *out_host);",
)


# ---- the numpy restatements the GPU file imports ------------------------------------------------------------------------------------------
def assemble_planes_ref(pkg, gathered, slot_elems, width, height, band_rows, world):
    """rt_assemble_planes: gathered = flat array of elements, rank q's [max_local_rows][width] at q * slot_elems; the full [height][width]
    plane by the row mapping of pkg.assemble_index (row y's position in a rank-major buffer of max_local_rows rows per rank)."""
    mx = pkg.max_local_rows(height, band_rows, world)
    idx = pkg.assemble_index(height, band_rows, world)
    rank, lr = idx // mx, idx % mx
    start = rank * slot_elems + lr * width
    return gathered[start[:, None] + np.arange(width)[None, :]]


def merge_ref(parts):
    """rt_merge_object_extents: parts [n_parts, n_objects] records folded with extents_ref.merge, starting from the identities."""
    out = extents_ref.identity(parts.shape[1])
    for p in parts:
        out = extents_ref.merge(out, p)
    return out


def test_the_restatements_on_hand_stated_values(pkg):
    # 7 rows, bands of 2, 3 ranks: bands 0..3 = rows (0,1) (2,3) (4,5) (6); rank 0 owns bands 0 and 3, so max_local_rows = 3
    g = np.full(3 * 5 * 2, -1, dtype=np.int64)   # slots of 5 rows' worth (a stride larger than a slot), width 2
    rows_of = {0: [0, 1, 6], 1: [2, 3], 2: [4, 5]}
    for q, rows in rows_of.items():
        for lr, y in enumerate(rows):
            g[q * 10 + lr * 2: q * 10 + lr * 2 + 2] = (10 * y, 10 * y + 1)
    full = assemble_planes_ref(pkg, g, 10, 2, 7, 2, 3)
    assert full.tolist() == [[10 * y, 10 * y + 1] for y in range(7)]
    a, b = extents_ref.identity(3), extents_ref.identity(3)
    a[0] = (4, 2, 3, 5, 6, 1.5, 2.5)
    b[0] = (1, 1, 9, 1, 9, 2.0, 7.0)
    b[2] = (2, 0, 0, 1, 0, 1e-7, 999999.0)
    got = merge_ref(np.stack([a, b]))
    assert tuple(got[0]) == (5, 1, 3, 5, 9, 1.5, 7.0) and extents_ref.same(got[1:2], extents_ref.identity(1)) and got[2] == b[2]
    assert extents_ref.same(merge_ref(np.stack([extents_ref.identity(4)] * 3)), extents_ref.identity(4))


# ---- declarations ------------------------------------------------------------------------------------------------------------------------
def test_prototypes_symbol_lists_and_libraries(pkg):
    text = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    sig = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for proto in PROTOTYPES:
        assert proto in sig, proto
    assert "#define RT_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", text)
    assert not re.search(r"\(rt_\*_multi\) has no", text)   # the sentences this layer's entry points made untrue
    for name in BASE_NEW:
        assert name in pkg.ABI_SYMBOLS and name not in pkg.MULTI_ABI_SYMBOLS
    for name in MULTI_NEW:
        assert name in pkg.MULTI_ABI_SYMBOLS and name not in pkg.ABI_SYMBOLS
    base = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    multi = subprocess.run(["nm", "-D", "--defined-only", pkg.MULTI_LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in BASE_NEW + ("rt_launch_assemble_planes", "rt_launch_merge_extents"):
        assert re.search(rf"\bT {name}\b", base) and not re.search(rf"\bT {name}\b", multi), name
    for name in MULTI_NEW:
        assert re.search(rf"\bT {name}\b", multi) and not re.search(rf"\bT {name}\b", base), name
    assert pkg.lib().rt_abi_version() == 3
    launch = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc", "rt_launch.h")).read()
    assert "rt_launch_assemble_planes(" in launch and "rt_launch_merge_extents(" in launch
    for m in ("set_scene", "set_scene_status", "gbuffer", "gbuffer_into", "object_extents", "object_extents_into", "pick", "pick_paths", "trace", "occluded", "shade",
              "paths"):
        assert callable(getattr(pkg.MultiRenderer, m)), m


def test_the_update_adapter_resolves_the_new_symbols():
    src = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "host", "src", "update-hip.cpp")).read()
    for name in ("rt_multi_query_ctx", "rt_multi_stream", "rt_set_scene_multi", "rt_multi_set_scene_status"):
        assert f'dlsym(g_multi_lib, "{name}")' in src, name
    assert "mi355rt_update_extents: not available with several devices (MI355RT_DEVICES)" in src   # (tests/test_extents_gpu.py pins that answer)
    assert "mi355rt_update_pick: not available with several devices (MI355RT_DEVICES)" in src      # (... and tests/test_gbuffer_gpu.py this one)
    for hook in ("pick_path", "trace", "shade", "scene"):
        assert f"mi355rt_update_{hook}: not available with several devices" not in src, hook


# ---- refusals that need no device -------------------------------------------------------------------------------------------------------
def test_every_new_function_refuses_null_and_names_itself(pkg):
    lib, multi = pkg.lib(), pkg.multi_lib()
    err = lib.rt_last_error
    cam = np.eye(4).reshape(16).copy()
    camp = cam.ctypes.data_as(C.POINTER(C.c_double))
    buf = np.zeros(64, dtype=np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    u = pkg.SceneUpdate()
    # a non-NULL handle that is never read: the NULL checks come first (64 KiB of zeroes, so that a mistake here would read zeroes)
    keep = C.create_string_buffer(1 << 16)
    h = C.c_void_p(C.addressof(keep))
    cases = [
        ("rt_assemble_planes", lib.rt_assemble_planes, [(None, p, 64, p, 4, None), (h, None, 64, p, 4, None), (h, p, 64, None, 4, None)]),
        ("rt_merge_object_extents", lib.rt_merge_object_extents, [(None, p, 1, p, None), (h, None, 1, p, None), (h, p, 1, None, None)]),
        ("rt_set_scene_multi", multi.rt_set_scene_multi, [(None, C.byref(u)), (h, None)]),
        ("rt_multi_set_scene_status", multi.rt_multi_set_scene_status, [(None, None, None, None, None)]),
        ("rt_render_gbuffer_multi", multi.rt_render_gbuffer_multi, [(None, camp, p, None, None, None), (h, None, p, None, None, None)]),
        ("rt_object_extents_multi", multi.rt_object_extents_multi, [(None, camp, None, p, None), (h, None, None, p, None), (h, camp, None, None, None)]),
        ("rt_object_extents_multi_host", multi.rt_object_extents_multi_host, [(None, camp, None, p), (h, None, None, p), (h, camp, None, None)]),
    ]
    for name, fn, calls in cases:
        for args in calls:
            lib.rt_set_last_error(b"")
            assert fn(*args) == -1, (name, args)
            assert name.encode() + b": null argument" in err(), (name, err())
    lib.rt_set_last_error(b"")
    assert multi.rt_multi_query_ctx(None) is None and b"rt_multi_query_ctx: null argument" in err()
    # decided from the arguments alone, in front of anything that reads the context
    assert lib.rt_assemble_planes(h, p, 64, p, 3, None) == -1 and b"rt_assemble_planes: elem_bytes is 3" in err()
    assert lib.rt_assemble_planes(h, p, 64, p, 32, None) == -1 and b"rt_assemble_planes: elem_bytes is 32" in err()
    assert lib.rt_merge_object_extents(h, p, 0, p, None) == -1 and b"rt_merge_object_extents: n_parts is 0" in err()
    assert lib.rt_merge_object_extents(h, C.c_void_p(buf.ctypes.data + 4), 1, p, None) == -1 and b"rt_merge_object_extents" in err() and b"8-byte aligned" in err()
    assert multi.rt_render_gbuffer_multi(h, camp, None, None, None, None) == -1 and b"rt_render_gbuffer_multi: all three planes are null" in err()
    assert multi.rt_object_extents_multi(h, camp, None, C.c_void_p(buf.ctypes.data + 4), None) == -1 and b"rt_object_extents_multi" in err() and b"8-byte aligned" in err()


# ---- the build's report ------------------------------------------------------------------------------------------------------------------
def test_build_report_lists_the_new_kernels_without_spill_or_private_segment():
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    lines = [l.rstrip() for l in open(report).read().splitlines() if l.startswith("rt_planes.o")]
    assert sum("assemble_planes_kerne" in l for l in lines) == 3 and sum("merge_extents_kernel" in l for l in lines) == 1, lines   # 4-, 8-, 16-byte elements
    for l in lines:
        assert re.search(r"SGPR spills +0 +VGPR spills +0 +scratch 0$", l), l
    make = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "Makefile")).read()
    rule = re.search(r"^(\$\(BUILD\)/csrc/rt_resolve\.o[^\n:]*):[^\n]*\n((?:\t[^\n]*\n)+)", make, flags=re.M)
    assert "$(BUILD)/csrc/rt_planes.o" in rule.group(1) and "-ffp-contract=off" in rule.group(2)   # built once, without contraction
    src = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc", "rt_planes.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "__shared__" not in code and "atomic" not in code and not re.search(r"\b(float|double)\b", code)
