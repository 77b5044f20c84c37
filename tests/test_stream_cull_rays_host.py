"""Culled ray queries (RT_FLAG_STREAM_CULL_RAYS, csrc/rt_stream_cull_rays.hip), host side: the ABI constant and
symbols, what the entry points answer before they look for a device, the build report's lines for the new kernels, the files the feature
must leave alone, the per-ray predicate asked about chunk bounds for the rays a caller can hand in (tests/tools/ray_cull_lab.py), and the
condition that keeps the GPU statistics test from being vacuous."""
import ctypes as C
import functools
import hashlib
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

CSRC = os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")
N_VERDICTS = 20000   # per family here, a few seconds in all; the full count (100 000 per family) is the lab's main: python tests/tools/ray_cull_lab.py
NEW_FILES = ("rt_stream_cull_rays.hpp", "rt_stream_cull_rays.hip")
KERNELS = {"ray_query_cull_kernel": 8, "shade_rays_cull_kernel": 4, "path_query_cull_kernel": 4}   # instantiations per build
LAUNCHERS = ("rt_launch_stream_cull_trace_rays", "rt_launch_stream_cull_occluded_rays", "rt_launch_stream_cull_shade_rays", "rt_launch_stream_cull_trace_paths")
# the files the feature calls into or stands beside, as they were before it (sha256)
UNTOUCHED = {"rt_stream_cull_bounce.hpp": "f4f6b3c4d618b80feda7186228001dad1adc4eabb48d844fcc57158034ac5c8e",
             "rt_ray_bound.hpp": "32c17c9aa85ae82b2add30121c1149e19d87f38e81a145cc2354c45140e0df4c"}


@pytest.fixture(autouse=True)
def the_feature(pkg):
    """Everything here is about the feature."""
    assert pkg.RT_FLAG_STREAM_CULL_RAYS == 2097152


@functools.lru_cache(maxsize=None)
def lab():
    import ray_cull_lab as RL
    RL.build()
    return RL


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_flag_in_header_and_binding(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"#define RT_FLAG_STREAM_CULL_RAYS 2097152u\b", hdr) and "#define RT_ABI_VERSION 3" in hdr
    assert pkg.RT_FLAG_STREAM_CULL_RAYS == 2097152 == 0x200000 == 2 * pkg.RT_FLAG_STREAM_CULL_BOUNCE
    names = set(re.findall(r"#define (RT_FLAG_\w+|RT_MULTI_\w+) (?:0x[0-9a-fA-F]+|\d+)u\b", hdr))
    assert {"RT_FLAG_STREAM", "RT_FLAG_STREAM_QUERIES", "RT_FLAG_STREAM_CULL", "RT_FLAG_STREAM_CULL_BOUNCE", "RT_FLAG_STREAM_CULL_RAYS", "RT_MULTI_SELF_EXCHANGE",
            "RT_MULTI_BANDWISE", "RT_MULTI_SPARSE"} <= names
    for name in names - {"RT_FLAG_STREAM_CULL_RAYS"}:
        assert not (getattr(pkg, name) & pkg.RT_FLAG_STREAM_CULL_RAYS), name


def test_symbols_and_prototypes(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"\bint rt_get_stream_cull_rays\(const rt_ctx \*ctx, uint32_t \*on\);", hdr)
    assert re.search(r"\bint rt_debug_stream_cull_rays\(rt_ctx \*ctx, uint64_t out\[8\]\);", hdr)
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("rt_get_stream_cull_rays", "rt_debug_stream_cull_rays") + tuple(f"{l}_{v}" for l in LAUNCHERS for v in ("strict", "fast")):
        assert re.search(rf"\bT {sym}\b", names), sym
        assert sym.startswith("rt_launch") or sym in pkg.ABI_SYMBOLS, sym
    lib = pkg.lib()
    assert lib.rt_get_stream_cull_rays.argtypes[1] == C.POINTER(C.c_uint32)
    assert lib.rt_debug_stream_cull_rays.argtypes[1] == C.POINTER(C.c_uint64)
    assert isinstance(pkg.Renderer.stream_cull_rays, property) and callable(pkg.Renderer.stream_cull_rays_stats)
    assert isinstance(pkg.MultiRenderer.stream_cull_rays, property)
    # declared once through RT_PER_VARIANT, with its query's one signature (the chunks in one record), and named by one slot of the launcher
    # table: the culled path's, under its own query (tests/tools/launch_table.py)
    import launch_table as LT
    launch = open(os.path.join(CSRC, "rt_launch.h")).read()
    for l in LAUNCHERS:
        assert len(re.findall(rf"RT_PER_VARIANT\(hipError_t, {l},", launch)) == 1, l
        assert LT.declared()[l].endswith(", const ChunkTables *chunks, hipStream_t stream") and "n_chunks" not in LT.declared()[l], l
        assert LT.declared()[l] == LT.declared()[l.replace("stream_cull_", "")], l      # the staged twin's
        assert LT.slot_of(l) == f"query[PATH_CULLED].{l[len('rt_launch_stream_cull_'):]}", l
    # the update.h adapter reads MI355RT_STREAM_CULL_RAYS
    assert b"MI355RT_STREAM_CULL_RAYS" in open(pkg.UPDATE_LIB_PATH, "rb").read()


def test_null_arguments_are_refused_before_a_device_is_looked_for(pkg):
    lib = pkg.lib()
    n, words = C.c_uint32(7), (C.c_uint64 * 8)(*([9] * 8))
    assert lib.rt_get_stream_cull_rays(None, C.byref(n)) == -1 and lib.rt_last_error() == b"rt_get_stream_cull_rays: null argument" and n.value == 7
    assert lib.rt_debug_stream_cull_rays(None, words) == -1 and b"rt_debug_stream_cull_rays: null argument" in lib.rt_last_error()
    assert list(words) == [9] * 8


def _create_rc(pkg, flags, name="quadratic"):
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(64, 48)
    d = sc.desc()
    cfg = pkg.Config(-1, 0, 1, 8, int(flags), pkg.RT_FMT_RGBA32F)
    ctx = C.c_void_p()
    rc = pkg.lib().rt_create(C.byref(ctx), C.byref(d), C.byref(cfg))
    if rc == 0:
        pkg.lib().rt_destroy(ctx)
    return rc, pkg.lib().rt_last_error().decode()


def test_the_flag_gets_past_the_create_checks_alone_and_with_every_other_flag(pkg):
    """No refusal of its own: alone, with the flags its decision reads, and with each other flag (and what that flag needs beside it)
    rt_create gets as far as the device query."""
    import torch
    f = pkg
    others = [0, f.RT_FLAG_FAST, f.RT_FLAG_COUNT, f.RT_FLAG_SIMPLE, f.RT_FLAG_NOCULL, f.RT_FLAG_STATIC_ORDER, f.RT_FLAG_NOSCAN, f.RT_FLAG_PLAIN_ORDER, f.RT_FLAG_NOSPLIT,
              f.RT_FLAG_NOLEAN, f.RT_FLAG_SSAA2, f.RT_FLAG_SSAA4, f.RT_FLAG_SSAA2 | f.RT_FLAG_SSAA_ADAPTIVE, f.RT_FLAG_SSAA4 | f.RT_FLAG_SSAA_ADAPTIVE | f.RT_FLAG_SSAA_GEOMETRY,
              f.RT_FLAG_STREAM, f.RT_FLAG_STREAM_QUERIES, f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_QUERIES, f.RT_FLAG_STREAM_CULL_BOUNCE,
              f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_QUERIES | f.RT_FLAG_STREAM_CULL_BOUNCE,
              f.RT_FLAG_STREAM | f.RT_FLAG_SSAA2 | f.RT_FLAG_SSAA_ADAPTIVE | f.RT_FLAG_STREAM_ADAPTIVE]
    for extra in others:
        for cull in (0, f.RT_FLAG_STREAM_CULL):
            with_flag, without = _create_rc(pkg, f.RT_FLAG_STREAM_CULL_RAYS | cull | extra), _create_rc(pkg, cull | extra)
            assert with_flag[0] == without[0], (extra, cull, with_flag, without)      # no refusal of its own: whatever the other flags get
            assert with_flag[0] in (0, -4), (extra, cull, with_flag)
            if not torch.cuda.is_available():
                assert with_flag[0] == -4, (extra, cull, with_flag)


# ---- the build --------------------------------------------------------------------------------------------------------------------------
def test_build_report_lists_the_new_kernels_without_spills():
    """Every instantiation of both builds -- <HAS_GQ, HAS_CUBIC> of the colour and the path kernel, <HAS_GQ, HAS_CUBIC, OCCLUSION> of the ray
    kernel --: none spills, none has a private segment, each runs at least two waves per SIMD (the ray kernels three).  No scene is
    excluded from the decision, so all sixteen must be there."""
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    text = open(report).read().splitlines()
    for variant in ("strict", "fast"):
        mine = [l for l in text if l.startswith(f"rt_stream_cull_rays_{variant}.o")]
        assert len(mine) == sum(KERNELS.values()), mine
        for l in mine:
            assert re.search(r"VGPR spills\s+0\s+scratch 0\b", l), l
            assert int(re.search(r"occupancy (\d+)\b", l).group(1)) >= 2, l
            assert int(re.search(r"VGPRs\s+(\d+)", l).group(1)) <= 256, l
        remarks = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "csrc", f"rt_stream_cull_rays_{variant}.o.remarks")).read()
        for kernel, count in KERNELS.items():      # ... and the full names, from the compiler's own remarks
            assert len(set(re.findall(rf"Function Name: (\S*{kernel}\S*)", remarks))) == count, (variant, kernel)
    # the twins' file keeps its own lines
    assert len([l for l in text if l.startswith("rt_stream_queries_strict.o")]) == len([l for l in text if l.startswith("rt_stream_queries_fast.o")]) > 16


def test_the_new_files_have_no_workgroup_barrier():
    for name in NEW_FILES:
        text = open(os.path.join(CSRC, name)).read()
        code = "\n".join(l.split("//")[0] for l in text.splitlines())
        assert "__syncthreads" not in code and "s_barrier" not in code and '"workgroup"' not in code and "rq_stage_tables" not in code, name
        assert "extern __shared__" not in code and "HIP_DYNAMIC_SHARED" not in code, name
        assert "__shared__" not in code or name.endswith(".hip"), name      # (nothing of the bounds goes to LDS: only the kernels' own slices)
    query = open(os.path.join(CSRC, "rt_stream_cull_rays.hpp")).read()
    assert "sq_stage_chunk" in query and "sc_sweep<OCCLUSION>" in query and "ray_reaches" in query and "rq_plain<OCCLUSION>" in query
    body = "\n".join(l.split("//")[0] for l in query.splitlines())
    assert "const RayBound rb = scr_ray_bound(o, d);" in body and "return ray_bound(o, dq);" in body and 'asm volatile("" : "+v"(dq.x), "+v"(dq.y), "+v"(dq.z));' in body      # one loop, the bound from the opaque direction
    assert "sc_query_bounce" not in body      # (see the head of that file: the contracted build)
    kernel = open(os.path.join(CSRC, "rt_stream_cull_rays.hip")).read()
    code = "\n".join(l.split("//")[0] for l in kernel.splitlines())
    assert "sq_query<" not in code      # no instantiation keeps the full sweep
    assert code.count("__shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];") == 3
    # every kernel's query object is the one over sc_query_ray, on the wave's own slice, and its work words leave through sc_flush
    assert code.count("smem + (threadIdx.x >> 6) * SQ_SLICE_BYTES, {false, {0u, 0u, 0u, 0u, 0u}}};") == 3 == len(re.findall(r"\bScRayQuery q\{(qa|sa\.qa|pa\.qa), ca, scene, ", code))
    assert code.count("if (ca.stats) sc_flush(q.bs.w, ca.stats, threadIdx.x & 63u);") == 3 and "atomicAdd" not in code
    obj = body.split("struct ScRayQuery {")[1].split("\n};\n")[0]
    assert "bs.on = ca.stats != nullptr && __ballot(use) != 0ull;" in obj and obj.count("sc_query_ray<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, ca, scene, slice, lane, o, d, use, t_max, best_t, best, bs);") == 1
    assert body.count("sc_query_ray<") == 1 and "const StreamCullArgs &ca;" in obj and "const RayQueryArgs &qa;" in obj      # (the kernel's own arguments: DESIGN.md section 30, "Shapes")
    # the shading loop is the shared one, under the one policy over a query object (rt_ray_kernels.hpp), which this file's colour kernel runs
    bodies = "\n".join(l.split("//")[0] for l in open(os.path.join(CSRC, "rt_ray_kernels.hpp")).read().splitlines())
    assert "RkShade<Query> pol{q, out_rec, i, live};" in bodies and "shade_loop<HAS_GQ, HAS_CUBIC>(sa, scene, lights, lane, pol, o, d, live)" in bodies
    assert "rk_shade_rays<HAS_GQ, HAS_CUBIC>(sa, scene, lights, rays, out_rgba, out_rec, q);" in code.split("void shade_rays_cull_kernel(")[1].split("\n}\n")[0]
    assert "sq_query<" not in bodies and "sc_query_ray" not in bodies      # the bodies know no family


def test_the_neighbours_are_untouched():
    """rt_stream_cull_bounce.hpp (the nearest-hit query this feature calls) and rt_ray_bound.hpp (the predicate) are what they were before
    the feature.  rt_stream_queries.hip (the twins) was pinned too while this feature's kernels restated its ray loader, grid and bodies; now
    there is no copy to keep in step: this feature's kernels run the bodies of rt_ray_kernels.hpp, as the twins do
    (but for the one that keeps the path body's text, held to it line by line), and this feature's files hold no ray load, grid rule,
    record store or loop of their own (tests/test_stream_shade_host.py says so of all five kernel files).  The twins still know nothing of
    culling."""
    for name, digest in UNTOUCHED.items():
        assert hashlib.sha256(open(os.path.join(CSRC, name), "rb").read()).hexdigest() == digest, name
    twin = open(os.path.join(CSRC, "rt_stream_queries.hip")).read()
    assert "rt_stream_cull" not in twin and "ray_reaches" not in twin
    import test_stream_shade_host as shared
    shared.test_the_ray_kernels_bodies_exist_once()
    shared.test_the_path_kernel_that_keeps_its_copy_is_the_bodys_text()
    for name in NEW_FILES:
        code = "\n".join(l.split("//")[0] for l in open(os.path.join(CSRC, name)).read().splitlines())
        for word in ("double2", "rq_store_record", "normal_vector", "reflect_ray", "__ballot(bouncing)", "max_grid ?", "gridDim"):
            assert word not in code, (name, word)


def test_the_launch_sites_pick_by_the_one_decision():
    capi = open(os.path.join(CSRC, "rt_capi.cpp")).read()
    assert ("cull[CULL_RAYS] = (ctx->cfg.flags & RT_FLAG_STREAM_CULL_RAYS) && cull[CULL_FRAME] && ctx->stream_queries && ctx->n_chunks >= 2u;") in capi
    assert capi.count("cull[CULL_RAYS] =") == 1
    # ... which picks the launchers once, for the context's life
    assert capi.count("ctx->ray_q = &ctx->kern->query[cull[CULL_RAYS] ? PATH_CULLED : plain];") == 1 == capi.count("ctx->ray_q =")
    assert "const TablePath plain = ctx->stream_queries ? PATH_STREAMED : PATH_STAGED;" in capi
    for name in ("trace_rays", "occluded_rays", "shade_rays", "trace_paths"):      # one site each (three behind trace_launch / shade_launch / paths_launch), with the family's chunks
        assert len(re.findall(rf"ctx->ray_q->{name}\([^\n]*, &ctx->chunks\[CULL_RAYS\], stream\);", capi)) == 1 == len(re.findall(rf"->{name}\(", capi)), name
    for name in ("gbuffer", "pick", "object_extents"):      # the pixel queries keep theirs
        assert f"ray_q->{name}" not in capi and len(re.findall(rf"{name}\([^\n]*CULL_RAYS", capi)) == 0, name


# ---- the predicate, asked about bounds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["far", "inside_member", "behind_near", "occlusion"])
def test_a_skipped_bound_has_no_member_the_oracle_accepts(family):
    """ray_reaches says "skip" => orc_intersect_ray gives no member a root with t >= EPS && t < MAX_T; for `occlusion`, none with t > EPS &&
    t < t_max, t_max at 0.9 ... 1.1 of the grazed member's root (one ulp either side, +inf and NaN among them).  Zero unsound in the strict
    and in the contracted build; an origin inside the bound always reaches it; two runs agree."""
    RL = lab()
    row = RL.run_family(family, N_VERDICTS)
    print(RL.format_row(row))
    assert row["cases"] >= N_VERDICTS and row["unsound"] == 0, row
    assert row["origin_inside_skipped"] == 0 and row["repeat_differs"] == 0, row
    assert 0 < row["accepted"] < row["cases"], row
    if RL.B.host_has_fma():
        assert row["fast_cases"] == row["cases"] and row["fast_unsound"] == 0, row
    if family == "inside_member":
        assert row["culled"] == 0, row       # (the bound holds the origin: such a ray is never culled for)
    else:
        assert row["culled"] > 0, row
    if family == "occlusion":
        assert row["limited"] > 0, row       # (t_max did cut roots the half-line has: the family is about something)


# ---- the statistics scene ---------------------------------------------------------------------------------------------------------------
def test_statistics_scene_is_not_vacuous(pkg):
    """The scene of tests/test_stream_cull_rays_gpu.py::test_statistics: bounce_cull_lab's 320 clustered spheres (5 chunks), 64 x 48, its own
    primary rays in row order as caller-supplied rays, a wave being 64 consecutive rays.  D = (wave, chunk) pairs, L = the pairs no lane's
    half-line comes within 1.01 r + 0.1 of; L >= D / 2.  8 x 8 block order leaves more, a shuffle next to nothing: the chunk level works
    on a wave's union."""
    e = lab().expectation("row")
    print({k: v for k, v in e.items() if k != "rays"})
    assert e["n_chunks"] == 5 and e["waves"] == 48 and e["D"] == 240 and len(e["rays"]) == 64 * 48
    assert e["L"] >= e["D"] / 2, e["L"]
    assert e["L"] == 184       # (the figure the GPU test's bound was set with)
    block, shuffled = lab().expectation("block"), lab().expectation("shuffled")
    assert block["D"] == shuffled["D"] == 240 and block["L"] > e["L"] > 2 * shuffled["L"], (block["L"], shuffled["L"])
