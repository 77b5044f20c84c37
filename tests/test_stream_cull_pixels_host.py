"""Culled pixel queries (RT_FLAG_STREAM_CULL_PIXELS, csrc/rt_stream_cull_pixels.hip), host side: the ABI constant
and symbols, what the entry points answer before they look for a device, the build report's lines for the new kernels, the shape of the
new files, the launch sites, and the condition that keeps the GPU statistics test from being vacuous (tests/tools/pixel_cull_lab.py)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

CSRC = os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")
NEW_FILES = ("rt_stream_cull_pixels.hpp", "rt_stream_cull_pixels.hip")
KERNELS = {"gbuffer_cull_kernel": 4, "extents_cull_kernel": 4}   # instantiations per build
LAUNCHERS = ("rt_launch_pixel_cull_gbuffer", "rt_launch_pixel_cull_pick", "rt_launch_pixel_cull_object_extents")
DECISION = "cull[CULL_PIXELS] = (ctx->cfg.flags & RT_FLAG_STREAM_CULL_PIXELS) && cull[CULL_FRAME] && ctx->stream_queries && ctx->n_chunks >= 2u;"


@pytest.fixture(autouse=True)
def the_feature(pkg):
    """Everything here is about the feature."""
    assert pkg.RT_FLAG_STREAM_CULL_PIXELS == 4194304


def code_of(name):
    return "\n".join(l.split("//")[0] for l in open(os.path.join(CSRC, name)).read().splitlines())


@functools.lru_cache(maxsize=None)
def lab():
    import pixel_cull_lab as PL
    PL.SC.build()
    return PL


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_flag_in_header_and_binding(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"#define RT_FLAG_STREAM_CULL_PIXELS 4194304u\b", hdr) and "#define RT_ABI_VERSION 3" in hdr
    assert pkg.RT_FLAG_STREAM_CULL_PIXELS == 4194304 == 0x400000 == 2 * pkg.RT_FLAG_STREAM_CULL_RAYS
    names = set(re.findall(r"#define (RT_FLAG_\w+|RT_MULTI_\w+) (?:0x[0-9a-fA-F]+|\d+)u\b", hdr))
    assert {"RT_FLAG_STREAM", "RT_FLAG_STREAM_QUERIES", "RT_FLAG_STREAM_CULL", "RT_FLAG_STREAM_CULL_RAYS", "RT_FLAG_STREAM_CULL_PIXELS"} <= names
    for name in names - {"RT_FLAG_STREAM_CULL_PIXELS"}:
        assert not (getattr(pkg, name) & pkg.RT_FLAG_STREAM_CULL_PIXELS), name
    # the header's comment: the decision, what is and is not culled, the results, the limits, what is out of scope
    text = hdr.split("/* Culled pixel queries (DESIGN.md section 34")[1].split("#define RT_FLAG_STREAM_CULL_PIXELS")[0]
    for word in ("stream cull pixels = RT_FLAG_STREAM_CULL_PIXELS && rt_get_stream_cull && rt_get_streamed_queries && at least 2 chunks", "Not culled:",
                 "Results are unchanged by definition", "Known limits:", "Out of scope:", "picks gain nothing", "the G pass of an RT_FLAG_SSAA_GEOMETRY frame"):
        assert word in text, word
    # ... and the lists it closes no longer name the pixel queries as unculled
    assert "culling in the streamed pixel queries" not in hdr and "Out of scope: the pixel queries" not in hdr
    assert "not by identity of kernel" in hdr


def test_symbols_and_prototypes(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"\bint rt_get_stream_cull_pixels\(const rt_ctx \*ctx, uint32_t \*on\);", hdr)
    assert re.search(r"\bint rt_debug_stream_cull_pixels\(rt_ctx \*ctx, uint64_t out\[8\]\);", hdr)
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("rt_get_stream_cull_pixels", "rt_debug_stream_cull_pixels") + tuple(f"{l}_{v}" for l in LAUNCHERS for v in ("strict", "fast")):
        assert re.search(rf"\bT {sym}\b", names), sym
        assert sym.startswith("rt_launch") or sym in pkg.ABI_SYMBOLS, sym
    lib = pkg.lib()
    assert lib.rt_get_stream_cull_pixels.argtypes[1] == C.POINTER(C.c_uint32)
    assert lib.rt_debug_stream_cull_pixels.argtypes[1] == C.POINTER(C.c_uint64)
    assert isinstance(pkg.Renderer.stream_cull_pixels, property) and callable(pkg.Renderer.stream_cull_pixels_stats)
    assert isinstance(pkg.MultiRenderer.stream_cull_pixels, property)
    # declared once through RT_PER_VARIANT, with its query's one signature (the chunks in one record), and named by one slot of the launcher
    # table: the culled path's, under its own query (tests/tools/launch_table.py)
    import launch_table as LT
    launch = open(os.path.join(CSRC, "rt_launch.h")).read()
    for l in LAUNCHERS:
        assert len(re.findall(rf"RT_PER_VARIANT\(hipError_t, {l},", launch)) == 1, l
        assert LT.declared()[l].endswith(", const ChunkTables *chunks, hipStream_t stream") and "n_chunks" not in LT.declared()[l], l
        assert LT.declared()[l] == LT.declared()[l.replace("pixel_cull_", "")], l      # the staged twin's
        assert LT.slot_of(l) == f"query[PATH_CULLED].{l[len('rt_launch_pixel_cull_'):]}", l
    # the update.h adapter reads MI355RT_STREAM_CULL_PIXELS
    assert b"MI355RT_STREAM_CULL_PIXELS" in open(pkg.UPDATE_LIB_PATH, "rb").read()


def test_null_arguments_are_refused_before_a_device_is_looked_for(pkg):
    lib = pkg.lib()
    n, words = C.c_uint32(7), (C.c_uint64 * 8)(*([9] * 8))
    assert lib.rt_get_stream_cull_pixels(None, C.byref(n)) == -1 and lib.rt_last_error() == b"rt_get_stream_cull_pixels: null argument" and n.value == 7
    assert lib.rt_debug_stream_cull_pixels(None, words) == -1 and b"rt_debug_stream_cull_pixels: null argument" in lib.rt_last_error()
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
    rt_create answers what the same flags get without it -- without a GPU, that no device was found."""
    import torch
    f = pkg
    others = [0, f.RT_FLAG_FAST, f.RT_FLAG_COUNT, f.RT_FLAG_SIMPLE, f.RT_FLAG_NOCULL, f.RT_FLAG_STATIC_ORDER, f.RT_FLAG_NOSCAN, f.RT_FLAG_PLAIN_ORDER, f.RT_FLAG_NOSPLIT,
              f.RT_FLAG_NOLEAN, f.RT_FLAG_SSAA2, f.RT_FLAG_SSAA4, f.RT_FLAG_SSAA2 | f.RT_FLAG_SSAA_ADAPTIVE, f.RT_FLAG_SSAA4 | f.RT_FLAG_SSAA_ADAPTIVE | f.RT_FLAG_SSAA_GEOMETRY,
              f.RT_FLAG_STREAM, f.RT_FLAG_STREAM_QUERIES, f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_QUERIES, f.RT_FLAG_STREAM_CULL_BOUNCE, f.RT_FLAG_STREAM_CULL_RAYS,
              f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_QUERIES | f.RT_FLAG_STREAM_CULL_BOUNCE | f.RT_FLAG_STREAM_CULL_RAYS,
              f.RT_FLAG_STREAM | f.RT_FLAG_SSAA2 | f.RT_FLAG_SSAA_ADAPTIVE | f.RT_FLAG_STREAM_ADAPTIVE]
    for extra in others:
        for cull in (0, f.RT_FLAG_STREAM_CULL):
            with_flag, without = _create_rc(pkg, f.RT_FLAG_STREAM_CULL_PIXELS | cull | extra), _create_rc(pkg, cull | extra)
            assert with_flag[0] == without[0], (extra, cull, with_flag, without)      # no refusal of its own: whatever the other flags get
            assert with_flag[0] in (0, -4), (extra, cull, with_flag)
            if not torch.cuda.is_available():
                assert with_flag[0] == -4, (extra, cull, with_flag)


# ---- the build --------------------------------------------------------------------------------------------------------------------------
def test_build_report_lists_the_new_kernels_without_spills():
    """Every instantiation <HAS_GQ, HAS_CUBIC> of both kernels in both builds: none spills, none has a private segment, each runs at least
    two waves per SIMD.  No scene is excluded from the decision, so all eight must be there."""
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    text = open(report).read().splitlines()
    for variant in ("strict", "fast"):
        mine = [l for l in text if l.startswith(f"rt_stream_cull_pixels_{variant}.o") and "ext_identities_cull_ker" not in l]
        assert len(mine) == sum(KERNELS.values()) == 8, mine
        for l in mine:
            assert re.search(r"VGPR spills\s+0\s+scratch 0\b", l), l
            assert int(re.search(r"occupancy (\d+)\b", l).group(1)) >= 2, l
            assert int(re.search(r"VGPRs\s+(\d+)", l).group(1)) <= 256, l
        remarks = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "csrc", f"rt_stream_cull_pixels_{variant}.o.remarks")).read()
        for kernel, count in KERNELS.items():      # ... and the full names, from the compiler's own remarks
            assert len(set(re.findall(rf"Function Name: (\S*{kernel}\S*)", remarks))) == count, (variant, kernel)
        assert len(set(re.findall(r"Function Name: (\S*ext_identities_cull_kernel\S*)", remarks))) == 1
    # the twins' file keeps its own lines
    assert len([l for l in text if l.startswith("rt_stream_queries_strict.o")]) == len([l for l in text if l.startswith("rt_stream_queries_fast.o")]) > 16


def test_the_new_files_have_no_workgroup_barrier_and_one_body_each():
    for name in NEW_FILES:
        code = code_of(name)
        assert "__syncthreads" not in code and "s_barrier" not in code and '"workgroup"' not in code and "rq_stage_tables" not in code, name
        assert "extern __shared__" not in code and "HIP_DYNAMIC_SHARED" not in code, name
        assert "__shared__" not in code or name.endswith(".hip"), name      # (nothing of the bounds goes to LDS: only the kernels' own slices)
        assert "extents_init" not in code and "EXT_INIT_KERNEL" not in code and "mono_set_" not in code and "rq_mono" not in code, name
    kernel = code_of("rt_stream_cull_pixels.hip")
    assert kernel.count("__shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];") == 2 == kernel.count("__shared__")
    assert len(re.findall(r"\bpk_gbuffer<", kernel)) == 1 and len(re.findall(r"\bpk_extents<", kernel)) == 1
    assert "sq_tables" not in kernel and "nearest" not in kernel and "#define" not in kernel and "atomicAdd" not in kernel
    for name, body_fn in (("gbuffer_cull_kernel", "pk_gbuffer"), ("extents_cull_kernel", "pk_extents")):
        body = kernel.split(f"void {name}(")[1].split("\n}\n")[0]
        assert len(re.findall(r"\bScPixels q\{fa, qa, ca, scene, smem \+ \(threadIdx\.x >> 6\) \* SQ_SLICE_BYTES, ps\};", body)) == 1 == len(re.findall(r"\bScPixels q\b", body)), name
        assert len(re.findall(rf"\b{body_fn}<HAS_GQ, HAS_CUBIC>\(", body)) == 1 == len(re.findall(r"\bpk_\w+<", body)), name
        assert "for (" not in body and "while (" not in body, name
        assert body.count("if (ca.stats) sc_flush(ps.w, ca.stats, threadIdx.x & 63u);") == 1, name
    assert len(re.findall(r"\bRK_LAUNCH\(fa, \((gbuffer|extents)_cull_kernel<GQ, CUB>\)", kernel)) == 2 and "rq_for_classes" not in kernel
    ident = kernel.split("void ext_identities_cull_kernel(")[1].split("\n}\n")[0]
    assert ident.count("ext_identity()") == 1 and ident.count(";") == 1      # one line of body
    # the query object: one call, the caller's monomials, SqPixels' cone and SqPixels' form of the other tables
    query = code_of("rt_stream_cull_pixels.hpp")
    obj = query.split("struct ScPixels {")[1].split("\n};\n")[0]
    assert obj.count("__device__") == 1 and "template <bool HAS_GQ, bool HAS_CUBIC>\n" in obj
    assert "void nearest(uint32_t lane, const Mono &m, bool live, bool block, double &best_t, int &best) const" in obj
    assert "sq_pixel_cone(fa.cull != 0u, block, m.d)" in obj and "rq_plain" not in obj and "sq_query" not in obj and "sc_query_primary" not in obj
    assert obj.count("sc_load_bound(ca, g, lane)") == 1 and obj.count("sq_stage_chunk(g_us, base, end, lane, slice)") == 1 and obj.count("sc_sweep<false>(") == 1
    assert obj.count("sphere_in_cone(") == 2
    assert obj.count("sq_tables<HAS_GQ, HAS_CUBIC, false, true>(rest, scene, slice, lane, m, live, cone, MAX_T, best_t, best, &fa);") == 1 and "rest.n_us = 0u;" in obj
    assert sorted(n for n in os.listdir(CSRC) if re.search(r"\bstruct ScPixels\b", code_of(n))) == ["rt_stream_cull_pixels.hpp"]


def test_the_launch_sites_pick_by_the_one_decision():
    capi = open(os.path.join(CSRC, "rt_capi.cpp")).read()
    assert DECISION in capi and capi.count("cull[CULL_PIXELS] =") == 1
    # ... which picks the launchers once, for the context's life: the culled ones by the decision, else the ones as before
    assert capi.count("ctx->pixel_q = &ctx->kern->query[cull[CULL_PIXELS] ? PATH_CULLED : plain];") == 1 == capi.count("ctx->pixel_q =")
    assert "const TablePath plain = ctx->stream_queries ? PATH_STREAMED : PATH_STAGED;" in capi
    # rt_render_gbuffer, rt_pick, and rt_object_extents and rt_object_extents_host through their one helper: one site each, with the family's chunks
    for name in ("gbuffer", "pick", "object_extents"):
        assert len(re.findall(rf"ctx->pixel_q->{name}\([^\n]*, &ctx->chunks\[CULL_PIXELS\], stream\);", capi)) == 1 == len(re.findall(rf"pixel_q->{name}\(", capi)), name
    assert capi.count("extents_launch(") == 3 and all(f'extents_launch("{who}", ctx, fa, r, ' in capi for who in ("rt_object_extents", "rt_object_extents_host"))
    # the work words: only under the environment switch and a true decision -- one allocation for all families, a family's eight where it culls
    assert re.search(r'if \(e && !std::strcmp\(e, "1"\)\)\n\s*if \(int rc = device_table\(ctx->d_cull_words, nullptr, sizeof\(unsigned long long\) \* 8 \* N_CULL_FAMILIES,', capi)
    assert "const bool words = ctx->d_cull_words && !(f == CULL_ADAPTIVE && fa.n_gq && fa.n_cub);" in capi
    assert "if (ctx->cull[f]) ctx->chunks[f] = ChunkTables{ctx->d_bounds.p, ctx->n_chunks, words ? ctx->d_cull_words + 8 * f : nullptr};" in capi
    assert capi.count("ctx->chunks[f] =") == 1 and len(re.findall(r"ctx->chunks\[\w+\](\.\w+)? =[^=]", capi)) == 1 and capi.count("d_cull_words.alloc") == 0
    # the G pass of an adaptive frame keeps the streamed kernels: it names its path itself
    g = capi.split("if (ctx->geometry) {")[1].split("RT_HIP(rt_launch_classify_geometry_strict(")[0]
    assert "pixel_q" not in g and "PATH_CULLED" not in g and "CULL_PIXELS" not in g
    assert "const QueryLaunchers &g = ctx->kern->query[ctx->stream_adaptive ? PATH_STREAMED : PATH_STAGED];" in g and g.count("g.gbuffer(") == 1 == g.count("g.pick(")


def test_the_docs_name_the_flag():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"^## 34\. ", design, re.M) and "RT_FLAG_STREAM_CULL_PIXELS" in design.split("## 34. ")[1]
    assert "RT_FLAG_STREAM_CULL_PIXELS" in readme and "test_stream_cull_pixels_gpu.py" in readme and "The pixel queries are not culled." not in readme
    assert "MI355RT_STREAM_CULL_PIXELS" in integ


# ---- the statistics scene ---------------------------------------------------------------------------------------------------------------
def test_statistics_scene_is_not_vacuous(pkg):
    """The scene of tests/test_stream_cull_pixels_gpu.py::test_statistics: stream_cull_lab's 320 clustered spheres (5 chunks), 64 x 48, 48
    blocks.  sphere_in_cone, restated in numpy and compiled for the host (they agree), asked about every (block, chunk bound): the cone
    skips at least a quarter of the pairs.  A condition on the inputs, not a measurement."""
    PL = lab()
    e = PL.expectation(pkg, PL.SC.cluster_scene(pkg))
    print(e)
    assert e["blocks"] == 48 and e["n_chunks"] == 5 and e["D"] == 240 and e["staged"] + e["skipped"] == e["D"]
    assert e["skipped"] >= (48 * e["n_chunks"]) / 4, e
    assert e["skipped"] == 211       # (the figure DESIGN.md section 34 quotes)
