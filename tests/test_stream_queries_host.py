"""The streamed query kernels (RT_FLAG_STREAM_QUERIES, csrc/rt_stream_queries.hip), host side: the ABI constant and
symbol, the NULL refusals before a device is looked for, the build report's lines for the new kernels, and -- on the composers alone --
the conditions that keep the GPU tests (tests/test_stream_queries_gpu.py) from being vacuous for the three scenes beyond the limit
(tests/tools/stream_query_scenes.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gbuffer_ref  # noqa: E402
import launch_table as LT  # noqa: E402
import query_table_scenes as Q  # noqa: E402
import stream_query_scenes as B  # noqa: E402
import stream_scenes as S  # noqa: E402
from test_query_tables_host import check_aimed_rays_own_their_targets, check_occlusion_spans_the_chunks, last_chunks  # noqa: E402

CSRC = os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")
LAUNCHERS = ("gbuffer", "pick", "object_extents", "trace_rays", "occluded_rays", "shade_rays", "trace_paths")


def header():
    return open(os.path.join(ROOT, "include", "mi355rt.h")).read()


def test_flag_in_header_and_binding(pkg):
    hdr = header()
    assert re.search(r"#define RT_FLAG_STREAM_QUERIES 16384u\b", hdr) and "#define RT_ABI_VERSION 3" in hdr
    assert pkg.RT_FLAG_STREAM_QUERIES == 16384
    # disjoint from every other flag of rt_config.flags, the header's and the binding's
    flags = {name: int(value, 0) for name, value in re.findall(r"#define (RT_(?:FLAG|MULTI)_[A-Z0-9_]+) (\d+|0x[0-9a-fA-F]+)u\b", hdr)}
    assert len(flags) >= 19 and flags["RT_FLAG_STREAM_QUERIES"] == 16384
    for name, value in flags.items():
        assert getattr(pkg, name) == value, name
        assert name == "RT_FLAG_STREAM_QUERIES" or not (value & 16384), name
    # RT_ABI_DIAGNOSTIC has the same value, in another word: the version rt_abi_version returns
    assert re.search(r"#define RT_ABI_DIAGNOSTIC 0x4000\b", hdr) and "RT_ABI_DIAGNOSTIC" in hdr.split("#define RT_FLAG_STREAM_QUERIES")[0].rsplit("/*", 1)[1]
    assert pkg.lib().rt_abi_version() == 3


def test_symbols_and_prototypes(pkg):
    assert re.search(r"\bint rt_get_streamed_queries\(const rt_ctx \*ctx, uint32_t \*streamed\);", header())
    assert "rt_get_streamed_queries" in pkg.ABI_SYMBOLS
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    launch = open(os.path.join(CSRC, "rt_launch.h")).read()
    assert re.search(r"\bT rt_get_streamed_queries\b", names)
    for what in LAUNCHERS:
        for variant in ("strict", "fast"):
            assert re.search(rf"\bT rt_launch_stream_{what}_{variant}\b", names), (what, variant)
        # declared once for both variants, with the staged twin's type in the table the contexts call through
        # (the table: struct QueryLaunchers has one member per query, of the staged launcher's type, and the streamed path's slot names this launcher)
        assert re.search(rf"RT_PER_VARIANT\(hipError_t, rt_launch_stream_{what},", launch) and LT.members()[0][what] == f"rt_launch_{what}", what
        assert LT.declared()[f"rt_launch_stream_{what}"] == LT.declared()[f"rt_launch_{what}"], what
        assert LT.slot_of(f"rt_launch_stream_{what}") == f"query[PATH_STREAMED].{what}" and LT.slot_of(f"rt_launch_{what}") == f"query[PATH_STAGED].{what}", what
    lib = pkg.lib()
    assert lib.rt_get_streamed_queries.argtypes[1] == C.POINTER(C.c_uint32)
    assert isinstance(pkg.Renderer.streamed_queries, property)
    # null arguments need no device
    n = C.c_uint32(7)
    assert lib.rt_get_streamed_queries(None, C.byref(n)) == -1 and b"rt_get_streamed_queries: null argument" in lib.rt_last_error() and n.value == 7
    assert lib.rt_get_streamed_queries(C.c_void_p(16), None) == -1 and b"rt_get_streamed_queries: null argument" in lib.rt_last_error()
    # the update.h adapter reads MI355RT_STREAM_QUERIES
    assert b"MI355RT_STREAM_QUERIES" in open(pkg.UPDATE_LIB_PATH, "rb").read()


def test_the_flag_has_no_refusal_of_its_own(pkg):
    """With every flag that gets past rt_create's checks on its own, rt_create gets as far as the device query (or creates the context)."""
    import torch
    from conftest import scene_path
    for extra in (0, pkg.RT_FLAG_STREAM, pkg.RT_FLAG_SIMPLE, pkg.RT_FLAG_FAST | pkg.RT_FLAG_NOCULL, pkg.RT_FLAG_COUNT, pkg.RT_FLAG_SSAA2,
                  pkg.RT_FLAG_SSAA4 | pkg.RT_FLAG_SSAA_ADAPTIVE | pkg.RT_FLAG_SSAA_GEOMETRY):
        sc = pkg.Scene.load_from_file(scene_path("quadratic")).set_size(64, 48)
        d = sc.desc()
        cfg = pkg.Config(-1, 0, 1, 8, int(pkg.RT_FLAG_STREAM_QUERIES | extra), pkg.RT_FMT_RGBA32F)
        ctx = C.c_void_p()
        rc = pkg.lib().rt_create(C.byref(ctx), C.byref(d), C.byref(cfg))
        if rc == 0:
            pkg.lib().rt_destroy(ctx)
        assert rc in (0, -4) and (rc == -4 or torch.cuda.is_available()), (extra, rc, pkg.lib().rt_last_error())


def test_build_report_lists_the_new_kernels_without_spills():
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    text = open(report).read().splitlines()
    # <HAS_GQ, HAS_CUBIC> each; the ray-query kernel also <OCCLUSION>.  (The report keeps 40 characters of a mangled name: the first 20 of a
    # kernel's own name are in it for both variants, and tell the six kernels apart from each other and from their staged twins.)
    for kernel, count in (("gbuffer_stream_kernel", 4), ("extents_stream_kernel", 4), ("ray_query_stream_kernel", 8), ("shade_rays_stream_kernel", 4),
                          ("path_query_stream_kernel", 4), ("extents_init_stream_kernel", 1)):
        for variant in ("strict", "fast"):
            mine = [l for l in text if l.startswith(f"rt_stream_queries_{variant}.o") and re.search(rf"\d{kernel[:20]}", l)]
            assert len(mine) == count, (kernel, variant, mine)
            for l in mine:
                assert re.search(r"VGPR spills\s+0\s+scratch 0\b", l), l


def test_the_kernel_file_has_no_workgroup_barrier_and_no_dynamic_lds():
    for name in ("rt_stream_queries.hip", "rt_stream_shade.hpp", "rt_ray_kernels.hpp", "rt_pixel_kernels.hpp"):   # ... the shared loop of the colour kernel and the kernels' bodies included
        text = open(os.path.join(CSRC, name)).read()
        code = "\n".join(l.split("//")[0] for l in text.splitlines())
        assert "__syncthreads" not in code and "s_barrier" not in code and "rq_stage_tables" not in code and '"workgroup"' not in code, name
        assert "extern __shared__" not in code and "HIP_DYNAMIC_SHARED" not in code and "rq_plain" not in code, name
        assert "__shared__" not in code or name == "rt_stream_queries.hip", name      # (a body takes no LDS: its kernel does)
    text = open(os.path.join(CSRC, "rt_stream_queries.hip")).read()
    code = "\n".join(l.split("//")[0] for l in text.splitlines())
    assert code.count("__shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];") == 5
    # the pixel family goes through sq_tables itself (no plain path) -- in its one query object, SqPixels, next to the loop in rt_stream.hpp, with
    # the cone of the staged twin (sq_pixel_cone) and the host's degree-3 records (HOST_CUB) --, the ray families through sq_query: the ray-query
    # and the colour kernel through their bodies (rt_ray_kernels.hpp) over the one query object that calls it, without a cone (SqQuery, next to sq_query in
    # rt_stream.hpp: 1), the path kernel, which keeps its body's text, itself (1); the frame kernels' policy over
    # sq_query keeps its two calls (rt_stream_shade.hpp)
    assert "sq_tables" not in code and "sq_query<" not in code.split("void gbuffer_stream_kernel(")[1] and code.count("sq_query<") == 1
    assert len(re.findall(r"SqPixels q\{fa, qa, scene, smem \+ \(threadIdx\.x >> 6\) \* SQ_SLICE_BYTES\};", code.split("void gbuffer_stream_kernel(")[1])) == 2      # the wave's own slice
    assert "sq_query<HAS_GQ, HAS_CUBIC, false>(qa, scene, slice, lane, o, d, bouncing, false, MAX_T, best_t, best);" in code.split("void path_query_stream_kernel")[1].split("// ---- pixels")[0]
    shade = "\n".join(l.split("//")[0] for l in open(os.path.join(CSRC, "rt_stream_shade.hpp")).read().splitlines())
    assert shade.count("sq_query<") == 2
    stream = "\n".join(l.split("//")[0] for l in open(os.path.join(CSRC, "rt_stream.hpp")).read().splitlines())
    assert stream.count("sq_query<") == 1
    assert "sq_query<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, scene, slice, lane, o, d, use, false, t_max, best_t, best);" in stream.split("struct SqQuery {")[1].split("\n};\n")[0]
    pixels = stream.split("struct SqPixels {")[1].split("\n};\n")[0]
    assert "sq_tables<HAS_GQ, HAS_CUBIC, false, true>(qa, scene, slice, lane, m, live, sq_pixel_cone(fa.cull != 0u, block, m.d), MAX_T, best_t, best, &fa);" in pixels
    assert "sq_query" not in pixels and "rq_plain" not in pixels and stream.count("sq_tables<HAS_GQ, HAS_CUBIC, false, true>") == 1
    bodies = "\n".join(l.split("//")[0] for l in open(os.path.join(CSRC, "rt_ray_kernels.hpp")).read().splitlines())
    assert "sq_query" not in bodies and "sq_tables" not in bodies
    pixel_bodies = "\n".join(l.split("//")[0] for l in open(os.path.join(CSRC, "rt_pixel_kernels.hpp")).read().splitlines())
    assert "sq_query" not in pixel_bodies and "sq_tables" not in pixel_bodies and "rq_tables" not in pixel_bodies
    assert len(re.findall(r"SqQuery q\{(qa|sa\.qa|pa\.qa), scene, smem \+ \(threadIdx\.x >> 6\) \* SQ_SLICE_BYTES\};", code)) == 2      # the wave's own slice
    colour = code.split("void shade_rays_stream_kernel")[1].split("void path_query_stream_kernel")[0]
    assert "SqQuery q{sa.qa, scene, smem + (threadIdx.x >> 6) * SQ_SLICE_BYTES};" in colour
    assert "rk_shade_rays<HAS_GQ, HAS_CUBIC>(sa, scene, lights, rays, out_rgba, out_rec, q);" in colour and "sq_query<" not in colour
    assert "RkShade<Query> pol{q, out_rec, i, live};" in bodies and "shade_loop<HAS_GQ, HAS_CUBIC>(sa, scene, lights, lane, pol, o, d, live);" in bodies


# ---- the conditions of the GPU tests, on the composers alone --------------------------------------------------------------------------------
def test_the_scenes_are_beyond_the_limit(pkg):
    sizes = {name: {k: len(v) for k, v in Q.tables(B.beyond(name).coefs).items()} for name in B.BEYOND}
    assert sizes[B.BEYOND[0]] == dict(sphere=Q.QUERY_LIMIT_SPHERES + 2, quadric=0, plane=0, cubic=0)
    assert sizes[B.BEYOND[1]] == dict(sphere=Q.QUERY_LIMIT_SPHERES + 65, quadric=0, plane=0, cubic=0)
    assert sizes[B.BEYOND[2]] == dict(sphere=B.MIXED_OBJECTS // 2, quadric=B.MIXED_OBJECTS // 2, plane=2, cubic=0)
    for name in B.BEYOND:
        assert B.table_bytes(B.beyond(name).coefs) > S.LDS_LIMIT, name
    assert len(Q.chunks(Q.tables(B.beyond(B.BEYOND[0]).coefs)["sphere"])) == 41 and len(Q.chunks(Q.tables(B.beyond(B.BEYOND[1]).coefs)["sphere"])) == 42
    c = B.beyond(B.BEYOND[1])
    assert (np.asarray(c.osc.reflection) > 0).sum() > 800 and c.osc.max_reflections == 2
    c = B.beyond(B.BEYOND[2])
    assert (np.asarray(c.osc.reflection) > 0).sum() > 300 and c.osc.max_reflections == 2
    assert max(B.FIELD_PREFIXES) <= len(B.beyond(B.BEYOND[0]).rays)


@pytest.mark.parametrize("name", B.BEYOND)
def test_beyond_cases(pkg, name):
    """The conditions of tests/test_query_tables_host.py::test_large_cases: a third of the aimed rays own their target, one in every chunk of
    every table; the blockers lie in at least ten chunks; an object of each table's last chunk owns a pixel of Q.ROWS."""
    c = B.beyond(name)
    n = len(c.coefs)
    assert 150 < len(c.targets) <= 250 + 2 * sum(len(Q.chunks(t)) for t in Q.tables(c.coefs).values()) and set(Q.boundary_targets(c.coefs)) <= set(c.targets)
    check_aimed_rays_own_their_targets(c, [n - 1] if name == B.BEYOND[0] else [])   # the large sphere appended last
    check_occlusion_spans_the_chunks(c, at_least=10, last_each_pass=False)
    obj = set(np.unique(gbuffer_ref.compose(c.osc, rows=Q.ROWS)["object"]).tolist())
    for table, ch in last_chunks(c.coefs).items():
        assert obj & set(ch), (table, "the last chunk owns no pixel of the composed rows")


def test_the_moved_case(pkg):
    import rays_ref
    sc, coefs, c = B.moved_beyond(pkg)
    before = B.beyond(B.BEYOND[0])
    assert c.targets == before.targets and (np.abs(c.coefs - before.coefs).max(axis=1) > 0).all()
    check_aimed_rays_own_their_targets(c, [len(coefs) - 1])
    assert not rays_ref.same_records(rays_ref.closest(before.osc, c.rays), rays_ref.closest(c.osc, c.rays))
