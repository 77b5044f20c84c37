"""Culled bounce rays (RT_FLAG_STREAM_CULL_BOUNCE, csrc/rt_stream_cull_bounce.hip), host side: the ABI constant and
symbols, what the entry points answer before they look for a device, the build report's lines for the new kernel, the per-ray predicate
asked about chunk bounds against the oracle (tests/tools/bounce_cull_lab.py), and the condition that keeps the GPU statistics test from
being vacuous."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

CSRC = os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")
N_VERDICTS = 20000   # per family here, a few seconds in all; the full count (100 000 per family) is the lab's main: python tests/tools/bounce_cull_lab.py
NEW_FILES = ("rt_ray_bound.hpp", "rt_stream_cull_bounce.hpp", "rt_stream_cull_bounce.hip", "rt_stream_shade.hpp", "rt_stream_shell.hpp")


@pytest.fixture(autouse=True)
def the_feature(pkg):
    """Everything here is about the feature."""
    assert pkg.RT_FLAG_STREAM_CULL_BOUNCE == 1048576


@functools.lru_cache(maxsize=None)
def lab():
    import bounce_cull_lab as B
    B.build()
    return B


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_flag_in_header_and_binding(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"#define RT_FLAG_STREAM_CULL_BOUNCE 1048576u\b", hdr) and "#define RT_ABI_VERSION 3" in hdr
    assert pkg.RT_FLAG_STREAM_CULL_BOUNCE == 1048576 == 0x100000 == 2 * pkg.RT_FLAG_STREAM_CULL
    names = set(re.findall(r"#define (RT_FLAG_\w+|RT_MULTI_\w+) (?:0x[0-9a-fA-F]+|\d+)u\b", hdr))
    assert {"RT_FLAG_STREAM", "RT_FLAG_STREAM_CULL", "RT_FLAG_STREAM_CULL_BOUNCE", "RT_MULTI_SELF_EXCHANGE", "RT_MULTI_BANDWISE", "RT_MULTI_SPARSE"} <= names
    for name in names - {"RT_FLAG_STREAM_CULL_BOUNCE"}:
        assert not (getattr(pkg, name) & pkg.RT_FLAG_STREAM_CULL_BOUNCE), name


def test_symbols_and_prototypes(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"\bint rt_get_stream_cull_bounce\(const rt_ctx \*ctx, uint32_t \*on\);", hdr)
    assert re.search(r"\bint rt_debug_stream_cull_bounce\(rt_ctx \*ctx, uint64_t out\[8\]\);", hdr)
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("rt_get_stream_cull_bounce", "rt_debug_stream_cull_bounce", "rt_launch_stream_cull_bounce_strict", "rt_launch_stream_cull_bounce_fast"):
        assert re.search(rf"\bT {sym}\b", names), sym
        assert sym.startswith("rt_launch") or sym in pkg.ABI_SYMBOLS, sym
    lib = pkg.lib()
    assert lib.rt_get_stream_cull_bounce.argtypes[1] == C.POINTER(C.c_uint32)
    assert lib.rt_debug_stream_cull_bounce.argtypes[1] == C.POINTER(C.c_uint64)
    assert isinstance(pkg.Renderer.stream_cull_bounce, property) and callable(pkg.Renderer.stream_cull_bounce_stats)
    assert isinstance(pkg.MultiRenderer.stream_cull_bounce, property)
    launch = open(os.path.join(CSRC, "rt_launch.h")).read()
    assert re.search(r"RT_PER_VARIANT\(hipError_t, rt_launch_stream_cull_bounce,", launch)
    assert re.search(r"decltype\(&rt_launch_stream_cull_bounce_strict\) stream_cull_bounce;", launch)
    # the update.h adapter reads MI355RT_STREAM_CULL_BOUNCE
    assert b"MI355RT_STREAM_CULL_BOUNCE" in open(pkg.UPDATE_LIB_PATH, "rb").read()


def test_null_arguments_are_refused_before_a_device_is_looked_for(pkg):
    lib = pkg.lib()
    n, words = C.c_uint32(7), (C.c_uint64 * 8)(*([9] * 8))
    assert lib.rt_get_stream_cull_bounce(None, C.byref(n)) == -1 and lib.rt_last_error() == b"rt_get_stream_cull_bounce: null argument" and n.value == 7
    assert lib.rt_debug_stream_cull_bounce(None, words) == -1 and b"rt_debug_stream_cull_bounce: null argument" in lib.rt_last_error()
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
    """No refusal of its own: alone, with RT_FLAG_STREAM_CULL, and with each other flag (and what that flag needs beside it) rt_create gets
    as far as the device query."""
    import torch
    f = pkg
    others = [0, f.RT_FLAG_FAST, f.RT_FLAG_COUNT, f.RT_FLAG_SIMPLE, f.RT_FLAG_NOCULL, f.RT_FLAG_STATIC_ORDER, f.RT_FLAG_NOSCAN, f.RT_FLAG_PLAIN_ORDER, f.RT_FLAG_NOSPLIT,
              f.RT_FLAG_NOLEAN, f.RT_FLAG_SSAA2, f.RT_FLAG_SSAA4, f.RT_FLAG_SSAA2 | f.RT_FLAG_SSAA_ADAPTIVE, f.RT_FLAG_SSAA4 | f.RT_FLAG_SSAA_ADAPTIVE | f.RT_FLAG_SSAA_GEOMETRY,
              f.RT_FLAG_STREAM, f.RT_FLAG_STREAM_QUERIES, f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_QUERIES,
              f.RT_FLAG_STREAM | f.RT_FLAG_SSAA2 | f.RT_FLAG_SSAA_ADAPTIVE | f.RT_FLAG_STREAM_ADAPTIVE]
    for extra in others:
        for cull in (0, f.RT_FLAG_STREAM_CULL):
            rc, msg = _create_rc(pkg, f.RT_FLAG_STREAM_CULL_BOUNCE | cull | extra)
            assert rc in (0, -4), (extra, cull, rc, msg)
            if not torch.cuda.is_available():
                assert rc == -4, (extra, cull, rc, msg)


# ---- the build --------------------------------------------------------------------------------------------------------------------------
def test_build_report_lists_the_new_kernel_without_spills():
    """All four instantiations <HAS_GQ, HAS_CUBIC> of both builds: none spills, none has a private segment, each runs two waves per SIMD."""
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    # (the report cuts a symbol at 40 characters: "_ZN10rtk_strict31stream_cull_bounce_fram")
    lines = [l for l in open(report).read().splitlines() if "stream_cull_bounce_fr" in l]
    for variant in ("strict", "fast"):
        mine = [l for l in lines if l.startswith(f"rt_stream_cull_bounce_{variant}.o")]
        assert len(mine) == 4, mine
    for l in lines:
        assert re.search(r"VGPR spills\s+0\s+scratch 0\b", l) and re.search(r"occupancy 2\b", l), l
        assert int(re.search(r"VGPRs\s+(\d+)", l).group(1)) <= 256, l
    for variant in ("strict", "fast"):   # ... and the full names, from the compiler's own remarks
        remarks = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "csrc", f"rt_stream_cull_bounce_{variant}.o.remarks")).read()
        assert len(set(re.findall(r"Function Name: (\S*stream_cull_bounce_frame_kernel\S*)", remarks))) == 4
    # the twin's file keeps its own four (tests/test_stream_cull_host.py counts them by another name)
    assert len([l for l in open(report).read().splitlines() if l.startswith("rt_stream_cull_strict.o")]) == 4


def test_the_new_files_have_no_workgroup_barrier():
    for name in NEW_FILES:
        text = open(os.path.join(CSRC, name)).read()
        code = "\n".join(l.split("//")[0] for l in text.splitlines())
        assert "__syncthreads" not in code and "s_barrier" not in code and '"workgroup"' not in code and "rq_stage_tables" not in code, name
        assert "extern __shared__" not in code and "HIP_DYNAMIC_SHARED" not in code, name
        assert "__shared__" not in code or name.endswith(".hip"), name      # (nothing of the bounds goes to LDS: only the kernel's own slices)
    query = open(os.path.join(CSRC, "rt_stream_cull_bounce.hpp")).read()
    assert "sq_stage_chunk" in query and "sc_sweep<false>" in query and "ray_reaches" in query
    kernel = open(os.path.join(CSRC, "rt_stream_cull_bounce.hip")).read()
    assert "sc_query_bounce<HAS_GQ, HAS_CUBIC>" in kernel and "sq_query<HAS_GQ, HAS_CUBIC, false>" not in kernel     # no instantiation keeps the full sweep


def test_the_twin_kernel_file_is_untouched():
    """The twin still sweeps its bounce rays in full: neither its kernel file nor the header that holds its shading policy (ScShade) can
    reach sc_query_bounce, even by mistake, and the policy's nearest-hit query of a segment k != 0 is sq_query without a cone."""
    for name in ("rt_stream_cull.hip", "rt_stream_cull.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "sc_query_bounce" not in text and not re.search(r'#\s*include\s*"rt_stream_cull_bounce\.hpp"', text), name
    twin = open(os.path.join(CSRC, "rt_stream_cull.hip")).read()
    assert "ScShade pol{qa, ca, scene, slice, st};" in twin and "shade_loop<HAS_GQ, HAS_CUBIC>(fa, scene, lights, lane, pol," in twin
    policy = open(os.path.join(CSRC, "rt_stream_cull.hpp")).read().split("struct ScShade {")[1]
    nearest = policy.split("void nearest(")[1].split("__device__")[0]
    assert re.search(r"if \(k == 0u\) sc_query_primary<HAS_GQ, HAS_CUBIC>\([^;]*;[^\n]*\n\s*else sq_query<HAS_GQ, HAS_CUBIC, false>\(qa, scene, slice, lane, o, d, use, false, MAX_T, best_t, best\);",
                     nearest), nearest


# ---- the predicate, asked about bounds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["rim", "any", "on_member", "inside", "behind"])
def test_a_skipped_bound_has_no_member_the_oracle_accepts(family):
    """ray_reaches says "skip" => orc_intersect_ray gives no member a root with t >= EPS && t < MAX_T.  A sphere grazed by the ray at
    relative clearances +-1e-1 ... +-1e-15, radii 1e-4 ... 10 scales, translations to 1e7, |d| from 1e-3 to 1e3, companions up to 1e5 radii
    away; the origin 1e-2 above a member, inside the bound, or with the chunk behind it.  Zero unsound; a skipped bound implies the grazed
    member's own predicate skips it; an origin inside the bound always reaches it; no sampled bound beyond the 1e-3 band is kept; two runs
    agree."""
    B = lab()
    row = B.run_family(family, N_VERDICTS)
    print(B.format_row(row))
    assert row["cases"] >= N_VERDICTS and row["unsound"] == 0, row
    assert row["member_kept_bound_skipped"] == 0 and row["origin_inside_skipped"] == 0, row
    assert row["inv_r_short"] == 0 and row["not_enclosed"] == 0 and row["kept"] == 0 and row["repeat_differs"] == 0, row
    assert row["accepted"] > 0 and row["accepted"] < row["cases"], row
    # the same predicate compiled as the FAST kernel build compiles it (-ffp-contract=fast), about the same bounds and truths
    if B.host_has_fma():
        assert row["fast_cases"] == row["cases"] and row["fast_unsound"] == 0, row
    if family in ("rim", "any"):
        assert row["beyond"] >= 50, row      # (the tightness sample is not empty)
    if family == "inside":
        assert row["culled"] == 0, row       # (by construction: the family shows that such a ray is never culled for)
    else:
        assert row["culled"] > 0, row


def test_rays_nothing_is_culled_for():
    """|d|^2 <= EPS, non-finite components and components beyond 1e100 always answer "test it" -- about a bound an ordinary ray skips."""
    for variant in ("strict", "fast") if lab().host_has_fma() else ("strict",):
        odd, away = lab().never_culled(variant)
        assert len(odd) >= 12 and (odd == 1).all(), (variant, odd)
        assert away == 0, variant


def test_header_compiles_for_the_host_with_the_formulas_of_pack_light():
    text = open(os.path.join(CSRC, "rt_ray_bound.hpp")).read()
    assert "namespace rtm" in text and "1.001 * sqrt(dd)" in text and "(d.x * d.x + d.y * d.y) + d.z * d.z" in text
    assert "sphere_relevant<false>(bound, rb.ball, rb.dir)" in text
    pack = open(os.path.join(CSRC, "rt_scene_pack.hpp")).read()
    assert "l.len_u = 1.001 * sqrt(l.u2);" in pack and "l.u2 = (l.dxx + l.dyy) + l.dzz;" in pack


# ---- the statistics scene ---------------------------------------------------------------------------------------------------------------
def test_statistics_scene_is_not_vacuous(pkg):
    """The scene of tests/test_stream_cull_bounce_gpu.py::test_statistics: stream_cull_lab's 320 clustered spheres (5 chunks), every one
    reflecting 0.6, max_reflections = 2, 64 x 48.  From the oracle's per-segment rays: D = (block, segment >= 1 with a bouncing lane) pairs x
    chunks, L = the triples no lane's half-line comes within 1.01 r + 0.1 of; L >= D / 4."""
    e = lab().expectation()
    print(e)
    assert e["n_chunks"] == 5 and e["queries"] >= 8 and e["D"] == e["queries"] * 5 and e["rays"] >= e["queries"]
    assert e["L"] >= e["D"] / 4, e
