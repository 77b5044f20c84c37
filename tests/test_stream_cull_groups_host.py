"""Grouped chunk bounds (RT_FLAG_STREAM_CULL_GROUPS, csrc/rt_stream_cull_groups.hip), host side: the ABI constant and
symbols, what the entry points answer before they look for a device, the build report's lines for the new kernels, the group bounds of
scene images held to 50-digit arithmetic, and the four culling predicates asked about group bounds beside their chunk bounds and members
(tests/tools/group_cull_lab.py).  No GPU."""
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
N_CASES = 13000      # per predicate and family: 8 x 13 000 = 104 000 sampled (group, query) pairs; the lab's main runs 100 000 per row
NEW_FILES = ("rt_stream_cull_groups.hpp", "rt_stream_cull_groups.hip", "rt_group_bounds.hip")


@functools.lru_cache(maxsize=None)
def lab():
    import group_cull_lab as G
    G.build()
    return G


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_flag_in_header_and_binding(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"#define RT_FLAG_STREAM_CULL_GROUPS 16777216u\b", hdr) and "#define RT_ABI_VERSION 3" in hdr
    assert pkg.RT_FLAG_STREAM_CULL_GROUPS == 16777216 == 0x1000000 == 2 * pkg.RT_FLAG_STREAM_CULL_REORDER
    names = set(re.findall(r"#define (RT_FLAG_\w+|RT_MULTI_\w+) (?:0x[0-9a-fA-F]+|\d+)u\b", hdr))
    assert {"RT_FLAG_STREAM", "RT_FLAG_STREAM_CULL", "RT_FLAG_STREAM_CULL_GROUPS", "RT_MULTI_SELF_EXCHANGE", "RT_MULTI_BANDWISE", "RT_MULTI_SPARSE"} <= names
    for name in names - {"RT_FLAG_STREAM_CULL_GROUPS"}:
        assert not (getattr(pkg, name) & pkg.RT_FLAG_STREAM_CULL_GROUPS), name
    para = hdr.split("#define RT_FLAG_STREAM_CULL_GROUPS")[0].split("#define RT_FLAG_STREAM_CULL_REORDER")[1]
    for text in ("stream groups = RT_FLAG_STREAM_CULL_GROUPS && rt_get_stream_cull && at least 2 groups", "4 097 unit spheres", "Results are unchanged by definition",
                 "Known limits:", "Out of scope:", "any fan-out other than 64", "a third level", "best_t pruning", "the flag as a default", "Not built:"):
        assert text in para, text


def test_symbols_and_prototypes(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"\bint rt_get_stream_groups\(const rt_ctx \*ctx, uint32_t \*on\);", hdr)
    assert re.search(r"\bint rt_debug_stream_groups\(rt_ctx \*ctx, uint64_t out\[8\]\);", hdr)
    assert re.search(r"\bint rt_debug_stream_group_bounds\(rt_ctx \*ctx, void \*out, size_t cap, size_t \*bytes\);", hdr)
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("rt_get_stream_groups", "rt_debug_stream_groups", "rt_debug_stream_group_bounds", "rt_launch_stream_cull_groups_strict", "rt_launch_stream_cull_groups_fast",
                "rt_launch_group_bounds"):
        assert re.search(rf"\bT {sym}\b", names), sym
        assert sym.startswith("rt_launch") or sym in pkg.ABI_SYMBOLS, sym
    lib = pkg.lib()
    assert lib.rt_get_stream_groups.argtypes[1] == C.POINTER(C.c_uint32)
    assert lib.rt_debug_stream_groups.argtypes[1] == C.POINTER(C.c_uint64)
    assert lib.rt_debug_stream_group_bounds.argtypes[3] == C.POINTER(C.c_size_t)
    assert isinstance(pkg.Renderer.stream_groups, property) and callable(pkg.Renderer.debug_stream_groups) and callable(pkg.Renderer.debug_stream_group_bounds)
    assert isinstance(pkg.MultiRenderer.stream_groups, property)
    # the update.h adapter reads MI355RT_STREAM_CULL_GROUPS
    assert b"MI355RT_STREAM_CULL_GROUPS" in open(pkg.UPDATE_LIB_PATH, "rb").read()


def test_the_launchers_live_in_a_record_of_their_own(pkg):
    launch = open(os.path.join(CSRC, "rt_launch.h")).read()
    assert re.search(r"RT_PER_VARIANT\(hipError_t, rt_launch_stream_cull_groups,", launch)
    assert re.search(r"struct GroupTables \{\s*const void \*groups;\s*uint32_t n_groups;\s*unsigned long long \*stats;\s*\};", launch)
    assert re.search(r"struct GroupLaunchers \{\s*decltype\(&rt_launch_stream_cull_groups_strict\) frame;\s*\};", launch)
    kernels = re.search(r"struct Kernels \{(.*?)\n\};", launch, flags=re.S).group(1)
    assert "groups" not in kernels
    assert 'extern "C" hipError_t rt_launch_group_bounds(const void *bounds, uint32_t n_chunks, void *groups, hipStream_t stream);' in launch
    capi = open(os.path.join(CSRC, "rt_capi.cpp")).read()
    assert "static const GroupLaunchers group_launchers_strict = RT_GROUP_LAUNCHERS(strict), group_launchers_fast = RT_GROUP_LAUNCHERS(fast);" in capi
    assert "k.frame = RT_CAT(rt_launch_stream_cull_groups, V);" in capi
    families = re.search(r"enum CullFamily \{(.*?)\};", capi, flags=re.S).group(1)
    assert "GROUP" not in families
    # the args records of the existing kernels are what they were; the group table travels in its own
    for name, struct in (("rt_stream_cull.hpp", "StreamCullArgs"), ("rt_scene_dev.h", "FrameArgs"), ("rt_set_scene.h", "SetSceneArgs")):
        body = re.search(rf"struct {struct} \{{(.*?)\n\}};", open(os.path.join(CSRC, name)).read(), flags=re.S).group(1)
        code = "\n".join(l.split("//")[0] for l in body.splitlines())
        assert "group" not in code.lower(), struct
    # one validation rule of the groups record's own, over sc_cull_args for the chunk part
    hpp = open(os.path.join(CSRC, "rt_stream_cull_groups.hpp")).read()
    assert "if (!sc_cull_args(fa, ct, ca)) return false;" in hpp and "gt->n_groups != (ca.n_chunks + SG_FANOUT - 1u) / SG_FANOUT" in hpp
    for name in NEW_FILES:
        text = open(os.path.join(CSRC, name)).read()
        assert "sc_cull_args(fa, chunks, ca)" not in text and "SQ_CHUNK - 1u) / SQ_CHUNK" not in text, name
    assert open(os.path.join(CSRC, "rt_stream_cull_groups.hip")).read().count("sg_group_args(fa, chunks, groups, ca, ga)") == 1


def test_null_arguments_are_refused_before_a_device_is_looked_for(pkg):
    lib = pkg.lib()
    n, words, size = C.c_uint32(7), (C.c_uint64 * 8)(*([9] * 8)), C.c_size_t(5)
    assert lib.rt_get_stream_groups(None, C.byref(n)) == -1 and lib.rt_last_error() == b"rt_get_stream_groups: null argument" and n.value == 7
    assert lib.rt_get_stream_groups(C.c_void_p(16), None) == -1 and lib.rt_last_error() == b"rt_get_stream_groups: null argument"
    assert lib.rt_debug_stream_groups(None, words) == -1 and lib.rt_last_error() == b"rt_debug_stream_groups: null argument" and list(words) == [9] * 8
    assert lib.rt_debug_stream_groups(C.c_void_p(16), None) == -1 and lib.rt_last_error() == b"rt_debug_stream_groups: null argument"
    assert lib.rt_debug_stream_group_bounds(None, None, 0, C.byref(size)) == -1 and lib.rt_last_error() == b"rt_debug_stream_group_bounds: null argument" and size.value == 5
    assert lib.rt_debug_stream_group_bounds(C.c_void_p(16), None, 0, None) == -1 and lib.rt_last_error() == b"rt_debug_stream_group_bounds: null argument"


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
              f.RT_FLAG_STREAM | f.RT_FLAG_SSAA2 | f.RT_FLAG_SSAA_ADAPTIVE | f.RT_FLAG_STREAM_ADAPTIVE,
              f.RT_FLAG_STREAM_CULL_BOUNCE, f.RT_FLAG_STREAM_CULL_RAYS, f.RT_FLAG_STREAM_CULL_PIXELS, f.RT_FLAG_STREAM_CULL_REORDER]
    for extra in others:
        for cull in (0, f.RT_FLAG_STREAM_CULL):
            rc, msg = _create_rc(pkg, f.RT_FLAG_STREAM_CULL_GROUPS | cull | extra)
            assert rc in (0, -4), (extra, cull, rc, msg)
            if not torch.cuda.is_available():
                assert rc == -4, (extra, cull, rc, msg)


# ---- the build --------------------------------------------------------------------------------------------------------------------------
def test_build_report_lists_the_new_kernels_without_spills():
    """<HAS_GQ, HAS_CUBIC, BOUNCE, STATS>: fifteen instantiations per build (the one that counts and culls bounce rays for general quadrics
    plus degree 3 is not built); none spills, none has a private segment, each runs two waves per SIMD.  The group-bounds kernel is built
    once."""
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    text = open(report).read().splitlines()
    lines = [l for l in text if "stream_cull_groups_fr" in l]
    for variant in ("strict", "fast"):
        mine = [l for l in lines if l.startswith(f"rt_stream_cull_groups_{variant}.o")]
        assert len(mine) == 15, mine
        remarks = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "csrc", f"rt_stream_cull_groups_{variant}.o.remarks")).read()
        built = set(re.findall(r"Function Name: \S*stream_cull_groups_frame_kernelI(Lb[01]ELb[01]ELb[01]ELb[01]E)", remarks))
        assert len(built) == 15 and "Lb1ELb1ELb1ELb1E" not in built, built
    for l in lines:
        assert re.search(r"VGPR spills\s+0\s+scratch 0\b", l) and re.search(r"occupancy 2\b", l), l
        assert int(re.search(r"VGPRs\s+(\d+)", l).group(1)) <= 256, l
    once = [l for l in text if l.startswith("rt_group_bounds.o")]
    assert len(once) == 1 and "group_bounds_kernel" in once[0] and re.search(r"VGPR spills\s+0\s+scratch 0\b", once[0]), once
    make = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "Makefile")).read()
    assert re.search(r"\$\(eval \$\(call VARIANT_RULES,rt_stream_cull_groups,", make)
    rule = re.search(r"^(\$\(BUILD\)/csrc/rt_resolve\.o[^\n:]*):[^\n]*\n((?:\t[^\n]*\n)+)", make, flags=re.M)
    assert "$(BUILD)/csrc/rt_group_bounds.o" in rule.group(1) and "-ffp-contract=off" in rule.group(2)      # built once, without contraction
    # the twins keep their own four each
    assert len([l for l in text if l.startswith("rt_stream_cull_strict.o")]) == 4 and len([l for l in text if l.startswith("rt_stream_cull_bounce_strict.o")]) == 4


def test_the_new_files_have_no_workgroup_barrier():
    for name in NEW_FILES:
        text = open(os.path.join(CSRC, name)).read()
        code = "\n".join(l.split("//")[0] for l in text.splitlines())
        assert "__syncthreads" not in code and "s_barrier" not in code and '"workgroup"' not in code and "rq_stage_tables" not in code, name
        assert "extern __shared__" not in code and "HIP_DYNAMIC_SHARED" not in code, name
        assert "__shared__" not in code or name == "rt_stream_cull_groups.hip", name      # (nothing of the bounds goes to LDS: only the kernel's own slices)
    hpp = open(os.path.join(CSRC, "rt_stream_cull_groups.hpp")).read()
    assert "sq_stage_chunk" in hpp and "sc_sweep<true>" in hpp and "sc_sweep<false>" in hpp and "ray_reaches" in hpp and "sphere_in_cone" in hpp
    kernel = open(os.path.join(CSRC, "rt_stream_cull_groups.hip")).read()
    assert "shade_loop<HAS_GQ, HAS_CUBIC>(fa, scene, lights, lane, pol," in kernel and "SgShade<BOUNCE> pol{" in kernel


def test_the_existing_kernel_files_are_untouched():
    """Neither twin can reach the grouped queries, and the update kernels know nothing of groups: the host enqueues rt_launch_group_bounds
    behind them."""
    for name in ("rt_stream_cull.hip", "rt_stream_cull.hpp", "rt_stream_cull_bounce.hip", "rt_stream_cull_bounce.hpp", "rt_set_scene.hip", "rt_reorder_scene.hip",
                 "rt_stream_shade.hpp", "rt_stream.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "sg_query" not in text and "GroupTables" not in text and not re.search(r'#\s*include\s*"rt_stream_cull_groups\.hpp"', text), name
    capi = open(os.path.join(CSRC, "rt_capi.cpp")).read()
    assert capi.count("rt_launch_group_bounds(ctx->d_bounds.p, ctx->n_chunks, ctx->d_groups.p, stream)") == 2
    for launcher in ("rt_launch_set_scene(&a, stream);", "rt_launch_reorder_scene(blob + fa.off_us"):
        behind = capi.split(launcher)[1]
        assert behind.index("rt_launch_group_bounds(") < behind.index("order_end("), launcher


# ---- the group bounds of scene images ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4096, 4097, 8193, 12289])
def test_group_bounds_of_the_field(pkg, n):
    """One group at 4 096 spheres; at 4 097 the second group is one chunk of one entry; 8 193 and 12 289: a third and a fourth likewise."""
    import stream_scenes as S
    row = lab().check_groups(S.field(pkg, n, S.FIELD_SEED).arrays())
    print(row)
    assert row["n_us"] == n and row["n_chunks"] == (n + 63) // 64 and row["n_groups"] == (n + 4095) // 4096 and row["n_inf"] == 0
    assert 0 < row["worst_slack"] < 1e-3      # (enclosing, and by a pad, not by a multiple)


def unbounded_tail_arrays(pkg, n=4200, at=(5, 1700, 4100)):
    """A raw-descriptor scene: the field at n spheres with three of them given r^2 <= 0 (c = |centre|^2 + 1, 0 and +1e300): unit spheres
    without a radius, which the order puts behind every bounded one -- the last chunk, hence the last group, is unbounded."""
    import stream_scenes as S
    a = S.field(pkg, n, S.FIELD_SEED).arrays()
    coefs = a["coefs"].copy()
    for i, extra in zip(at, (1.0, 0.0, 1e300)):
        c = -0.5 * coefs[i, 16:19]
        coefs[i, 19] = float(c @ c) + extra
    return dict(a, coefs=coefs)


def test_group_bounds_with_an_unbounded_last_group(pkg):
    a = unbounded_tail_arrays(pkg)
    row = lab().check_groups(a)
    print(row)
    assert row["n_us"] == 4200 and row["n_groups"] == 2 and row["n_inf"] == 1
    import stream_cull_lab as SC
    g = lab().group_image(SC.image(a)[1]).view(SC.US_DTYPE)
    assert np.isfinite(g["r"][0]) and np.isposinf(g["r"][1]) and g["inv_r"][1] == 0.0


# ---- the predicates, asked about group bounds -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def predicate_rows():
    return lab().run_predicates(N_CASES)


@pytest.mark.parametrize("predicate", ["sphere_in_cone", "sphere_relevant<false>", "sphere_relevant<true>", "ray_reaches"])
def test_a_skipped_group_has_no_kept_chunk_bound_and_no_kept_member(predicate):
    """No sampled group verdict of "skip" stands beside a "test it" for either chunk bound or for any member's own entry, nor beside a
    member the oracle accepts; the group encloses its chunk balls and spheres and carries at least their inv_r; two runs agree; and the
    predicate does skip groups, so none of this holds by never skipping."""
    rows = [r for r in predicate_rows() if r["predicate"] == predicate]
    assert [r["family"] for r in rows] == ["rim", "any"]
    for r in rows:
        print(lab().format_row(r))
        assert r["cases"] >= 0.9 * N_CASES, r      # (a directional light with |d|^2 <= EPS is dropped by the generator)
        assert r["unsound_chunk"] == 0 and r["unsound_member"] == 0 and r["unsound_oracle"] == 0, r
        assert r["not_enclosed"] == 0 and r["inv_r_short"] == 0 and r["repeat_differs"] == 0, r
        assert 0 < r["accepted"] < r["cases"], r
    assert sum(r["skipped"] for r in rows) > 0, rows
    assert rows[0]["skipped"] > 0, rows[0]      # the grazing family itself: chunk A on the group's rim


def test_the_sample_is_large_enough():
    assert sum(r["cases"] for r in predicate_rows()) >= 100000


# ---- the statistics scene ---------------------------------------------------------------------------------------------------------------
def test_statistics_scene_is_not_vacuous(pkg):
    """The scene of tests/test_stream_cull_groups_gpu.py::test_work_words: two clusters of 4 096 spheres, one group each.  At least a quarter
    of the primary group verdicts are skips -- a condition on the input, checked here before any device value is read."""
    import stream_scenes as S
    G = lab()
    sc = G.two_clusters(pkg)
    e = G.primary_expectation(S.oracle_of(pkg, sc), sc.arrays())
    print(e)
    assert e["blocks"] == 48 and e["n_groups"] == 2 and e["n_chunks"] == 128 and e["asked"] == 96
    assert e["asked"] - e["entered"] >= e["asked"] / 4 and e["entered"] > 0 and e["staged"] > 0, e
