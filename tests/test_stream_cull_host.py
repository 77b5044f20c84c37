"""Culled streamed frames (RT_FLAG_STREAM_CULL, csrc/rt_stream_cull.hip), host side: the ABI constants and
symbols, what rt_create answers before it looks for a device, the build report's lines for the new kernel, the scene image of a flagged
context (tests/tools/stream_cull_lab.py: the ordered table and the chunk bounds, by the library's own host functions), the culling
predicates asked about chunk bounds against the oracle, and the condition that keeps the GPU statistics test from being vacuous."""
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
import raw_desc_scenes as R  # noqa: E402
import stream_scenes as S  # noqa: E402

CSRC = os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")
N_VERDICTS = 100000


@pytest.fixture(autouse=True)
def the_feature(pkg):
    """Everything here is about the feature; the lab's tests run library code that exists only with it."""
    assert pkg.RT_FLAG_STREAM_CULL == 524288


@functools.lru_cache(maxsize=None)
def lab():
    import stream_cull_lab as SC
    SC.build()
    return SC


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_flag_in_header_and_binding(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"#define RT_FLAG_STREAM_CULL 524288u\b", hdr) and "#define RT_ABI_VERSION 3" in hdr
    assert pkg.RT_FLAG_STREAM_CULL == 524288 == 0x80000
    names = set(re.findall(r"#define (RT_FLAG_\w+|RT_MULTI_\w+) (?:0x[0-9a-fA-F]+|\d+)u\b", hdr))
    assert {"RT_FLAG_STREAM", "RT_FLAG_STREAM_QUERIES", "RT_FLAG_STREAM_ADAPTIVE", "RT_MULTI_SELF_EXCHANGE", "RT_MULTI_BANDWISE", "RT_MULTI_SPARSE"} <= names
    for name in names - {"RT_FLAG_STREAM_CULL"}:
        assert not (getattr(pkg, name) & pkg.RT_FLAG_STREAM_CULL), name


def test_symbols_and_prototypes(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"\bint rt_get_stream_cull\(const rt_ctx \*ctx, uint32_t \*on\);", hdr)
    assert re.search(r"\bint rt_debug_stream_bounds\(rt_ctx \*ctx, void \*out, size_t cap, size_t \*bytes\);", hdr)
    assert re.search(r"\bint rt_debug_stream_cull\(rt_ctx \*ctx, uint64_t out\[8\]\);", hdr)
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("rt_get_stream_cull", "rt_debug_stream_bounds", "rt_debug_stream_cull", "rt_launch_stream_cull_strict", "rt_launch_stream_cull_fast"):
        assert re.search(rf"\bT {sym}\b", names), sym
        assert sym.startswith("rt_launch") or sym in pkg.ABI_SYMBOLS, sym
    lib = pkg.lib()
    assert lib.rt_get_stream_cull.argtypes[1] == C.POINTER(C.c_uint32)
    assert lib.rt_debug_stream_bounds.argtypes == lib.rt_debug_scene_blob.argtypes
    assert lib.rt_debug_stream_cull.argtypes[1] == C.POINTER(C.c_uint64)
    assert isinstance(pkg.Renderer.stream_cull, property) and callable(pkg.Renderer.stream_bounds) and callable(pkg.Renderer.stream_cull_stats)
    launch = open(os.path.join(CSRC, "rt_launch.h")).read()
    assert re.search(r"RT_PER_VARIANT\(hipError_t, rt_launch_stream_cull,", launch) and re.search(r"decltype\(&rt_launch_stream_cull_strict\) stream_cull;", launch)
    # null arguments need no device
    n, size, words = C.c_uint32(7), C.c_size_t(7), (C.c_uint64 * 8)()
    assert lib.rt_get_stream_cull(None, C.byref(n)) == -1 and lib.rt_last_error() == b"rt_get_stream_cull: null argument" and n.value == 7
    assert lib.rt_debug_stream_bounds(None, None, 0, C.byref(size)) == -1 and b"rt_debug_stream_bounds: null argument" in lib.rt_last_error() and size.value == 7
    assert lib.rt_debug_stream_cull(None, words) == -1 and b"rt_debug_stream_cull: null argument" in lib.rt_last_error()
    # the update.h adapter reads MI355RT_STREAM_CULL
    assert b"MI355RT_STREAM_CULL" in open(pkg.UPDATE_LIB_PATH, "rb").read()


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
    """No refusal of its own: with each other flag (and what that flag needs beside it) rt_create gets as far as the device query."""
    import torch
    f = pkg
    others = [0, f.RT_FLAG_FAST, f.RT_FLAG_COUNT, f.RT_FLAG_SIMPLE, f.RT_FLAG_NOCULL, f.RT_FLAG_STATIC_ORDER, f.RT_FLAG_NOSCAN, f.RT_FLAG_PLAIN_ORDER, f.RT_FLAG_NOSPLIT,
              f.RT_FLAG_NOLEAN, f.RT_FLAG_SSAA2, f.RT_FLAG_SSAA4, f.RT_FLAG_SSAA2 | f.RT_FLAG_SSAA_ADAPTIVE, f.RT_FLAG_SSAA4 | f.RT_FLAG_SSAA_ADAPTIVE | f.RT_FLAG_SSAA_GEOMETRY,
              f.RT_FLAG_STREAM, f.RT_FLAG_STREAM_QUERIES, f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_QUERIES,
              f.RT_FLAG_STREAM | f.RT_FLAG_SSAA2 | f.RT_FLAG_SSAA_ADAPTIVE | f.RT_FLAG_STREAM_ADAPTIVE]
    for extra in others:
        rc, msg = _create_rc(pkg, pkg.RT_FLAG_STREAM_CULL | extra)
        assert rc in (0, -4), (extra, rc, msg)
        if not torch.cuda.is_available():
            assert rc == -4, (extra, rc, msg)


# ---- the build --------------------------------------------------------------------------------------------------------------------------
def test_build_report_lists_the_new_kernel_without_spills():
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    # (the report cuts a symbol at 40 characters: "_ZN10rtk_strict24stream_cull_frame_kerne")
    lines = [l for l in open(report).read().splitlines() if "stream_cull_frame_ker" in l]
    for variant in ("strict", "fast"):
        mine = [l for l in lines if l.startswith(f"rt_stream_cull_{variant}.o")]
        assert len(mine) == 4, mine   # <HAS_GQ, HAS_CUBIC>
    for l in lines:
        assert re.search(r"VGPR spills\s+0\s+scratch 0\b", l), l
    for variant in ("strict", "fast"):   # ... and the full names, from the compiler's own remarks
        remarks = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "csrc", f"rt_stream_cull_{variant}.o.remarks")).read()
        assert len(set(re.findall(r"Function Name: (\S*stream_cull_frame_kernel\S*)", remarks))) == 4


def test_the_new_files_have_no_workgroup_barrier():
    for name in ("rt_stream_cull.hip", "rt_stream_cull.hpp", "rt_stream_shade.hpp", "rt_stream_shell.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        code = "\n".join(l.split("//")[0] for l in text.splitlines())
        assert "__syncthreads" not in code and "s_barrier" not in code and '"workgroup"' not in code and "rq_stage_tables" not in code, name
        assert "extern __shared__" not in code and "HIP_DYNAMIC_SHARED" not in code, name
    assert "sq_stage_chunk" in open(os.path.join(CSRC, "rt_stream_cull.hpp")).read()


# ---- the scene image of a flagged context ---------------------------------------------------------------------------------------------
def raw_scene_with_unbounded_spheres(n=150, seed=9):
    """Raw descriptors: n unit-sphere records of which every seventh has r^2 <= 0 (c = |centre|^2, or larger), so the table's tail has no radius."""
    rng = np.random.default_rng(seed)
    coefs = np.zeros((n, 20))
    coefs[:, 10:13] = 1.0
    c = rng.uniform([-12, -8, 18], [12, 8, 32], (n, 3))
    coefs[:, 16:19] = -2.0 * c
    r2 = np.where(np.arange(n) % 7 == 3, np.where(np.arange(n) % 2 == 0, 0.0, -0.5), 0.09)
    coefs[:, 19] = (c * c).sum(axis=1) - r2
    return dict(coefs=coefs, reflection=np.zeros(n, np.float32), albedo=rng.uniform(0.2, 1, (n, 3)).astype(np.float32), light_is_spherical=np.array([0, 1], np.uint8),
                light_p=np.array([[0.2, -1.0, 0.6], [4.0, 12.0, 2.0]]), light_color=np.ones((2, 3), np.float32))


@pytest.mark.parametrize("case", ["field65", "field129", "large", "field10000", "mixed_large", "raw_unbounded", "raw_seeds"])
def test_ordered_table_and_bounds(pkg, case):
    """The flagged blob differs from the unflagged one only inside the unit-sphere table and is a permutation of it; every finite bound
    encloses every member ball (50-digit arithmetic) with inv_r >= every member's; chunks with an unbounded member are +inf; poisoned fill
    shows every byte written; two runs give identical bytes (tests/tools/stream_cull_lab.py: check_image)."""
    SC = lab()
    if case == "raw_seeds":
        for seed in range(0, R.N_SEEDS, 2):
            SC.check_image(SC.arrays_of_oracle(R.scene(seed)[0]))
        return
    if case == "raw_unbounded":
        got = SC.check_image(raw_scene_with_unbounded_spheres())
        assert got["n_us"] == 150 and got["n_chunks"] == 3 and got["n_inf"] == 1, got   # (22 spheres without a radius: all in the last chunk)
        return
    n_large = S.first_count_beyond_lds(pkg)
    sc = {"field65": lambda: S.field(pkg, 65, S.FIELD_SEED), "field129": lambda: S.field(pkg, 129, S.FIELD_SEED),
          "large": lambda: S.field(pkg, n_large, S.LARGE_SEED, big_last=True), "field10000": lambda: S.field(pkg, 10000, 3),
          "mixed_large": lambda: S.mixed_large(pkg, 2000, S.MIXED_SEED)}[case]()
    got = SC.check_image(sc.arrays())
    want = {"field65": 65, "field129": 129, "large": n_large + 1, "field10000": 10000, "mixed_large": 1000}[case]
    assert got["n_us"] == want and got["n_chunks"] == (want + 63) // 64 and got["n_inf"] == 0, got


def test_the_order_groups_neighbours(pkg):
    """Not a result, but the point of the order: a chunk of the 10 000-sphere field holds 1 / 157 of the spheres, and its bound is far
    smaller than the field (a chunk of the unordered table spans all of it: its bound is about the field's half diagonal)."""
    SC = lab()
    a = S.field(pkg, 10000, 3).arrays()
    _, bounds, w = SC.image(a)
    r = bounds.view(SC.US_DTYPE)["r"]
    c = -0.5 * a["coefs"][:, 16:19]
    half_diagonal = 0.5 * float(np.linalg.norm(c.max(axis=0) - c.min(axis=0)))
    print("median bound radius", float(np.median(r)), "largest", float(r.max()), "half diagonal of the field", half_diagonal)
    assert w["n_chunks"] == 157 and np.median(r) < half_diagonal / 3 and r.max() < half_diagonal


# ---- the predicates, asked about bounds -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,family", [("cone", "rim"), ("cone", "any"), ("sh_dir", "rim"), ("sh_dir", "any"), ("sh_sph", "rim"), ("sh_sph", "any"),
                                         ("sh_sph", "light")])
def test_a_skipped_bound_has_no_member_the_oracle_accepts(kind, family):
    """Bound verdict "skip" => the oracle accepts no member for any ray of the block (cone) or of the chunk of hits (directional, point
    light).  Members on the rim of their bound, grazed at relative clearances +-1e-1 ... +-1e-15; radii 1e-4 ... 10 scales; bounds up to 1e5
    member radii wide; translations to 1e7; point lights inside and next to the bound.  At least 1e5 verdicts per predicate and family,
    zero unsound, between a quarter and three quarters of each set accepted.  Beyond the 1e-3 band of section 14 -- taken at the scale the
    bound's own margin has, which carries the largest 1 / r of the members -- the bound must be culled; the number kept beyond the band at
    section 14's own scale (1 / r of the bound) is printed."""
    SC = lab()
    done = seed = 0
    tot = dict(cases=0, culled=0, accepted=0, unsound=0, inv_r_short=0, not_enclosed=0, beyond14=0, kept14=0, beyond=0, kept=0)
    while done < N_VERDICTS:
        k = min(20000, N_VERDICTS - done)
        rec, v, t, g, members, _ = SC.bound_cases(kind, family, k, seed)
        bc, br, bq = -0.5 * rec[:, 0:3], (rec[:, 3] if kind == "cone" else rec[:, 4]), (rec[:, 4] if kind == "cone" else rec[:, 5])
        fin = np.isfinite(br)
        reach = (np.linalg.norm(members[:, :, :3] - bc[:, None, :], axis=2) + members[:, :, 3]).max(axis=1)
        b14, k14, b, kb = SC.kept_beyond_band(kind, rec, v, sample=120, seed=seed)
        for key, val in (("cases", k), ("culled", int((v == 0).sum())), ("accepted", int((t != 0).sum())), ("unsound", int(((v == 0) & (t != 0)).sum())),
                         ("inv_r_short", int((fin & (bq < members[:, :, 4].max(axis=1))).sum())), ("not_enclosed", int((fin & (br < reach)).sum())),
                         ("beyond14", b14), ("kept14", k14), ("beyond", b), ("kept", kb)):
            tot[key] += val
        done += k
        seed += 1
    print(kind, family, tot)
    assert tot["cases"] >= 100000 and tot["unsound"] == 0, tot
    assert tot["cases"] / 4 <= tot["accepted"] <= 3 * tot["cases"] / 4, tot
    assert tot["inv_r_short"] == 0 and tot["not_enclosed"] == 0, tot
    assert tot["culled"] > 0 and tot["kept"] == 0, tot


# ---- the statistics scene ---------------------------------------------------------------------------------------------------------------
def test_statistics_scene_is_not_vacuous(pkg):
    """The scene of tests/test_stream_cull_gpu.py::test_statistics: mirror-free, 64 x 48, several chunks, both of the field's lights.  From
    the oracle's hit points: D = blocks with a hit x lights x chunks, L = the (block, light, chunk) triples whose bound lies beyond the
    1e-3 band of the Euclidean criterion; L >= D / 4."""
    SC = lab()
    e = SC.stats_expectation(pkg, SC.cluster_scene(pkg))
    print(e)
    assert e["n_chunks"] == 5 and e["blocks"] >= 8 and e["D"] == e["blocks"] * 2 * 5
    assert e["L"] >= e["D"] / 4, e
