"""Culled streamed adaptive passes (csrc/rt_stream_cull_adaptive.hip), host side: the entry points and what they
answer before a device is looked for, the build report's lines for the new kernel (no spill, two waves per SIMD), the new file's
wave-only discipline, the wave cone on the CPU (tests/tools/wave_cone_lab.cpp compiles csrc/rt_wave_cone.hpp for the host) for the
cases of tests/test_stream_cull_adaptive_gpu.py, and the conditions that keep the GPU tests from being vacuous -- on the oracle alone."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import stream_adaptive_scenes as A  # noqa: E402
import launch_table as LT  # noqa: E402
import stream_cull_adaptive_scenes as CA  # noqa: E402

CSRC = os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")
BUILD = os.path.join(ROOT, "cuda-ray-tracer_amd", "build")


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_prototypes(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"\bint rt_get_stream_cull_adaptive\(const rt_ctx \*ctx, uint32_t \*on\);", hdr)
    assert re.search(r"\bint rt_debug_stream_cull_adaptive\(rt_ctx \*ctx, uint64_t out\[8\]\);", hdr)
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("rt_get_stream_cull_adaptive", "rt_debug_stream_cull_adaptive", "rt_launch_stream_cull_ray_list_strict", "rt_launch_stream_cull_ray_list_fast"):
        assert re.search(rf"\bT {sym}\b", names), sym
        assert sym.startswith("rt_launch") or sym in pkg.ABI_SYMBOLS, sym
    lib = pkg.lib()
    assert lib.rt_get_stream_cull_adaptive.argtypes[1] == C.POINTER(C.c_uint32)
    assert lib.rt_debug_stream_cull_adaptive.argtypes[1] == C.POINTER(C.c_uint64)
    assert isinstance(pkg.Renderer.stream_cull_adaptive, property) and callable(pkg.Renderer.stream_cull_adaptive_stats)
    launch = open(os.path.join(CSRC, "rt_launch.h")).read()
    assert len(re.findall(r"RT_PER_VARIANT\(hipError_t, rt_launch_stream_cull_ray_list,", launch)) == 1
    assert re.search(r"decltype\(&rt_launch_stream_cull_ray_list_strict\) stream_cull_ray_list;", launch)   # the Kernels member
    capi = open(os.path.join(CSRC, "rt_capi.cpp")).read()
    assert LT.slot_of("rt_launch_stream_cull_ray_list") == "stream_cull_ray_list"      # ... filled by its name (tests/tools/launch_table.py)
    # the halo and the refine launch go through one function, which holds the one call of each of the three launchers
    one = capi.split("static hipError_t ray_list_launch(")[1].split("\n}\n")[0]
    for launcher in ("kern->stream_cull_ray_list(", "kern->stream_ray_list(", "kern->ray_list("):
        assert one.count(launcher) == 1 and capi.count(launcher) == 1, launcher
    assert capi.split("static int render_impl(")[1].split("\n}\n")[0].count("ray_list_launch(") == 2 and capi.count("ray_list_launch(") == 3


def test_null_arguments_are_refused_before_a_device_is_looked_for(pkg):
    lib = pkg.lib()
    n, words = C.c_uint32(7), (C.c_uint64 * 8)(*([9] * 8))
    assert lib.rt_get_stream_cull_adaptive(None, C.byref(n)) == -1 and lib.rt_last_error() == b"rt_get_stream_cull_adaptive: null argument" and n.value == 7
    assert lib.rt_debug_stream_cull_adaptive(None, words) == -1 and lib.rt_last_error() == b"rt_debug_stream_cull_adaptive: null argument"
    assert list(words) == [9] * 8


# ---- the build --------------------------------------------------------------------------------------------------------------------------
def test_build_report_lists_the_new_kernel_without_spills_at_two_waves_per_simd():
    """35 instantiations per variant: K = 1 (RGBA32F) and K = 2 / 4 in both formats, times <HAS_GQ, HAS_CUBIC>, without the work words
    (20) and with them (15: the counting kernel for general quadrics AND degree 3 does not fit and is not built)."""
    report = os.path.join(BUILD, "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    lines = [l for l in open(report).read().splitlines() if re.search(r"\d\dray_list_cull_kernel", l)]
    for variant in ("strict", "fast"):
        mine = [l for l in lines if l.startswith(f"rt_stream_cull_adaptive_{variant}.o")]
        assert len(mine) == 35, (variant, len(mine))
    assert len(lines) == 70
    for l in lines:
        assert re.search(r"VGPR spills\s+0\s+scratch 0\b", l), l
        assert int(re.search(r"occupancy\s+(\d+)", l).group(1)) >= 2, l
    for variant in ("strict", "fast"):   # ... and the full names, from the compiler's own remarks
        remarks = open(os.path.join(BUILD, "csrc", f"rt_stream_cull_adaptive_{variant}.o.remarks")).read()
        names = set(re.findall(r"Function Name: (\S*ray_list_cull_kernel\S*)", remarks))
        assert len(names) == 35
        flags = {tuple(re.search(r"kernelILi(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", n).groups()) for n in names}
        want = {(k, f, g, c, s) for k, fs in (("1", "0"), ("2", "01"), ("4", "01")) for f in fs for g in "01" for c in "01" for s in "01"} - \
               {(k, f, "1", "1", "1") for k in "124" for f in "01"}
        assert flags == want, flags ^ want
    # the neighbours' counts are what they were
    assert len([l for l in open(report).read().splitlines() if re.search(r"\d\dray_list_stream_kernel", l)]) == 40


def test_the_new_files_have_no_workgroup_barrier_and_no_dynamic_lds():
    for name in ("rt_stream_cull_adaptive.hip", "rt_wave_cone.hpp", "rt_stream_shade.hpp", "rt_stream_shell.hpp", "rt_ray_list.hpp", "rt_wave_ball.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        code = "\n".join(l.split("//")[0] for l in text.splitlines())
        for word in ("__syncthreads", "s_barrier", '"workgroup"', "rq_stage_tables", "extern __shared__", "HIP_DYNAMIC_SHARED"):
            assert word not in code, (name, word)
    text = open(os.path.join(CSRC, "rt_stream_cull_adaptive.hip")).read()
    assert "__shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];" in text          # 24 KiB, static
    assert len(re.findall(r"\), g, block, 0, stream,", text)) == 1
    # the shadow rule: the wave-cone policy is the block policy with two members replaced, so the ball and the culled shadow query are the
    # block policy's own (rt_stream_cull.hpp: ScShade), the ball read back through lane 0
    assert "struct ScaShade : ScShade {" in text and "Segment seg = ScShade::segment(hit, sp);" in text and text.count("sq_readlane(seg.ball.") == 4
    assert "void occluded(" not in text.split("struct ScaShade : ScShade {")[1].split("};")[0]
    assert "ScaShade pol{{qa, ca, scene, slice, st}, nocone};" in text and "shade_loop<HAS_GQ, HAS_CUBIC>(fa, scene, lights, lane, pol, origin, it.dir, it.use);" in text
    block = open(os.path.join(CSRC, "rt_stream_cull.hpp")).read().split("struct ScShade {")[1]
    assert "seg.cull = wave_hit_ball(hit, sp, seg.ball);" in block and block.count("sc_query_shadow<") == 2
    for variant in ("strict", "fast"):
        remarks = open(os.path.join(BUILD, "csrc", f"rt_stream_cull_adaptive_{variant}.o.remarks")).read()
        assert set(re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)) == {"24576"}


# ---- the wave cone on the CPU -------------------------------------------------------------------------------------------------------------
def report(what, r):
    print(what, {k: v for k, v in r.items() if k not in ("cones", "verdicts")})


@pytest.mark.parametrize("key", CA.SCENES, ids=[" ".join(str(v) for v in key) for key in CA.SCENES])
def test_list_waves_lie_in_their_cone_and_no_rejected_chunk_holds_a_hit(key):
    """Every list wave of the oracle's refined list, k = 2 and 4, tau = -1 and 1/32: every used lane satisfies dot(axis, d) >= cos_t bit
    for bit, the axis is a used lane's direction bit for bit, and no sample's primary hit lies in a chunk that sphere_in_cone rejects."""
    culled = 0
    for k in (2, 4):
        for tau in (-1.0, CA.TAU):
            xy, _ = CA.list_waves(key, k, tau)
            r = CA.check_waves(key, k, xy)
            report((key, k, tau), r)
            assert r["waves"] > 0 and r["bad_lanes"] == 0 and r["axis_not_a_lane"] == 0 and r["unsound"] == 0, (key, k, tau)
            assert r["hit_pairs"] > 0
            culled += r["culled"]
    assert culled > 0, key   # (some chunk is rejected for some wave: the verdicts are not all "test it")


@pytest.mark.parametrize("case", CA.BANDS, ids=[f"world{c[1]}-band{c[2]}" for c in CA.BANDS])
def test_banded_list_waves_and_halo_waves(case):
    key, world, band, k, _ = case
    halo_used = halo_unused = 0
    for rank in range(world):
        for tau in (0.0, CA.TAU):
            xy, _ = CA.list_waves(key, k, tau, world, rank, band)
            r = CA.check_waves(key, k, xy)
            assert r["bad_lanes"] == 0 and r["axis_not_a_lane"] == 0 and r["unsound"] == 0, (case, rank, tau)
        hxy = CA.halo_waves(key, world, rank, band)
        r = CA.check_waves(key, 1, hxy)
        report((case, rank, "halo"), r)
        assert r["waves"] > 0 and r["bad_lanes"] == 0 and r["axis_not_a_lane"] == 0 and r["unsound"] == 0, (case, rank)
        halo_used += r["used_lanes"]
        halo_unused += r["waves"] * 64 - r["used_lanes"]
        # a halo wave that straddles two slots (37 columns are no divisor of 64), hence two rows that are 2 band + 1 ... rows apart
        rows = [set(w[w[:, 0] >= 0][:, 1].tolist()) for w in hxy]
        assert any(len(s) > 1 for s in rows), (case, rank)
    assert halo_used > 0 and halo_unused > 0   # (off-image halo rows and the last wave's tail)


def test_geometry_list_waves():
    """The lists of RT_FLAG_SSAA_GEOMETRY at min_cos -inf and 0.9 (object and normal edges beside the colour edges)."""
    import ssaa_adaptive_ref as ada
    import ssaa_geometry_ref as geo
    key = CA.GEOMETRY
    obj, nrm = A.planes(key)
    for k, c in ((2, -CA.INF), (4, 0.9)):
        for tau in (CA.TAU, CA.INF):
            mask = ada.refine_mask(CA.frame(key), tau) | geo.geo_mask(obj, nrm, c)
            assert mask.any() and not mask.all()
            xy, _ = CA.list_waves(key, k, tau, mask=mask)
            r = CA.check_waves(key, k, xy)
            report((key, k, tau, c), r)
            assert r["waves"] > 0 and r["bad_lanes"] == 0 and r["axis_not_a_lane"] == 0 and r["unsound"] == 0 and r["hit_pairs"] > 0, (k, tau, c)


def test_some_wave_straddles_two_blocks_and_some_wave_has_unused_lanes():
    straddle = partial = False
    for key in CA.SCENES:
        for k in (2, 4):
            xy, pix = CA.list_waves(key, k, CA.TAU)
            straddle = straddle or CA.straddles_two_blocks(pix)
            n_items = int((pix[:, :, 0] >= 0).sum())
            partial = partial or n_items % (64 // (k * k)) != 0
    assert straddle and partial


# ---- the conditions of the GPU tests -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CA.SCENES, ids=[" ".join(str(v) for v in key) for key in CA.SCENES])
def test_refined_sets_are_neither_empty_nor_everything_and_reach_the_first_and_last_chunk(key):
    import ssaa_adaptive_ref as ada
    mask = ada.refine_mask(CA.frame(key), CA.TAU)
    assert mask.any() and not mask.all(), key
    chunk, bounds = CA.table(key)
    xy, _ = CA.list_waves(key, 2, CA.TAU)
    c = CA.cones_of(key, 2, xy)
    own = c["owner"][c["use"] != 0]
    hit = set(chunk[own[own >= 0]].tolist())
    assert 0 in hit and len(bounds) - 1 in hit and len(bounds) >= 2, (key, sorted(hit), len(bounds))


def test_statistics_scene_is_not_vacuous():
    """tests/test_stream_cull_adaptive_gpu.py::test_statistics: D0 = waves x chunks, L >= D0 / 4, and the oracle's hits need fewer chunks
    than D0 - L."""
    e = CA.stats_expectation()
    print(e)
    assert e["n_chunks"] == 5 and e["D0"] == (64 * 48 * 16 // 64) * 5
    assert e["L"] >= e["D0"] / 4, e
    assert 0 < e["H"] <= e["D0"] - e["L"] and e["unsound"] == 0 and e["bad_lanes"] == 0, e
