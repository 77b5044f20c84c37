"""Streamed adaptive supersampling (RT_FLAG_STREAM_ADAPTIVE, csrc/rt_stream_adaptive.hip), host side: the ABI
constant and symbol, the NULL refusal and the flag-only refusal before a device is looked for, the launcher table's new member, the build
report's lines for the new kernel, and -- on the CPU oracle alone -- the conditions that keep the GPU tests
(tests/test_stream_adaptive_gpu.py) from being vacuous, for every scene, tau and band layout they use (tests/tools/stream_adaptive_scenes.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import query_table_scenes as Q  # noqa: E402
import ssaa_adaptive_ref as ada  # noqa: E402
import ssaa_geometry_ref as geo  # noqa: E402
import stream_adaptive_scenes as A  # noqa: E402
import stream_scenes as S  # noqa: E402

CSRC = os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")


def header():
    return open(os.path.join(ROOT, "include", "mi355rt.h")).read()


def test_flag_in_header_and_binding(pkg):
    hdr = header()
    assert re.search(r"#define RT_FLAG_STREAM_ADAPTIVE 32768u\b", hdr) and "#define RT_ABI_VERSION 3" in hdr
    assert pkg.RT_FLAG_STREAM_ADAPTIVE == 32768 == 0x8000 < pkg.RT_MULTI_SELF_EXCHANGE
    flags = {name: int(value, 0) for name, value in re.findall(r"#define (RT_(?:FLAG|MULTI)_[A-Z0-9_]+) (\d+|0x[0-9a-fA-F]+)u\b", hdr)}
    assert len(flags) >= 20 and flags["RT_FLAG_STREAM_ADAPTIVE"] == 32768
    for name, value in flags.items():
        assert getattr(pkg, name) == value, name
        assert name == "RT_FLAG_STREAM_ADAPTIVE" or not (value & 32768), name
    assert pkg.lib().rt_abi_version() == 3


def test_symbols_and_prototypes(pkg):
    assert re.search(r"\bint rt_get_streamed_adaptive\(const rt_ctx \*ctx, uint32_t \*streamed\);", header())
    assert "rt_get_streamed_adaptive" in pkg.ABI_SYMBOLS
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("rt_get_streamed_adaptive", "rt_launch_stream_ray_list_strict", "rt_launch_stream_ray_list_fast"):
        assert re.search(rf"\bT {sym}\b", names), sym
    # declared once for both variants, with its own member in the table the contexts call through
    launch = open(os.path.join(CSRC, "rt_launch.h")).read()
    assert re.search(r"RT_PER_VARIANT\(hipError_t, rt_launch_stream_ray_list,", launch)
    assert re.search(r"decltype\(&rt_launch_stream_ray_list_strict\) stream_ray_list;", launch.split("struct Kernels")[1])
    assert "RT_CAT(rt_launch_stream_ray_list, V)" in open(os.path.join(CSRC, "rt_capi.cpp")).read()
    lib = pkg.lib()
    assert lib.rt_get_streamed_adaptive.argtypes[1] == C.POINTER(C.c_uint32)
    assert isinstance(pkg.Renderer.streamed_adaptive, property)
    # null arguments need no device
    n = C.c_uint32(7)
    assert lib.rt_get_streamed_adaptive(None, C.byref(n)) == -1 and b"rt_get_streamed_adaptive: null argument" in lib.rt_last_error() and n.value == 7
    assert lib.rt_get_streamed_adaptive(C.c_void_p(16), None) == -1 and b"rt_get_streamed_adaptive: null argument" in lib.rt_last_error()
    # the update.h adapter reads MI355RT_STREAM_ADAPTIVE
    assert b"MI355RT_STREAM_ADAPTIVE" in open(pkg.UPDATE_LIB_PATH, "rb").read()


def _create_rc(pkg, flags):
    sc = pkg.Scene.load_from_file(scene_path("quadratic")).set_size(64, 48)
    d = sc.desc()
    cfg = pkg.Config(-1, 0, 1, 8, int(flags), pkg.RT_FMT_RGBA32F)
    ctx = C.c_void_p()
    rc = pkg.lib().rt_create(C.byref(ctx), C.byref(d), C.byref(cfg))
    msg = pkg.lib().rt_last_error().decode()
    if rc == 0:
        pkg.lib().rt_destroy(ctx)
    return rc, msg


def test_flag_only_refusals_come_before_the_device_query(pkg):
    """RT_ERR_INVALID (-1), not RT_ERR_NO_DEVICE (-4), on a machine without a GPU too."""
    for extra in (0, pkg.RT_FLAG_SSAA2, pkg.RT_FLAG_STREAM, pkg.RT_FLAG_STREAM | pkg.RT_FLAG_SSAA4, pkg.RT_FLAG_SIMPLE):
        rc, msg = _create_rc(pkg, pkg.RT_FLAG_STREAM_ADAPTIVE | extra)
        assert rc == -1 and "RT_FLAG_STREAM_ADAPTIVE needs RT_FLAG_SSAA_ADAPTIVE" in msg, (extra, rc, msg)
    # the refusals around it keep their answers: RT_FLAG_STREAM with RT_FLAG_SSAA_ADAPTIVE without the new flag, and RT_FLAG_STREAM with RT_FLAG_COUNT with it
    ada2 = pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA_ADAPTIVE
    rc, msg = _create_rc(pkg, pkg.RT_FLAG_STREAM | ada2)
    assert rc == -1 and "RT_FLAG_STREAM is not available with RT_FLAG_SSAA_ADAPTIVE (the refine pass has no streamed kernel)" in msg
    rc, msg = _create_rc(pkg, pkg.RT_FLAG_STREAM | ada2 | pkg.RT_FLAG_STREAM_ADAPTIVE | pkg.RT_FLAG_COUNT)
    assert rc == -1 and "RT_FLAG_STREAM is not available with RT_FLAG_COUNT" in msg
    rc, msg = _create_rc(pkg, pkg.RT_FLAG_STREAM | pkg.RT_FLAG_SIMPLE | ada2 | pkg.RT_FLAG_STREAM_ADAPTIVE)
    assert rc == -1 and "RT_FLAG_STREAM and RT_FLAG_SIMPLE exclude each other" in msg


def test_the_flag_gets_past_the_checks_with_adaptive_supersampling(pkg):
    import torch
    ada4 = pkg.RT_FLAG_SSAA4 | pkg.RT_FLAG_SSAA_ADAPTIVE | pkg.RT_FLAG_STREAM_ADAPTIVE
    for extra in (0, pkg.RT_FLAG_STREAM, pkg.RT_FLAG_SSAA_GEOMETRY, pkg.RT_FLAG_STREAM | pkg.RT_FLAG_SSAA_GEOMETRY | pkg.RT_FLAG_FAST, pkg.RT_FLAG_SIMPLE,
                  pkg.RT_FLAG_COUNT, pkg.RT_FLAG_STREAM_QUERIES):
        rc, msg = _create_rc(pkg, ada4 | extra)
        assert rc in (0, -4) and (rc == -4 or torch.cuda.is_available()), (extra, rc, msg)


def test_build_report_lists_the_new_kernel_without_spills():
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    lines = [l for l in open(report).read().splitlines() if re.search(r"\d\dray_list_stream_kernel", l)]
    for variant in ("strict", "fast"):
        mine = [l for l in lines if l.startswith(f"rt_stream_adaptive_{variant}.o")]
        assert len(mine) == 20, mine   # K = 1 <HAS_GQ, HAS_CUBIC>; K = 2 and 4 <RGBA8, HAS_GQ, HAS_CUBIC>
    assert len(lines) == 40
    for l in lines:
        assert re.search(r"VGPR spills\s+0\s+scratch 0\b", l), l
        assert int(re.search(r"occupancy\s+(\d+)", l).group(1)) >= 2, l   # what create_adaptive sizes the grids for (SA_WG_PER_CU)
    assert re.search(r"constexpr uint32_t SA_WG_PER_CU = 2;", open(os.path.join(CSRC, "rt_capi.cpp")).read())


def test_the_kernel_file_has_no_workgroup_barrier_and_no_dynamic_lds():
    def code_of(name):
        return "\n".join(l.split("//")[0] for l in open(os.path.join(CSRC, name)).read().splitlines())
    # the kernel's file, the shared loop with the policy over sq_query, the items and the resolve
    codes = {name: code_of(name) for name in ("rt_stream_adaptive.hip", "rt_stream_shade.hpp", "rt_stream_shell.hpp", "rt_ray_list.hpp")}
    for name, code in codes.items():
        assert "__syncthreads" not in code and "s_barrier" not in code and "rq_stage_tables" not in code and '"workgroup"' not in code, name
        assert "extern __shared__" not in code and "HIP_DYNAMIC_SHARED" not in code, name
    code = codes["rt_stream_adaptive.hip"]
    assert code.count("__shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];") == 1
    assert "__shared__" not in codes["rt_stream_shade.hpp"] and "__shared__" not in codes["rt_stream_shell.hpp"] and "__shared__" not in codes["rt_ray_list.hpp"]
    # both object loops go through sq_query without a block cone: the kernel has no query of its own, it runs the shared loop under the
    # policy over sq_query with the cone off; that policy has exactly one nearest-hit and one occlusion call, and the only cone argument
    # that is not the literal false is the policy's `cone`, which this kernel sets to false
    assert "sq_query<" not in code and "sc_query" not in code
    assert code.count("SqShade pol{qa, scene, slice, false};") == 1 and code.count("SqShade") == 1
    assert code.count("shade_loop<HAS_GQ, HAS_CUBIC>(fa, scene, lights, lane, pol, origin, it.dir, it.use);") == 1
    shade = codes["rt_stream_shade.hpp"]
    assert shade.count("sq_query<HAS_GQ, HAS_CUBIC, false>") == 1 and shade.count("sq_query<HAS_GQ, HAS_CUBIC, true>") == 1 and shade.count("sq_query<") == 2
    assert "sq_query<HAS_GQ, HAS_CUBIC, false>(qa, scene, slice, lane, o, d, use, k == 0u && cone, MAX_T, best_t, best);" in shade
    assert "sq_query<HAS_GQ, HAS_CUBIC, true>(qa, scene, slice, lane, so, sd, use, false, max_t, unused_t, blocked);" in shade
    # no lane leaves early: none of the three keywords inside the loop function -- except its final `return res;`, the last statement of
    # its body -- none in the policy's queries, none in the kernel, none in the items and the resolve
    loop = shade.split("F3 shade_loop(")[1].split("struct ShadeNoSegment")[0]
    assert loop.count("return") == 1 and re.search(r"\n    return res;\n}\s*$", loop.rstrip() + "\n") and "break" not in loop and "continue" not in loop
    policy = shade.split("struct SqShade {")[1]
    assert policy.count("return") == 1 and "return Segment{};" in policy and "break" not in policy and "continue" not in policy
    kernel = code.split("void ray_list_stream_kernel")[1].split("template <int K, bool RGBA8>\nstatic")[0]
    assert "return" not in kernel and "break" not in kernel and "continue" not in kernel
    assert "struct SlItem" not in codes["rt_stream_shell.hpp"] and '#include "rt_ray_list.hpp"' in codes["rt_stream_shell.hpp"]
    lists = codes["rt_ray_list.hpp"].split("struct SlItem {")[1]
    assert lists.count("return") == 1 and "    return it;\n" in lists and "break" not in lists and "continue" not in lists
    assert "rt_stream_adaptive" in open(os.path.join(ROOT, "cuda-ray-tracer_amd", "Makefile")).read()


# ---- the conditions of the GPU tests, on the oracle alone --------------------------------------------------------------------------------
def mirrors_bounce(osc):
    return osc.max_reflections > 0 and (np.asarray(osc.reflection) > 1e-7).any()


def check_samples(key, k, mask, last_object=False):
    """(b) some refined pixel has a sample whose primary hit lies in the first chunk of its table and some one in a last chunk (the
    highest-index object where asked); (f) where the scene has mirrors and a depth, a sample of a refined pixel bounces."""
    so = A.SampleOwners(key, k)
    osc = so.osc
    n = len(osc.reflection)
    refl = np.asarray(osc.reflection)
    want_bounce = mirrors_bounce(osc)

    if last_object:   # (thousands of objects: one intersection per sample instead of the nearest-hit loop)
        spheres = Q.tables(np.asarray(osc.coefs).reshape(-1, 20))["sphere"]
        assert len(spheres) > 8 * Q.CHUNK and so.pos[n - 1][1] == so.last[so.pos[n - 1][0]] and so.owns_sample_in(n - 1, mask), (key, k)
        assert any(so.owns_sample_in(o, mask) for o in spheres[:Q.CHUNK]), (key, k)
        assert not want_bounce
        return

    def enough(seen):
        return so.spans_first_and_last_chunk(seen) and (not want_bounce or any(refl[o] > 1e-7 for o in seen))
    seen = so.of_pixels(mask, enough)
    assert so.spans_first_and_last_chunk(seen), (key, k, sorted(seen)[:8])
    assert not want_bounce or any(refl[o] > 1e-7 for o in seen), (key, k)


@pytest.mark.parametrize("key", A.FORCED, ids=[" ".join(str(v) for v in key) for key in A.FORCED])
def test_forced_cases(pkg, key):
    """(a) at tau = 1/32 the refined set is neither empty nor the whole frame; (b), (f) by check_samples on the 2 x 2 samples."""
    p = A.frame(key)
    mask = ada.refine_mask(p, A.TAU)
    assert mask.any() and not mask.all(), key
    assert ada.refine_mask(p, 0.0).sum() >= mask.sum() and not ada.refine_mask(p, A.INF).any()
    check_samples(key, 2, mask)
    assert (A.frame(key, 2).shape[0], A.frame(key, 4).shape[1]) == (2 * p.shape[0], 4 * p.shape[1])


def test_some_forced_case_leaves_a_wave_partly_filled(pkg):
    """(c) per k, a refined count that is no multiple of the 64 / k^2 pixels of a wave."""
    counts = [int(ada.refine_mask(A.frame(key), A.TAU).sum()) for key in A.FORCED]
    assert any(c % 16 for c in counts) and any(c % 4 for c in counts), counts
    # ... and in the banded cases, per rank
    for key, world, band, k, _ in A.BANDS:
        per_rank = [int(A.banded_mask(A.frame(key), A.TAU, world, r, band)[1].sum()) for r in range(world)]
        assert any(c % (64 // (k * k)) for c in per_rank), (world, band, per_rank)


@pytest.mark.parametrize("case", A.BANDS, ids=[f"world{c[1]}-band{c[2]}" for c in A.BANDS])
def test_banded_cases(pkg, case):
    """(d) in every rank some pixel is refined only because of a halo-row neighbour; the halo rows include off-image ones (the first band
    of rank 0 starts at row 0) and the width is no multiple of a wave's 64 halo pixels, so waves straddle halo slots."""
    key, world, band, k, _ = case
    p = A.frame(key)
    h, w = p.shape[:2]
    assert h % (world * band) and w % 64 and (2 * w) % 64
    whole = ada.refine_mask(p, A.TAU)
    assert whole.any() and not whole.all()
    for rank in range(world):
        rows, with_halo = A.banded_mask(p, A.TAU, world, rank, band)
        _, without = A.banded_mask(p, A.TAU, world, rank, band, halo=False)
        assert np.array_equal(with_halo, whole[rows]), rank
        assert (with_halo & ~without).any(), (rank, "no pixel depends on a halo row")
    check_samples(key, k, whole)


def test_geometry_case(pkg):
    """(e) with tau = +inf the geometric mask is not empty, and min_cos = 0.9 refines a strict superset of the object-id edges; so per layout."""
    key = A.GEOMETRY
    p = A.frame(key)
    obj, nrm = A.planes(key)
    ids, turned = geo.geo_mask(obj, nrm, -A.INF), geo.geo_mask(obj, nrm, 0.9)
    assert ids.any() and not turned.all() and (turned & ~ids).any() and not (ids & ~turned).any()
    colour = ada.refine_mask(p, A.TAU)
    assert (colour & ~turned).any() or (turned & ~colour).any()   # the two terms are different sets
    for world, rank, band in A.GEO_LAYOUTS:
        for c in A.GEO_COSES:
            rows, m = A.banded_mask(p, A.INF, world, rank, band, obj, nrm, c)
            assert m.any() and not m.all() and np.array_equal(m, geo.geo_mask(obj, nrm, c)[rows]), (world, rank, c)
        if world > 1:   # (d) for the geometric term: an object edge that runs along a band edge is seen only through the halo records
            _, without = A.banded_mask(p, A.INF, world, rank, band, obj, nrm, -A.INF, halo=False)
            assert (A.banded_mask(p, A.INF, world, rank, band, obj, nrm, -A.INF)[1] & ~without).any(), (world, rank)
    check_samples(key, 2, turned)


def test_beyond_cases(pkg):
    """The three scenes beyond a limit: each is beyond the limit it is named for (and the 569-object one within the wavefront kernel's), (a)
    holds, and the highest-index object owns a sample of a refined pixel."""
    lds = pkg.lib().rt_wavefront_lds_bytes_strict
    lds.restype, lds.argtypes = C.c_size_t, [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_uint32]
    n_list = len(A.oracle_scene(A.BEYOND_LIST)[0].reflection)
    assert n_list == 569 and n_list * 288 > S.LDS_LIMIT >= (n_list - 1) * 288
    big = A.beyond_wavefront(pkg)
    n_big = len(A.oracle_scene(big)[0].reflection)
    assert n_big == S.first_count_beyond_lds(pkg) and lds(n_big * 80, 2, 0, n_big, 0, 0) > S.LDS_LIMIT >= lds(n_list * 80, 3, 0, n_list, 0, 0)
    n_geo = len(A.oracle_scene(A.BEYOND_GBUFFER)[0].reflection)
    assert n_geo == A.GEO_SPHERES == 2562 and n_geo * 64 > S.LDS_LIMIT
    for key in (A.BEYOND_LIST, big):
        mask = ada.refine_mask(A.frame(key), A.TAU)
        assert mask.any() and not mask.all(), key
        check_samples(key, 2, mask, last_object=True)
    obj, nrm = A.planes(A.BEYOND_GBUFFER)
    mask = ada.refine_mask(A.frame(A.BEYOND_GBUFFER), A.TAU) | geo.geo_mask(obj, nrm, 0.9)
    assert mask.any() and not mask.all() and geo.geo_mask(obj, nrm, -A.INF).any()
    check_samples(A.BEYOND_GBUFFER, 2, mask, last_object=True)
