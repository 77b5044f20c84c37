"""Every kernel past 64 degree-3 objects ("More than 64 degree-3 objects").  The streamed kernels walk the degree-3
class table as an index list staged through LDS 64 entries at a time (csrc/rt_stream.hpp: sq_tables, the HAS_CUBIC block); the staged
ones walk it in plain loops (csrc/rt_rayquery.hpp: rq_tables; csrc/rt_wavefront.hip: S.cub[j]).  The scenes are the fields of bent
ellipsoids of tests/tools/cubic_field_scenes.py with 64, 65 and 129 of them: one exactly full chunk, one entry behind a full chunk,
three chunks.

The sharp assertions compare device results with each other bit for bit -- a dropped or repeated chunk, or an early exit between chunks,
cannot survive them: the streamed frame against rt_shade_rays(rt_primary_rays) (the staged rq_tables), culled frames against the
unculled one, adaptive passes against the full supersampled frame, streamed queries against the staged ones, the staged frame kernels
against each other.  Against the oracle, degree 3 is held at the project's bar: no pixel beyond 1e-5 under the device's cbrt / acos /
cos.  The conditions that keep all this from being vacuous are asserted on the oracle alone in tests/test_cubic_chunks_host.py for
these very scenes (F.SEED, F.SCENES): the two files move together."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, compare

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cubic_device_lab as D  # noqa: E402  (the oracle under the device's cbrt / acos / cos)
import cubic_field_scenes as F  # noqa: E402
import query_table_scenes as Q  # noqa: E402
import raw_desc_scenes as R  # noqa: E402
import rays_ref  # noqa: E402
import ssaa_ref  # noqa: E402
from test_raw_descriptor_gpu import rgba8_of  # noqa: E402
from test_ssaa_adaptive_gpu import ada_flags, kflag  # noqa: E402
from test_stream_gpu import shade_of_primary  # noqa: E402
from test_stream_queries_gpu import all_pixels, assert_same_outputs, assert_within_one_context, forced, pixel_outputs, ray_outputs  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = ("64", "65", "129")
TAU = 1.0 / 32.0    # the mid threshold of the adaptive tests (tests/tools/stream_adaptive_scenes.py)


@functools.lru_cache(maxsize=None)
def osc_of(name):
    return F.scene(name)


def frame(pkg, osc, flags, fmt=None, expect=()):
    """One frame of a context; `expect`: (getter, value) pairs the context must report."""
    r = pkg.Renderer(R.desc(pkg, osc), device=0, flags=flags, **({} if fmt is None else dict(fmt=fmt)))
    try:
        for getter, value in expect:
            assert getattr(r, getter) == value, (getter, getattr(r, getter))
        r.update()
        return r.download().copy()
    finally:
        r.cleanup_update()


def assert_quantised(got8, got32, what):
    """The RGBA8 frame is the stated quantisation of the RGBA32F frame."""
    q, ok = rgba8_of(got32)
    assert got8.dtype == np.uint8 and ok.all() and np.array_equal(got8[..., :3], q[..., :3]) and np.all(got8[..., 3] == 255), what


def streamed_against_the_staged_tables(pkg, osc, what):
    """RT_FLAG_STREAM's frame == rt_shade_rays(rt_primary_rays) of the same context, bit for bit; RGBA8 its quantisation."""
    r = pkg.Renderer(R.desc(pkg, osc), device=0, flags=pkg.RT_FLAG_STREAM)
    try:
        assert r.streamed
        r.update()
        got, want = r.download().copy(), shade_of_primary(pkg, r)
    finally:
        r.cleanup_update()
    print(what, "pixels that differ from rt_shade_rays(rt_primary_rays):", R.n_diff(got, want))
    assert np.all(got[..., 3] == 1.0) and R.same(got, want), (what, R.n_diff(got, want))
    assert_quantised(frame(pkg, osc, pkg.RT_FLAG_STREAM, fmt=pkg.RT_FMT_RGBA8), got, what)
    return got


# ---- streamed frames, strict -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", COUNTS)
def test_streamed_frame(pkg, name):
    """64, 65 and 129 degree-3 objects.  Against the oracle under the device's libm no pixel is beyond 1e-5; the count against the glibc
    oracle is printed, not asserted -- the max(3, 0.2 %) allowance of tests/test_stream_gpu.py was sized for one to six degree-3 objects
    per frame (measured: DESIGN.md section 8)."""
    osc = osc_of(name)
    got = streamed_against_the_staged_tables(pkg, osc, name)
    c = compare(got[..., :3], osc.render(nthreads=8))
    print(f"{name}: against the glibc oracle {c['n_bad_pixels']} of {osc.width * osc.height} pixels beyond 1e-5 (max rel {c['max_rel']:.3e})")
    c = D.compare_device_libm(pkg, got[..., :3], osc)
    print(f"{name}: against the device-libm oracle {c}")
    assert c["n_bad_pixels"] == 0, c


@pytest.mark.parametrize("name", ["65 quadric", "65 37x21"])
def test_streamed_frame_with_a_quadric_and_with_partial_blocks(pkg, name):
    """The <1, 1> instantiation (one ellipsoid with cross terms), and a 37 x 21 frame, which has partial tiles and 8 x 8 blocks."""
    streamed_against_the_staged_tables(pkg, osc_of(name), name)


# ---- culled frames, strict and RT_FLAG_FAST -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["65 spheres", "65 spheres quadric", "129 spheres"])
def test_culled_frames(pkg, name):
    """With the 65-sphere field the culling decisions are true (rest.n_us = 0 hands the degree-3 table to the same loop).  Strict: the
    STREAM | STREAM_CULL and STREAM | STREAM_CULL | STREAM_CULL_BOUNCE frames equal the RT_FLAG_STREAM frame, which equals
    rt_shade_rays(rt_primary_rays), bit for bit.  FAST: the culled and bounce-culled frames equal the unculled FAST frame bit for bit,
    and that one is held against the strict frame at the project's FAST bar (max(2, 0.2 % of the pixels) beyond 1e-5)."""
    f, osc = pkg, osc_of(name)
    cull, bounce = f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_CULL, f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_CULL | f.RT_FLAG_STREAM_CULL_BOUNCE
    plain = streamed_against_the_staged_tables(pkg, osc, name)
    a = frame(pkg, osc, cull, expect=(("streamed", True), ("stream_cull", True), ("stream_cull_bounce", False)))
    assert R.same(a, plain), (name, "RT_FLAG_STREAM_CULL", R.n_diff(a, plain))
    b = frame(pkg, osc, bounce, expect=(("stream_cull", True), ("stream_cull_bounce", True)))
    assert R.same(b, plain), (name, "RT_FLAG_STREAM_CULL_BOUNCE", R.n_diff(b, plain))
    fast = frame(pkg, osc, f.RT_FLAG_STREAM | f.RT_FLAG_FAST, expect=(("stream_cull", False),))
    a = frame(pkg, osc, cull | f.RT_FLAG_FAST, expect=(("stream_cull", True),))
    assert R.same(a, fast), (name, "FAST, RT_FLAG_STREAM_CULL", R.n_diff(a, fast))
    b = frame(pkg, osc, bounce | f.RT_FLAG_FAST, expect=(("stream_cull_bounce", True),))
    assert R.same(b, fast), (name, "FAST, RT_FLAG_STREAM_CULL_BOUNCE", R.n_diff(b, fast))
    c = compare(fast[..., :3], plain[..., :3])
    print(f"{name}: FAST against strict {c}")
    assert c["n_bad_pixels"] <= max(2, int(0.002 * osc.width * osc.height)), (name, c)


# ---- streamed adaptive passes --------------------------------------------------------------------------------------------------------------
def test_streamed_adaptive_passes(pkg):
    """STREAM | SSAA2 | SSAA_ADAPTIVE | STREAM_ADAPTIVE with and without STREAM_CULL on 65 degree-3 objects and the sphere field: at
    tau < 0 every pixel is refined and the frame is the STREAM | SSAA2 frame bit for bit -- itself the exact resolve of the 128 x 96
    streamed frame, which is held to the staged tables; at a mid tau the culled and unculled frames and
    rt_get_ssaa_refined are identical, and the refined set is neither empty nor everything."""
    osc = osc_of("65 spheres")
    un = pkg.RT_FLAG_STREAM | ada_flags(pkg, 2, pkg.RT_FLAG_STREAM_ADAPTIVE)
    full = frame(pkg, osc, pkg.RT_FLAG_STREAM | kflag(pkg, 2))
    # (the anchor: the supersampled frame is the resolve of the plain streamed frame of the 2 x finer grid, and that one is
    # rt_shade_rays(rt_primary_rays) -- without it every frame of this test runs the same streamed loop and they could all be wrong alike)
    fine = streamed_against_the_staged_tables(pkg, osc.with_size(2 * osc.width, 2 * osc.height), "65 spheres, 128 x 96")
    assert R.same(full, ssaa_ref.resolve(fine, 2)), R.n_diff(full, ssaa_ref.resolve(fine, 2))
    out = {}
    for flags, decision in ((un, False), (un | pkg.RT_FLAG_STREAM_CULL, True)):
        r = pkg.Renderer(R.desc(pkg, osc), device=0, flags=flags)
        try:
            assert r.streamed_adaptive and r.stream_cull_adaptive is decision
            for tau in (-1.0, TAU):
                r.set_ssaa_threshold(tau)
                r.update()
                out[(decision, tau)] = (r.download().copy(), r.refined)
        finally:
            r.cleanup_update()
    for decision in (False, True):
        got, n = out[(decision, -1.0)]
        assert n == osc.width * osc.height and R.same(got, full), (decision, n, R.n_diff(got, full))
    (a, na), (b, nb) = out[(False, TAU)], out[(True, TAU)]
    print(f"adaptive, tau 1/32: {na} of {osc.width * osc.height} pixels refined")
    assert R.same(a, b) and na == nb and 0 < na < osc.width * osc.height, (na, nb, R.n_diff(a, b))


# ---- streamed queries ----------------------------------------------------------------------------------------------------------------------
def oracle_primary_hits(pkg, osc):
    """The reference's nearest hit of every primary ray under the device's cbrt / acos / cos, as rays_ref.closest forms it -- from the
    records of tests/tools/cubic_guard_lab.cpp (every primary ray against every degree-3 object, in pixel then object order), which the
    oracle answers at C speed.  For scenes of degree-3 objects alone."""
    rays, where = D.enumerate_rays(osc)
    rays = rays[where["kind"] == 0]
    n, h, w = len(osc.objects), osc.height, osc.width
    assert len(rays) == h * w * n and np.array_equal(rays["obj"].reshape(h * w, n)[0], np.arange(n))
    (t, _, _), _, rounds = D.oracle_rays_device_libm(D.lib(pkg), osc, rays)
    t = np.where((t >= F.K_EPS) & (t < F.K_MAX_T), t, np.inf).reshape(h * w, n)
    best = t.argmin(axis=1)           # (the first of equal roots, as `t < best_t` keeps it)
    out = np.zeros(h * w, dtype=rays_ref.HIT_DTYPE)
    out["t"], out["object"] = t[np.arange(h * w), best], np.where(np.isfinite(t.min(axis=1)), best, -1)
    coefs, dp = osc.coefs, C.POINTER(C.c_double)
    p, nv = np.zeros(3), np.zeros(3)
    first = rays.reshape(h * w, n)[:, 0]
    for i in np.flatnonzero(out["object"] >= 0).tolist():
        p[:] = first["o"][i] + np.float64(out["t"][i]) * first["d"][i]
        F.O.lib().orc_normal_vector(coefs[out["object"][i]].ctypes.data_as(dp), p.ctypes.data_as(dp), nv.ctypes.data_as(dp))
        out["point"][i], out["normal"][i] = p, nv.astype(np.float32)
    return out, rounds


def assert_trace_at_the_degree_3_bar(got, ref, what):
    """tests/test_rays_gpu.py: cubic_check's assertions -- the object equal at every ray, t within 1e-8 relative, the normals by
    conftest.compare, no ray left out."""
    nobj = int((got["object"] != ref["object"]).sum())
    hit = ref["object"] >= 0
    rel = np.abs(got["t"][hit] - ref["t"][hit]) / np.abs(ref["t"][hit])
    c = compare(got["normal"], ref["normal"])
    print(f"{what}: object differs at {nobj} of {len(ref)} rays, max rel t {float(rel.max()) if rel.size else 0.0:.3e}, normals {c}")
    assert nobj == 0, what
    assert np.array_equal(np.isposinf(got["t"]), ~hit)
    assert np.all(rel <= 1e-8), (what, float(rel.max()))
    assert c["n_bad_pixels"] == 0, (what, c)
    assert hit.any()


@pytest.mark.parametrize("name", COUNTS)
def test_streamed_queries(pkg, oracle, name):
    """RT_FLAG_STREAM | RT_FLAG_STREAM_QUERIES against the unflagged context (the staged kernels), as
    tests/test_stream_queries_gpu.py::test_six_cubic_objects_forced: the frame's primary rays plus one ray aimed at each body;
    rt_trace_rays, rt_occluded_rays, rt_shade_rays, rt_trace_paths / rt_pick_paths, every G-buffer plane, rt_pick on every pixel and
    rt_object_extents of the whole frame and of one rectangle, bit for bit.  The G-buffer shows positions below RT_CUB_AT_MAX (the
    host's records: HOST_CUB), within 4 .. 63 and, past one chunk, beyond 63.  The trace records are held to the oracle's nearest hit
    under the device's libm at the bar of the degree-3 query tests."""
    osc = osc_of(name)
    w, h = osc.width, osc.height
    aimed = F.aimed_rays(osc)
    rays = np.concatenate([rays_ref.primary_rays(osc), aimed])
    rng = np.random.default_rng(Q.TMAX_SEED)
    t_max = np.where(rng.random(len(rays)) < 0.5, Q.K_MAX_T, rng.uniform(5.0, 60.0, len(rays)))
    rects, xy = (None, Q.RECTS_SMALL[(w, h)]), all_pixels(w, h)
    sc = R.desc(pkg, osc)
    r, plain = pkg.Renderer(sc, device=0, flags=forced(pkg)), pkg.Renderer(sc, device=0)
    try:
        assert r.streamed and r.streamed_queries and not plain.streamed and not plain.streamed_queries
        got = ray_outputs(r, rays, t_max)
        assert_same_outputs(got, ray_outputs(plain, rays, t_max), name)
        px = pixel_outputs(r, rects, xy)
        assert_same_outputs(px, pixel_outputs(plain, rects, xy), name)
        assert_within_one_context(r, px, xy, name, plane0=False)
    finally:
        r.cleanup_update()
        plain.cleanup_update()
    table = np.array(Q.tables(osc.coefs)["cubic"])
    seen = px["object"]
    assert np.isin(seen, table[:F.RT_CUB_AT_MAX]).any() and np.isin(seen, table[F.RT_CUB_AT_MAX:F.CHUNK]).any()
    assert np.isin(seen, table[F.CHUNK:]).any() == (len(table) > F.CHUNK)
    blocked = got["rt_occluded_rays, t_max"]
    assert 0 < int(blocked.sum()) < len(rays) and (got["rt_trace_rays"]["object"][-len(aimed):] >= 0).any()
    ref, rounds = oracle_primary_hits(pkg, osc)
    assert_trace_at_the_degree_3_bar(got["rt_trace_rays"][:w * h], ref, f"{name}, primary rays (libm rounds {rounds})")
    ref, _, rounds = oracle.under_libm(lambda: rays_ref.closest(osc, aimed), D.evaluator(D.lib(pkg)))
    assert_trace_at_the_degree_3_bar(got["rt_trace_rays"][w * h:], ref, f"{name}, aimed rays (libm rounds {rounds})")


# ---- the staged kernels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["65", "129"])
def test_staged_frame_kernels(pkg, name):
    """The wavefront kernel's S.cub[j] loops (nearest hit and shadow phases) and the simple kernel, all of whose work for
    j >= RT_CUB_AT_MAX had been run for two objects only: the default, RT_FLAG_SIMPLE and RT_FLAG_NOCULL frames equal each other bit for
    bit, the RT_FLAG_COUNT frame equals the product frame, and the default frame has no pixel beyond 1e-5 against the oracle under the
    device's libm."""
    osc = osc_of(name)
    sc = R.desc(pkg, osc)
    got = R.render_desc(pkg, sc)
    for what, flags in (("RT_FLAG_SIMPLE", pkg.RT_FLAG_SIMPLE), ("RT_FLAG_NOCULL", pkg.RT_FLAG_NOCULL), ("RT_FLAG_COUNT", pkg.RT_FLAG_COUNT)):
        other = frame(pkg, osc, flags, expect=(("streamed", False),))
        assert R.same(got, other), (name, what, R.n_diff(got, other))
    c = D.compare_device_libm(pkg, got[..., :3], osc)
    print(f"{name}, staged: against the device-libm oracle {c}")
    assert c["n_bad_pixels"] == 0, c
