"""The query kernels at every table size they accept: rt_render_gbuffer, rt_pick and rt_object_extents
(csrc/rt_gbuffer.hip: nearest_hit), rt_trace_rays and rt_occluded_rays (csrc/rt_rayquery.hpp: rq_tables), rt_shade_rays and
rt_trace_paths (the same loops) walk the class tables in LDS 64 entries at a time.  Here they run on tables of 64, 65, 129 and 193
entries of one class, on six degree-3 objects, and on the sizes only a streamed context allows, up to the 2 560 spheres whose table
is exactly the 160 KiB a workgroup can have.

Contexts are strict and every comparison of a scene of degree <= 2 is bit for bit, on integer views, against a CPU composer
(tests/tools/rays_ref.py, shade_ref.py, paths_ref.py, gbuffer_ref.py, extents_ref.py) or the oracle's frame; the cases that compare
device results with device results say so.  Scenes, seeds, target lists, aimed rays and rows come from tests/tools/query_table_scenes.py;
the conditions that keep these tests from being vacuous (the aimed rays own their targets in every chunk of every table, the blockers
span the chunks, the last chunks own pixels) are asserted on the composers alone in tests/test_query_tables_host.py for these very
inputs: the two files move together."""
import functools
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cubic_device_lab as D  # noqa: E402  (the oracle under the device's cbrt / acos / cos)
import extents_ref  # noqa: E402
import gbuffer_ref  # noqa: E402
import paths_ref  # noqa: E402
import query_table_scenes as Q  # noqa: E402
import raw_desc_scenes as R  # noqa: E402
import rays_ref  # noqa: E402
import shade_ref  # noqa: E402
import stream_scenes as S  # noqa: E402
import test_gbuffer_gpu as G  # noqa: E402
import test_paths_gpu as P  # noqa: E402
import test_rays_gpu as T  # noqa: E402
import test_shade_gpu as H  # noqa: E402
from test_extents_gpu import assert_same as assert_extents, from_planes  # noqa: E402
from test_rays_gpu import occluded_dev, rescaled, trace_dev  # noqa: E402
from test_stream_gpu import check_both_formats  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- what a case asks of a context -------------------------------------------------------------------------------------------------------
class Composed:
    """The composers' answers to a case's aimed rays, formed once per case and left unchanged."""

    def __init__(self, osc, rays, t_max):
        self.hits = rays_ref.closest(osc, rays)
        self.blocked, self.blocked_all = rays_ref.occluded(osc, rays, t_max), rays_ref.occluded(osc, rays)
        self.colours, self.first = shade_ref.shade(osc, rays, hits=True)
        self.paths = paths_ref.paths(osc, rays)


def check_ray_queries(r, c, want, what):
    """rt_trace_rays, rt_occluded_rays (the t_max array and NULL), rt_shade_rays (colour and the optional hit) and rt_trace_paths on the
    aimed rays of case `c` against `want`."""
    T.assert_records(trace_dev(r, c.rays), want.hits, (what, "rt_trace_rays"))
    T.assert_records(r.trace(c.rays["o"], c.rays["d"]), want.hits, (what, "rt_trace_rays_host"))
    assert np.array_equal(occluded_dev(r, c.rays, c.t_max), want.blocked), (what, "rt_occluded_rays, t_max")
    assert np.array_equal(occluded_dev(r, c.rays), want.blocked_all), (what, "rt_occluded_rays, NULL")
    got, rec = H.shade_dev(r, c.rays, hits=True)
    H.assert_colours(got, want.colours, (what, "rt_shade_rays"))
    H.assert_records_as_composer(rec, want.first, (what, "rt_shade_rays, hits"))
    H.assert_same_bits(H.shade_dev(r, c.rays)[0], got, (what, "rt_shade_rays without hits"))
    P.assert_composer(P.paths_dev(r, c.rays), want.paths, (what, "rt_trace_paths"))


def pick_records(ref):
    """The G-buffer composer's planes as rt_pick's records, in row-major order."""
    out = np.zeros(ref["object"].size, dtype=rays_ref.HIT_DTYPE)
    out["t"], out["object"] = ref["t"].reshape(-1), ref["object"].reshape(-1)
    out["point"], out["normal"] = ref["point"].reshape(-1, 3), ref["normal"].reshape(-1, 4)[:, :3]
    return out


def device_planes(r):
    o, t, n, ms = r.gbuffer()
    assert ms is not None and ms >= 0.0
    return o.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy()


def check_pixel_queries(r, osc, rows, rects, what):
    """The G-buffer's planes, rt_pick of every pixel and rt_object_extents of `rects` on the global rows `rows` (None: the whole frame)
    against the G-buffer composer and the reduction of ITS planes."""
    w, h = osc.width, osc.height
    ys = np.arange(h) if rows is None else np.asarray(rows)
    ref = gbuffer_ref.compose(osc, rows=ys)
    got = device_planes(r)
    assert got[0].shape == (h, w)
    G.assert_exact(tuple(p[ys] for p in got), ref, (what, "rt_render_gbuffer"))
    xy = np.stack([np.tile(np.arange(w), len(ys)), np.repeat(ys, w)], axis=1)
    T.assert_records(r.pick(xy), pick_records(ref), (what, "rt_pick"))
    n = len(osc.objects)
    for rect in rects:
        want = extents_ref.reduce_planes(ref["object"], ref["t"], n, np.arange(w), ys, rect)
        assert_extents(r.object_extents(None, rect), want, (what, "rt_object_extents", rect))
        assert rect is None or 0 < int(want["pixels"].sum()) < w * h
    return ref


def shade_of_primary(r):
    """rt_shade_rays on the rays rt_primary_rays forms for the context's frame."""
    import torch
    rays, _ = r.primary_rays()
    out = torch.empty((r.height, r.width, 4), dtype=torch.float32, device=rays.device)
    r.shade_into(rays.data_ptr(), r.height * r.width, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- a. chunk boundaries, one class at a time ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Q.SMALL, ids=lambda c: f"{c[1]} {c[0]}")
def test_chunk_boundaries(pkg, case):
    """64, 65, 129 and 193 spheres or general quadrics and 65 planes, every third (fourth) a mirror: the last chunk is full, holds a single
    entry behind one, two or three full ones.  One aimed ray per object at depths 0, 1 and 4; the planes, every pixel's pick and the
    extents of the 64 x 48 and the 37 x 21 frame (partial tiles and blocks) with the cone loop and with the plain loop
    (RT_FLAG_NOCULL); shade_rays(primary_rays) is the oracle's frame."""
    c = Q.small_case(pkg, case)
    for depth in Q.DEPTHS:
        osc = c.at_depth(depth)
        r = pkg.Renderer(c.sc.set_max_reflections(depth), device=0)
        assert not r.streamed
        check_ray_queries(r, c, Composed(osc, c.rays, c.t_max), (case, "depth", depth))
        r.cleanup_update()
    for w, h in Q.SIZES:
        cs = Q.small_case(pkg, case, w, h)
        ref = None
        for flags in (0, pkg.RT_FLAG_NOCULL):
            r = pkg.Renderer(cs.sc, device=0, flags=flags)
            if ref is None:
                ref = check_pixel_queries(r, cs.osc, None, (None, Q.RECTS_SMALL[(w, h)]), (case, w, h))
                got = shade_of_primary(r)
                assert np.all(got[..., 3] == 1.0) and R.same_as_oracle(got[..., :3], cs.osc.render(nthreads=8)), (case, w, h, "shade_rays(primary_rays)")
            else:
                G.assert_exact(device_planes(r), ref, (case, w, h, "RT_FLAG_NOCULL"))
                T.assert_records(r.pick(np.stack([np.tile(np.arange(w), h), np.repeat(np.arange(h), w)], axis=1)), pick_records(ref), (case, w, h, "rt_pick, RT_FLAG_NOCULL"))
                assert_extents(r.object_extents(), extents_ref.reduce_planes(ref["object"], ref["t"], len(cs.osc.objects), np.arange(w), np.arange(h)), (case, "NOCULL"))
            r.cleanup_update()


# ---- b. six degree-3 objects ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rt_trace_rays", "rt_shade_rays", "rt_trace_paths", "rt_occluded_rays", "pixels"])
def test_six_cubic_objects(pkg, oracle, which):
    """tests/test_cubic_gpu.py's scene with six degree-3 objects at 64 x 48: the fifth and sixth take the per-lane branch
    `j >= RT_CUB_AT_MAX` of nearest_hit.  The rescaled primary rays of the frame plus one aimed ray per object, to the bars of the
    existing degree-3 query tests (their cubic_check functions, imported).  rt_occluded_rays has no such test to take a bar from: its
    flags are held to the composer under the device's libm with the bound the frames and rt_shade_rays have, max(3, 0.2 % of the rays)
    -- a shadow decision that flips changes a colour, so it cannot ask for less than the colours do.  rt_pick and the extents are
    compared with the device's own planes, bit for bit."""
    c = Q.cubic_case(pkg)
    osc, sc = c.osc, c.sc
    assert np.isfinite(c.rays["d"]).all() and np.isfinite(c.rays["o"]).all() and (np.abs(c.rays["d"]).max(axis=1) > 0).all()
    rays = np.concatenate([rescaled(rays_ref.primary_rays(osc), 1), c.rays])
    if which == "rt_trace_rays":
        T.cubic_check(pkg, oracle, sc, osc, rays, "six cubics, rt_trace_rays")
    elif which == "rt_shade_rays":
        H.cubic_check(pkg, oracle, sc, osc, rays, "six cubics, rt_shade_rays")
    elif which == "rt_trace_paths":
        P.cubic_check(pkg, oracle, sc, osc, rays, "six cubics, rt_trace_paths")
    elif which == "rt_occluded_rays":
        r = pkg.Renderer(sc, device=0)
        # (the floor and the surfaces close the view: with K_MAX_T every primary ray is blocked, so half of them end 0.5 .. 1.5 times as
        # far as their closest hit under glibc)
        n, rng = len(rays) - len(c.rays), np.random.default_rng(Q.TMAX_SEED)
        first = rays_ref.closest(osc, rays[:n])["t"]
        t_max = np.concatenate([np.where((rng.random(n) < 0.5) & np.isfinite(first), first * rng.uniform(0.5, 1.5, n), Q.K_MAX_T), c.t_max])
        got = occluded_dev(r, rays, t_max)
        r.cleanup_update()
        ref, _, rounds = oracle.under_libm(lambda: rays_ref.occluded(osc, rays, t_max), D.evaluator(D.lib(pkg)))
        print(f"six cubics, rt_occluded_rays: {int((got != ref).sum())} of {len(rays)} flags differ from the device-libm composer ({int(ref.sum())} blocked), libm rounds {rounds}")
        assert int((got != ref).sum()) <= max(3, int(0.002 * len(rays))) and len(rays) // 10 < ref.sum() < len(rays) - len(rays) // 10
    else:
        G.cubic_check(pkg, oracle, sc, osc, None, "six cubics, rt_render_gbuffer")
        r = pkg.Renderer(sc, device=0)
        o, t, n = device_planes(r)
        w, h = osc.width, osc.height
        rec = r.pick(np.stack([np.tile(np.arange(w), h), np.repeat(np.arange(h), w)], axis=1))
        assert np.array_equal(rec["object"], o.reshape(-1)) and np.array_equal(rec["t"].view(np.uint64), t.reshape(-1).view(np.uint64))
        assert np.array_equal(np.ascontiguousarray(rec["normal"]).view(np.uint32), n.reshape(-1, 4)[:, :3].view(np.uint32))
        assert np.isin(o, Q.tables(c.coefs)["cubic"][4:]).any()
        for rect in (None, Q.RECTS_SMALL[(64, 48)]):
            assert_extents(r.object_extents(None, rect), from_planes(r, None, rect), ("six cubics", rect))
        r.cleanup_update()


# ---- c. the sizes a streamed context allows ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large(name):
    import __graft_entry__ as graft
    return Q.large_case(graft.load_package(), name)


@pytest.mark.parametrize("name", Q.LARGE)
def test_large_tables(pkg, name):
    """The largest scene the wavefront frame kernel takes (its frame is rendered and is the oracle's in both formats: the largest LDS that
    kernel is ever given), the first scene beyond it with a large sphere appended, about 2 000 spheres, ellipsoids and planes
    (160 096 table bytes), and 2 560 spheres, whose table is exactly the 163 840 bytes of LDS a workgroup can have (the extents then take
    the path without LDS accumulators).  The aimed rays go to the first and last entry of every chunk and to three more per chunk; the
    planes, the picks and the extents are compared on eight rows of the 64 x 48 frame."""
    c = large(name)
    want = Composed(c.osc, c.rays, c.t_max)
    if name == Q.LARGE[0]:
        check_both_formats(pkg, c.sc, c.osc.render(nthreads=8), name, flags=0, expect_streamed=False)
    r = pkg.Renderer(c.sc, device=0)
    assert r.streamed == (name != Q.LARGE[0])
    check_ray_queries(r, c, want, name)
    check_pixel_queries(r, c.osc, Q.ROWS, Q.RECTS_LARGE, name)
    r.cleanup_update()


def test_one_sphere_more_is_refused_by_every_query(pkg):
    """2 561 spheres: each of the seven entry points answers RT_ERR_SCENE (-2) under its own name, and the frame still renders."""
    import torch
    sc = S.field(pkg, Q.QUERY_LIMIT_SPHERES + 1, S.LARGE_SEED)
    r = pkg.Renderer(sc, device=0)
    try:
        assert r.streamed
        rays = torch.zeros((8, 6), dtype=torch.float64, device="cuda:0")
        rays[:, 5] = 1.0
        hits, last = (torch.zeros((8, 6), dtype=torch.float64, device="cuda:0") for _ in range(2))
        rgba = torch.zeros((8, 4), dtype=torch.float32, device="cuda:0")
        flags, ends = torch.zeros((8,), dtype=torch.int32, device="cuda:0"), torch.zeros((8, 4), dtype=torch.int32, device="cuda:0")
        ext = torch.zeros((Q.QUERY_LIMIT_SPHERES + 1, 5), dtype=torch.int64, device="cuda:0")
        calls = (("rt_render_gbuffer", r.gbuffer), ("rt_pick", lambda: r.pick([(1, 1)])),
                 ("rt_object_extents", lambda: r.object_extents_into(None, None, ext.data_ptr())),
                 ("rt_trace_rays", lambda: r.trace_into(rays.data_ptr(), 8, hits.data_ptr())),
                 ("rt_occluded_rays", lambda: r.occluded_into(rays.data_ptr(), None, 8, flags.data_ptr())),
                 ("rt_shade_rays", lambda: r.shade_into(rays.data_ptr(), 8, rgba.data_ptr())),
                 ("rt_trace_paths", lambda: r.paths_into(rays.data_ptr(), 8, 1, hits.data_ptr(), last.data_ptr(), ends.data_ptr())))
        for who, call in calls:
            with pytest.raises(pkg.RtError) as e:
                call()
            assert e.value.code == -2 and re.match(rf"{who}: scene needs \d+ bytes of LDS per workgroup \(limit 160 KiB\)", e.value.message), (who, e.value.message)
        r.update()
        got = r.download()
        assert np.all(got[..., 3] == 1.0) and R.same_as_oracle(got[..., :3], S.oracle_of(pkg, sc).render(nthreads=8))
    finally:
        r.cleanup_update()


# ---- d. context kinds ------------------------------------------------------------------------------------------------------------------------
def test_a_simple_context_beyond_its_limit_answers_as_the_default_one(pkg):
    """RT_FLAG_SIMPLE on the scene that is streamed by size: streamed too, and the same bits for every aimed ray (device against
    device; the default context is held to the composers by test_large_tables)."""
    c = large(Q.LARGE[1])
    a, b = pkg.Renderer(c.sc, device=0), pkg.Renderer(c.sc, device=0, flags=pkg.RT_FLAG_SIMPLE)
    try:
        assert a.streamed and b.streamed
        T.assert_records(trace_dev(b, c.rays), trace_dev(a, c.rays), "rt_trace_rays")
        assert np.array_equal(occluded_dev(b, c.rays, c.t_max), occluded_dev(a, c.rays, c.t_max)) and np.array_equal(occluded_dev(b, c.rays), occluded_dev(a, c.rays))
        (ca, ra), (cb, rb) = H.shade_dev(a, c.rays, hits=True), H.shade_dev(b, c.rays, hits=True)
        H.assert_same_bits(cb, ca, "rt_shade_rays")
        assert P.bits_equal(rb, ra)
        for x, y in zip(P.paths_dev(b, c.rays), P.paths_dev(a, c.rays)):
            assert P.bits_equal(x, y), "rt_trace_paths"
    finally:
        a.cleanup_update()
        b.cleanup_update()


# ---- e. after a scene update -------------------------------------------------------------------------------------------------------------------
def test_after_rt_set_scene_the_queries_are_the_moved_scenes(pkg):
    """Every sphere of the scene that is streamed by size moved (tests/test_stream_gpu.py: test_set_scene_moves_the_large_field): trace,
    occluded, gbuffer and object_extents of the updated context equal a fresh context's on the moved scene bit for bit (device against
    device), and the aimed rays equal the composers on the moved scene."""
    sc, coefs, c = Q.moved_case(pkg)
    r, fresh = pkg.Renderer(sc, device=0), pkg.Renderer(c.sc, device=0)
    try:
        assert r.streamed and fresh.streamed
        before = trace_dev(r, c.rays)
        r.set_scene(coefs=coefs)
        got = trace_dev(r, c.rays)
        assert not rays_ref.same_records(got, before)
        T.assert_records(got, trace_dev(fresh, c.rays), "rt_trace_rays")
        assert np.array_equal(occluded_dev(r, c.rays, c.t_max), occluded_dev(fresh, c.rays, c.t_max)) and np.array_equal(occluded_dev(r, c.rays), occluded_dev(fresh, c.rays))
        assert G.same_bits(device_planes(r), device_planes(fresh))
        assert_extents(r.object_extents(), fresh.object_extents(), "rt_object_extents")
        T.assert_records(got, rays_ref.closest(c.osc, c.rays), "rt_trace_rays against the composer")
        assert np.array_equal(occluded_dev(r, c.rays, c.t_max), rays_ref.occluded(c.osc, c.rays, c.t_max))
        assert np.array_equal(occluded_dev(r, c.rays), rays_ref.occluded(c.osc, c.rays))
    finally:
        r.cleanup_update()
        fresh.cleanup_update()


# ---- f. the FAST build, once ---------------------------------------------------------------------------------------------------------------------
def test_fast_build_statistics(pkg):
    """FAST against strict (device against device) on the 129-quadric and the 193-sphere field: `object` of rt_trace_rays (the aimed
    rays and the frame's primary rays) and of the G-buffer agree on at least 99 %, the bar of test_rays_gpu.py::test_fast_build_statistics;
    the figures are printed as there."""
    for case in (("quadric", 129), ("sphere", 193)):
        c = Q.small_case(pkg, case)
        rays = np.concatenate([c.rays, rays_ref.primary_rays(c.osc)])
        ra, rb = pkg.Renderer(c.sc, device=0), pkg.Renderer(c.sc, device=0, flags=pkg.RT_FLAG_FAST)
        a, b = trace_dev(ra, rays), trace_dev(rb, rays)
        pa, pb = device_planes(ra), device_planes(rb)
        ra.cleanup_update()
        rb.cleanup_update()
        both = (a["object"] >= 0) & (b["object"] >= 0)
        rel = np.abs(a["t"][both] - b["t"][both]) / np.abs(a["t"][both])
        agree, agree_planes = float((a["object"] == b["object"]).mean()), float((pa[0] == pb[0]).mean())
        print(f"FAST vs strict, {case[1]} {case[0]} field: rt_trace_rays object differs at {int((a['object'] != b['object']).sum())} of {len(rays)} rays "
              f"({100 * agree:.3f} % agree), max rel t difference {float(rel.max()):.3e}; G-buffer object differs at {int((pa[0] != pb[0]).sum())} of {pa[0].size} pixels "
              f"({100 * agree_planes:.3f} % agree)")
        assert agree >= 0.99 and agree_planes >= 0.99, (case, agree, agree_planes)
        assert both.any() and a["object"].max() >= 128
