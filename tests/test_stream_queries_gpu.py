"""The streamed query kernels (RT_FLAG_STREAM_QUERIES, csrc/rt_stream_queries.hip): rt_render_gbuffer, rt_pick,
rt_object_extents, rt_trace_rays, rt_occluded_rays, rt_shade_rays, rt_trace_paths and rt_pick_paths with the class tables streamed through
a wave-private LDS slice, on scenes of any size.

Contexts are strict unless a case says otherwise.  "Forced" is RT_FLAG_STREAM | RT_FLAG_STREAM_QUERIES, which gives a small scene the
streamed query kernels; every case asserts Renderer.streamed_queries.  A comparison is bit for bit, either against the CPU composers
(the checks of tests/test_query_tables_gpu.py, imported) or against a context without the flag, which runs the staged kernels (device
against device).  Scenes, aimed rays and rows come from tests/tools/query_table_scenes.py and, beyond the 160 KiB limit, from
tests/tools/stream_query_scenes.py; the conditions that keep these tests from being vacuous are asserted on the composers alone in
tests/test_query_tables_host.py and tests/test_stream_queries_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import extents_ref  # noqa: E402
import gbuffer_ref  # noqa: E402
import query_table_scenes as Q  # noqa: E402
import rays_ref  # noqa: E402
import stream_query_scenes as B  # noqa: E402
import test_paths_gpu as P  # noqa: E402
import test_shade_gpu as H  # noqa: E402
from test_extents_gpu import assert_same as assert_extents, from_planes, n_objects  # noqa: E402
from test_query_tables_gpu import Composed, check_pixel_queries, check_ray_queries, device_planes, large, pick_records, shade_of_primary  # noqa: E402
from test_rays_gpu import occluded_dev, to_device, trace_dev  # noqa: E402

pytestmark = pytest.mark.gpu


def flag(pkg):
    return pkg.RT_FLAG_STREAM_QUERIES


def forced(pkg):
    return pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_QUERIES


def all_pixels(w, h):
    return np.stack([np.tile(np.arange(w), h), np.repeat(np.arange(h), w)], axis=1)


def ray_outputs(r, rays, t_max):
    """Every output of the four ray entry points on `rays`, by name."""
    out = {"rt_trace_rays": trace_dev(r, rays), "rt_occluded_rays, t_max": occluded_dev(r, rays, t_max), "rt_occluded_rays, NULL": occluded_dev(r, rays)}
    out["rt_shade_rays"], out["rt_shade_rays, hits"] = H.shade_dev(r, rays, hits=True)
    out["rt_trace_paths, segments"], out["rt_trace_paths, last"], out["rt_trace_paths, ends"] = P.paths_dev(r, rays)
    return out


def pixel_outputs(r, rects, xy):
    """The planes, rt_pick and rt_pick_paths of the pixels xy and rt_object_extents of every rectangle, by name."""
    o, t, n = device_planes(r)
    out = {"object": o, "t": t, "normal": n, "rt_pick": r.pick(xy)}
    out["rt_pick_paths, segments"], out["rt_pick_paths, ends"] = r.pick_paths(xy)
    for rect in rects:
        out[("rt_object_extents", rect)] = r.object_extents(None, rect)
    return out


def assert_same_outputs(got, want, what):
    assert got.keys() == want.keys()
    for key in got:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, key)


def assert_within_one_context(r, px, xy, what, plane0=True):
    """The promises inside one context: rt_pick is the planes' entry, rt_object_extents the reduction of the planes, and plane 0 of
    rt_pick_paths is rt_pick (degree <= 2)."""
    at = (xy[:, 1], xy[:, 0])
    rec = px["rt_pick"]
    assert np.array_equal(rec["object"], px["object"][at]) and np.array_equal(rec["t"].view(np.uint64), px["t"][at].view(np.uint64)), (what, "rt_pick")
    assert np.array_equal(np.ascontiguousarray(rec["normal"]).view(np.uint32), np.ascontiguousarray(px["normal"][at][:, :3]).view(np.uint32)), (what, "rt_pick, normal")
    for key in px:
        if isinstance(key, tuple):
            assert_extents(px[key], extents_ref.reduce_planes(px["object"], px["t"], n_objects(r), np.arange(r.width), r.row_map(), key[1]), (what, key))
    if plane0:
        seg0 = px["rt_pick_paths, segments"][0]
        assert np.array_equal(seg0["object"], rec["object"]) and np.array_equal(seg0["t"].view(np.uint64), rec["t"].view(np.uint64)), (what, "rt_pick_paths, plane 0")


# ---- 1. chunk boundaries, forced ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Q.SMALL, ids=lambda c: f"{c[1]} {c[0]}")
def test_chunk_boundaries_forced(pkg, case):
    """64, 65, 129 and 193 spheres or general quadrics and 65 planes: the last chunk is full, or holds a single entry behind one, two or
    three full ones.  The checks of tests/test_query_tables_gpu.py::test_chunk_boundaries on a forced context, and every output equal
    to the unflagged context's."""
    c = Q.small_case(pkg, case)
    for depth in Q.DEPTHS:
        osc = c.at_depth(depth)
        sc = c.sc.set_max_reflections(depth)
        r, plain = pkg.Renderer(sc, device=0, flags=forced(pkg)), pkg.Renderer(sc, device=0)
        try:
            assert r.streamed and r.streamed_queries and not plain.streamed_queries
            check_ray_queries(r, c, Composed(osc, c.rays, c.t_max), (case, "depth", depth))
            assert_same_outputs(ray_outputs(r, c.rays, c.t_max), ray_outputs(plain, c.rays, c.t_max), (case, "depth", depth))
        finally:
            r.cleanup_update()
            plain.cleanup_update()
    for w, h in Q.SIZES:
        cs = Q.small_case(pkg, case, w, h)
        rects, xy = (None, Q.RECTS_SMALL[(w, h)]), all_pixels(w, h)
        for extra in (0, pkg.RT_FLAG_NOCULL):
            r, plain = pkg.Renderer(cs.sc, device=0, flags=forced(pkg) | extra), pkg.Renderer(cs.sc, device=0, flags=extra)
            try:
                assert r.streamed_queries and not plain.streamed_queries
                check_pixel_queries(r, cs.osc, None, rects, (case, w, h, extra))
                px = pixel_outputs(r, rects, xy)
                assert_same_outputs(px, pixel_outputs(plain, rects, xy), (case, w, h, extra))
                assert_within_one_context(r, px, xy, (case, w, h, extra))
            finally:
                r.cleanup_update()
                plain.cleanup_update()


# ---- 2. six degree-3 objects, forced -------------------------------------------------------------------------------------------------------------
def test_six_cubic_objects_forced(pkg):
    """Two of the six degree-3 objects lie beyond RT_CUB_AT_MAX: the pixel family takes the host's records at the frame's origin for the
    first four and forms the other two's per lane, as the staged kernels do.  Every entry point equals the unflagged context's, bit for bit
    (the aimed rays and the frame's primary rays; every pixel, the whole frame and a rectangle)."""
    c = Q.cubic_case(pkg)
    w, h = c.osc.width, c.osc.height
    rays = np.concatenate([c.rays, rays_ref.primary_rays(c.osc)])
    t_max = np.concatenate([c.t_max, np.full(w * h, Q.K_MAX_T)])
    rects, xy = (None, Q.RECTS_SMALL[(w, h)]), all_pixels(w, h)
    r, plain = pkg.Renderer(c.sc, device=0, flags=forced(pkg)), pkg.Renderer(c.sc, device=0)
    try:
        assert r.streamed_queries and not plain.streamed_queries
        assert_same_outputs(ray_outputs(r, rays, t_max), ray_outputs(plain, rays, t_max), "six cubics")
        px = pixel_outputs(r, rects, xy)
        assert_same_outputs(px, pixel_outputs(plain, rects, xy), "six cubics")
        assert_within_one_context(r, px, xy, "six cubics", plane0=False)
        cubic = Q.tables(c.coefs)["cubic"]
        assert np.isin(px["object"], cubic[:4]).any() and np.isin(px["object"], cubic[4:]).any()
    finally:
        r.cleanup_update()
        plain.cleanup_update()


# ---- 3. at the limit -------------------------------------------------------------------------------------------------------------------------------
def test_at_the_limit_the_flag_alone_streams(pkg):
    """2 560 spheres: the tables are exactly the 160 KiB the staged kernels can have, and the context is streamed by size, so the flag
    alone gives it the streamed queries.  They equal the composers and the unflagged context, which still runs the staged launch."""
    c = large(Q.LARGE[3])
    r, plain = pkg.Renderer(c.sc, device=0, flags=flag(pkg)), pkg.Renderer(c.sc, device=0)
    try:
        assert r.streamed and r.streamed_queries and plain.streamed and not plain.streamed_queries
        check_ray_queries(r, c, Composed(c.osc, c.rays, c.t_max), Q.LARGE[3])
        check_pixel_queries(r, c.osc, Q.ROWS, Q.RECTS_LARGE, Q.LARGE[3])
        assert_same_outputs(ray_outputs(r, c.rays, c.t_max), ray_outputs(plain, c.rays, c.t_max), Q.LARGE[3])
        rects, xy = (None,) + Q.RECTS_LARGE, all_pixels(64, 48)
        assert_same_outputs(pixel_outputs(r, rects, xy), pixel_outputs(plain, rects, xy), Q.LARGE[3])
    finally:
        r.cleanup_update()
        plain.cleanup_update()


# ---- 4. beyond the limit ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.BEYOND)
def test_beyond_the_limit(pkg, name):
    """2 562 spheres (two entries in the 41st chunk), 2 625 spheres with mirrors at depth 2, and 1 050 spheres, 1 050 general quadrics and
    two planes: no staged query kernel takes these.  With the flag alone the aimed rays, the planes on Q.ROWS, every pick there and the
    extents of Q.RECTS_LARGE equal the composers; a default and an RT_FLAG_SIMPLE context answer alike."""
    c = B.beyond(name)
    rects, xy = (None,) + Q.RECTS_LARGE, all_pixels(64, 48)
    r, simple = pkg.Renderer(c.sc, device=0, flags=flag(pkg)), pkg.Renderer(c.sc, device=0, flags=flag(pkg) | pkg.RT_FLAG_SIMPLE)
    try:
        assert r.streamed and r.streamed_queries and simple.streamed and simple.streamed_queries
        check_ray_queries(r, c, Composed(c.osc, c.rays, c.t_max), name)
        check_pixel_queries(r, c.osc, Q.ROWS, Q.RECTS_LARGE, name)
        px = pixel_outputs(r, rects, xy)
        assert_within_one_context(r, px, xy, name)
        assert_same_outputs(ray_outputs(simple, c.rays, c.t_max), ray_outputs(r, c.rays, c.t_max), (name, "RT_FLAG_SIMPLE"))
        assert_same_outputs(pixel_outputs(simple, rects, xy), px, (name, "RT_FLAG_SIMPLE"))
    finally:
        r.cleanup_update()
        simple.cleanup_update()


# ---- 5. partial waves and mixed lanes ----------------------------------------------------------------------------------------------------------------
def test_prefixes_of_the_rays_and_of_the_pixels(pkg):
    """1, 63, 64, 65 and 257 of the aimed rays of the 2 562-sphere field (NaN, inf, 1e120 and zero-direction rays among them, so plain
    and table lanes share waves): each entry point returns the same prefix of the full run's result; so do rt_pick and rt_pick_paths of
    1, 65 and all pixels."""
    c = B.beyond(B.BEYOND[0])
    assert not np.isfinite(c.rays["d"]).all() and (np.abs(c.rays["d"]).max(axis=1) == 0).any()
    r = pkg.Renderer(c.sc, device=0, flags=flag(pkg))
    try:
        assert r.streamed_queries
        full = ray_outputs(r, c.rays, c.t_max)
        for n in B.FIELD_PREFIXES:
            got = ray_outputs(r, c.rays[:n], c.t_max[:n])
            want = {k: (v[:, :n] if k == "rt_trace_paths, segments" else v[:n]) for k, v in full.items()}
            assert_same_outputs(got, want, n)
        xy = all_pixels(64, 48)
        rec, (seg, ends) = r.pick(xy), r.pick_paths(xy)
        for n in (1, 65):
            got, (gseg, gends) = r.pick(xy[:n]), r.pick_paths(xy[:n])
            assert got.tobytes() == rec[:n].tobytes() and gends.tobytes() == ends[:n].tobytes(), n
            assert np.ascontiguousarray(gseg).tobytes() == np.ascontiguousarray(seg[:, :n]).tobytes(), n
    finally:
        r.cleanup_update()


# ---- 6. extents without LDS accumulators -----------------------------------------------------------------------------------------------------------------
def test_extents_and_the_merge_of_three_ranks(pkg):
    """The streamed extents kernel has no accumulators in LDS: every wave merges into the output.  The whole frame and both rectangles
    are the reduction of the context's planes; as world = 3 with bands of 8 rows the three ranks' records, merged by
    rt_merge_object_extents, are the single context's (each rectangle lies in one band: two ranks own none of it)."""
    import torch
    c = B.beyond(B.BEYOND[0])
    rects = (None,) + Q.RECTS_LARGE
    one = pkg.Renderer(c.sc, device=0, flags=flag(pkg))
    n = n_objects(one)
    try:
        assert one.streamed_queries
        want = [one.object_extents(None, rect) for rect in rects]
        for rect, w in zip(rects, want):
            assert_extents(w, from_planes(one, None, rect), ("one context", rect))
        assert all(w["pixels"].sum() > 0 for w in want)
        ranks = [pkg.Renderer(c.sc, device=0, rank=k, world=3, band_rows=8, flags=flag(pkg)) for k in range(3)]
        try:
            for rect, w in zip(rects, want):
                parts = torch.zeros((3, n * 5), dtype=torch.int64, device="cuda:0")
                out = torch.zeros((n * 5,), dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                empty = 0
                for k, rk in enumerate(ranks):
                    assert rk.streamed_queries
                    rk.object_extents_into(None, rect, parts[k].data_ptr())
                    torch.cuda.synchronize()
                    mine = parts[k].cpu().numpy().view(extents_ref.DTYPE)
                    assert_extents(mine, from_planes(rk, None, rect), ("rank", k, rect))
                    empty += mine.tobytes() == extents_ref.identity(n).tobytes()
                owners = set(range(3)) if rect is None else {(y // 8) % 3 for y in range(rect[1], rect[3] + 1)}
                assert empty == 3 - len(owners) and (rect is None or empty == 2), (rect, empty)   # a rank without a row of the rectangle: the identities alone
                one.merge_object_extents(parts.data_ptr(), 3, out.data_ptr())
                torch.cuda.synchronize()
                assert_extents(out.cpu().numpy().view(extents_ref.DTYPE), w, ("merged", rect))
        finally:
            for rk in ranks:
                rk.cleanup_update()
    finally:
        one.cleanup_update()


# ---- 7. after a scene update ---------------------------------------------------------------------------------------------------------------------------------
def test_after_rt_set_scene_the_queries_are_the_moved_scenes(pkg):
    sc, coefs, c = B.moved_beyond(pkg)
    rects, xy = (None,) + Q.RECTS_LARGE, all_pixels(64, 48)
    r, fresh = pkg.Renderer(sc, device=0, flags=flag(pkg)), pkg.Renderer(c.sc, device=0, flags=flag(pkg))
    try:
        assert r.streamed_queries and fresh.streamed_queries
        before = trace_dev(r, c.rays)
        r.set_scene(coefs=coefs)
        assert r.streamed_queries
        got = ray_outputs(r, c.rays, c.t_max)
        assert not rays_ref.same_records(got["rt_trace_rays"], before)
        assert_same_outputs(got, ray_outputs(fresh, c.rays, c.t_max), "moved, rays")
        assert_same_outputs(pixel_outputs(r, rects, xy), pixel_outputs(fresh, rects, xy), "moved, pixels")
        check_ray_queries(r, c, Composed(c.osc, c.rays, c.t_max), "moved")
        check_pixel_queries(r, c.osc, Q.ROWS, Q.RECTS_LARGE, "moved")
    finally:
        r.cleanup_update()
        fresh.cleanup_update()


# ---- 8. one captured graph ---------------------------------------------------------------------------------------------------------------------------------------
def test_one_graph_of_an_update_and_four_queries(pkg):
    """rt_set_scene, rt_trace_rays, rt_shade_rays, rt_render_gbuffer and rt_object_extents, all with ms == NULL, as a linear chain on one
    stream: replayed twice, with the moved and then with the first coefficients, the graph gives what the uncaptured calls give."""
    import torch
    sc, moved, c = B.moved_beyond(pkg)
    first = sc.arrays()["coefs"].copy()
    r = pkg.Renderer(sc, device=0, flags=flag(pkg))
    s = torch.cuda.Stream()
    n, nr, w, h = n_objects(r), len(c.rays), r.width, r.height
    try:
        assert r.streamed_queries
        with torch.cuda.stream(s):
            d_coefs, d_rays = torch.from_numpy(moved.copy()).to("cuda:0"), to_device(c.rays)
            hits = torch.zeros((nr, 6), dtype=torch.float64, device="cuda:0")
            rgba = torch.zeros((nr, 4), dtype=torch.float32, device="cuda:0")
            po, pt = torch.zeros((h, w), dtype=torch.int32, device="cuda:0"), torch.zeros((h, w), dtype=torch.float64, device="cuda:0")
            pn = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
            ext = torch.zeros((n * 5,), dtype=torch.int64, device="cuda:0")
        outs = (hits, rgba, po, pt, pn, ext)
        torch.cuda.synchronize()

        def chain():
            r.set_scene_into(coefs=d_coefs.data_ptr(), stream=s.cuda_stream)
            r.trace_into(d_rays.data_ptr(), nr, hits.data_ptr(), stream=s.cuda_stream, timed=False)
            r.shade_into(d_rays.data_ptr(), nr, rgba.data_ptr(), stream=s.cuda_stream, timed=False)
            r.gbuffer_into(None, po.data_ptr(), pt.data_ptr(), pn.data_ptr(), stream=s.cuda_stream, timed=False)
            r.object_extents_into(None, None, ext.data_ptr(), stream=s.cuda_stream, timed=False)

        plain = []
        for coefs in (moved, first):   # the uncaptured calls, on the same stream
            with torch.cuda.stream(s):
                d_coefs.copy_(torch.from_numpy(coefs.copy()))
            chain()
            s.synchronize()
            plain.append([o.cpu().numpy().tobytes() for o in outs])
        assert all(a != b for a, b in zip(*plain))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            chain()
        for k, coefs in enumerate((moved, first)):
            with torch.cuda.stream(s):
                d_coefs.copy_(torch.from_numpy(coefs.copy()))
                for o in outs:
                    o.view(torch.uint8).fill_(0xAB)
                g.replay()
            s.synchronize()
            assert [o.cpu().numpy().tobytes() for o in outs] == plain[k], ("replay", k)
        del g
    finally:
        torch.cuda.synchronize()
        r.cleanup_update()


# ---- 9. the FAST build, forced ---------------------------------------------------------------------------------------------------------------------------------------
def test_fast_build_statistics_forced(pkg):
    """FAST against strict, both forced (device against device), on the 129-quadric and the 193-sphere field, to the bar of
    tests/test_query_tables_gpu.py::test_fast_build_statistics: `object` of rt_trace_rays and of the G-buffer agree on at least 99 %.
    Inside the FAST context the staged family's promises hold: a pick is the planes' entry, the extents are their reduction."""
    for case in (("quadric", 129), ("sphere", 193)):
        c = Q.small_case(pkg, case)
        rays = np.concatenate([c.rays, rays_ref.primary_rays(c.osc)])
        ra, rb = pkg.Renderer(c.sc, device=0, flags=forced(pkg)), pkg.Renderer(c.sc, device=0, flags=forced(pkg) | pkg.RT_FLAG_FAST)
        try:
            assert ra.streamed_queries and rb.streamed_queries
            a, b = trace_dev(ra, rays), trace_dev(rb, rays)
            pa = device_planes(ra)
            xy = all_pixels(64, 48)
            px = pixel_outputs(rb, (None, Q.RECTS_SMALL[(64, 48)]), xy)
            assert_within_one_context(rb, px, xy, (case, "FAST"))
        finally:
            ra.cleanup_update()
            rb.cleanup_update()
        both = (a["object"] >= 0) & (b["object"] >= 0)
        rel = np.abs(a["t"][both] - b["t"][both]) / np.abs(a["t"][both])
        agree, agree_planes = float((a["object"] == b["object"]).mean()), float((pa[0] == px["object"]).mean())
        print(f"FAST vs strict, forced, {case[1]} {case[0]} field: rt_trace_rays object differs at {int((a['object'] != b['object']).sum())} of {len(rays)} rays "
              f"({100 * agree:.3f} % agree), max rel t difference {float(rel.max()):.3e}; G-buffer object differs at {int((pa[0] != px['object']).sum())} of {pa[0].size} "
              f"pixels ({100 * agree_planes:.3f} % agree)")
        assert agree >= 0.99 and agree_planes >= 0.99, (case, agree, agree_planes)
        assert both.any() and a["object"].max() >= 128


# ---- 10. several contexts ----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_flag_reaches_every_context_of_rt_create_multi(pkg):
    c = B.beyond(B.BEYOND[0])
    one = pkg.Renderer(c.sc, device=0, flags=flag(pkg))
    try:
        want_planes, want_ext, want_hits = device_planes(one), one.object_extents(), trace_dev(one, c.rays)
    finally:
        one.cleanup_update()
    m = pkg.MultiRenderer(c.sc, [0, 0], band_rows=8, parts=2, flags=flag(pkg))
    try:
        assert m.query.streamed_queries
        o, t, n, _ = m.gbuffer()
        m.wait()
        got = (o.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy())
        for a, b in zip(got, want_planes):
            assert a.tobytes() == b.tobytes(), "rt_render_gbuffer_multi"
        assert_extents(m.object_extents(), want_ext, "rt_object_extents_multi_host")
        assert rays_ref.same_records(m.trace(c.rays["o"], c.rays["d"]), want_hits), "rt_trace_rays on rt_multi_query_ctx"
    finally:
        m.cleanup_update()


# ---- 11. the update.h adapter -------------------------------------------------------------------------------------------------------------------------------------------
ADAPTER = r"""
import ctypes as C, os, re, subprocess, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "tools"))
import __graft_entry__ as g
import gbuffer_ref, query_table_scenes as Q, rays_ref, stream_query_scenes as B
pkg = g.load_package()
c = B.beyond(B.BEYOND[0])
row = Q.ROWS[3]
ref = gbuffer_ref.compose(c.osc, rows=np.array([row]))
upd = C.CDLL(pkg.UPDATE_LIB_PATH)
names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
update = getattr(upd, re.search(r"\b(_Z\d+updateRKN3glm3matI\S*)\b", names).group(1))
cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
update.argtypes, update.restype = [C.c_void_p], C.c_float
upd.mi355rt_update_pick.argtypes = [C.c_uint, C.c_uint, C.c_void_p]
cam = np.ascontiguousarray(pkg.IDENTITY, dtype=np.float64)
init(7, c.sc._h)
update(cam.ctypes.data)
got = np.zeros(c.osc.width, dtype=rays_ref.HIT_DTYPE)
rcs = [upd.mi355rt_update_pick(x, row, C.c_void_p(got[x:].ctypes.data)) for x in range(c.osc.width)]
err = pkg.lib().rt_last_error().decode()
cleanup()
want = np.zeros(c.osc.width, dtype=rays_ref.HIT_DTYPE)
want["t"], want["object"], want["point"], want["normal"] = ref["t"][0], ref["object"][0], ref["point"][0], ref["normal"][0][:, :3]
print("pick", sorted(set(rcs)), bool(rays_ref.same_records(got, want)), int((want["object"] >= 0).sum()) > 0, err)
"""


def test_the_adapter_picks_on_the_large_field():
    """init_update() with MI355RT_STREAM_QUERIES=1 (a fresh process, for the environment): mi355rt_update_pick on a row of the 2 562-sphere
    field returns the composer's records; without the switch the hook refuses the scene as it always has."""
    def run(**env):
        return subprocess.run([sys.executable, "-c", ADAPTER, ROOT], capture_output=True, text=True, timeout=180, env=dict(os.environ, **env))
    out = run(MI355RT_STREAM_QUERIES="1")
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("pick [0] True True"), out.stdout
    out = run(MI355RT_STREAM_QUERIES="0")
    assert out.returncode == 0, out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("pick [-2] False True") and "scene needs" in last and "bytes of LDS per workgroup (limit 160 KiB)" in last, out.stdout


# ---- 12. the flag alone on a small scene ----------------------------------------------------------------------------------------------------------------------------------
def test_the_flag_alone_leaves_a_small_scene_to_the_staged_kernels(pkg):
    c = Q.small_case(pkg, ("sphere", 129))
    rects, xy = (None, Q.RECTS_SMALL[(64, 48)]), all_pixels(64, 48)
    r, plain = pkg.Renderer(c.sc, device=0, flags=flag(pkg)), pkg.Renderer(c.sc, device=0)
    try:
        assert not r.streamed and not r.streamed_queries and not plain.streamed_queries
        assert_same_outputs(ray_outputs(r, c.rays, c.t_max), ray_outputs(plain, c.rays, c.t_max), "the flag alone")
        assert_same_outputs(pixel_outputs(r, rects, xy), pixel_outputs(plain, rects, xy), "the flag alone")
        got = shade_of_primary(r)
        assert got.tobytes() == shade_of_primary(plain).tobytes()
    finally:
        r.cleanup_update()
        plain.cleanup_update()
