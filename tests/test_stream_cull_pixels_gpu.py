"""Culled pixel queries on the GPU (RT_FLAG_STREAM_CULL_PIXELS; csrc/rt_stream_cull_pixels.hip): rt_render_gbuffer,
rt_pick, rt_object_extents, the _host and multi-GPU forms with the unit-sphere chunks culled by the block's cone.  The outputs are the
streamed queries' by definition: every strict output of degree <= 2 here is compared bit for bit with the CPU composers (the checks of
tests/test_query_tables_gpu.py, imported), with the same context without the new flag ("unflagged") and, where a staged kernel takes the
scene, with the unflagged staged context; degree 3 and RT_FLAG_FAST against the unflagged context of the same build.  "Five flags" is
RT_FLAG_STREAM | RT_FLAG_STREAM_QUERIES | RT_FLAG_STREAM_CULL | RT_FLAG_STREAM_CULL_PIXELS.  The host-side condition (the statistics
scene's skipped pairs) is in tests/test_stream_cull_pixels_host.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import pixel_cull_lab as PL  # noqa: E402
import query_table_scenes as Q  # noqa: E402
import stream_cull_lab as SC  # noqa: E402
import stream_query_scenes as B  # noqa: E402
import stream_scenes as S  # noqa: E402
from test_extents_gpu import assert_same as assert_extents, n_objects  # noqa: E402
from test_query_tables_gpu import check_pixel_queries, device_planes  # noqa: E402
from test_stream_cull_bounce_gpu import cubic_mirror_and_field  # noqa: E402
from test_stream_cull_host import raw_scene_with_unbounded_spheres  # noqa: E402
from test_stream_queries_gpu import all_pixels, assert_same_outputs, assert_within_one_context, pixel_outputs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def the_feature(pkg):
    assert pkg.RT_FLAG_STREAM_CULL_PIXELS == 4194304


def five(pkg):
    return pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_QUERIES | pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_PIXELS


def by_size(pkg):
    """The flags of a scene that is streamed by its size, without RT_FLAG_STREAM."""
    return five(pkg) & ~pkg.RT_FLAG_STREAM


def renderer(pkg, sc, flags, expect=True, **kw):
    r = pkg.Renderer(sc, device=0, flags=flags, **kw)
    assert r.stream_cull_pixels is expect, (r.stream_cull_pixels, r.stream_cull, r.streamed_queries, r.streamed)
    return r


def pair(pkg, sc, flags, **kw):
    """The flagged context and the same context without the new flag."""
    r = renderer(pkg, sc, flags, **kw)
    twin = renderer(pkg, sc, flags & ~pkg.RT_FLAG_STREAM_CULL_PIXELS, False, **kw)
    assert twin.streamed_queries and twin.stream_cull
    return r, twin


def cleanup(*rs):
    for r in rs:
        if r is not None:
            r.cleanup_update()


def check_against_twin(pkg, sc, flags, rects, xy, what, within=True, plane0=True, cam=None, **kw):
    """Planes, picks of xy and the extents of rects: the flagged context's equal the unflagged context's, and its own promises hold."""
    r, twin = pair(pkg, sc, flags, **kw)
    try:
        if cam is None:
            px = pixel_outputs(r, rects, xy)
            assert_same_outputs(px, pixel_outputs(twin, rects, xy), (what, "without the flag"))
            if within:
                assert_within_one_context(r, px, xy, what, plane0=plane0)
        else:
            px = cam_outputs(r, cam, rects, xy)
            assert_same_outputs(px, cam_outputs(twin, cam, rects, xy), (what, "without the flag"))
        return px
    finally:
        cleanup(r, twin)


def cam_outputs(r, cam, rects, xy):
    o, t, n, _ = r.gbuffer(cam)
    out = {"object": o.cpu().numpy(), "t": t.cpu().numpy(), "normal": n.cpu().numpy(), "rt_pick": r.pick(xy, cam=cam)}
    for rect in rects:
        out[("rt_object_extents", rect)] = r.object_extents(cam, rect)
    return out


# ---- 1. chunk boundaries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 129, 193])
@pytest.mark.parametrize("size", Q.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_chunk_boundaries(pkg, n, size):
    """65 / 129 / 193 spheres: one entry behind one, two and three full chunks, on the 64 x 48 frame and on the 37 x 21 one, whose partial
    tiles and blocks form their cones from clamped corner lanes.  Planes, the pick of every pixel, the extents of the whole frame and of a
    rectangle: against the composers, the unflagged context and the unflagged staged context."""
    assert ("sphere", n) in Q.SMALL
    w, h = size
    cs = Q.small_case(pkg, ("sphere", n), w, h)
    rects, xy = (None, Q.RECTS_SMALL[(w, h)]), all_pixels(w, h)
    r, twin = pair(pkg, cs.sc, five(pkg))
    plain = pkg.Renderer(cs.sc, device=0)
    try:
        assert not plain.streamed_queries
        check_pixel_queries(r, cs.osc, None, rects, (n, w, h))
        px = pixel_outputs(r, rects, xy)
        assert_same_outputs(px, pixel_outputs(twin, rects, xy), (n, w, h, "without the flag"))
        assert_same_outputs(px, pixel_outputs(plain, rects, xy), (n, w, h, "staged"))
        assert_within_one_context(r, px, xy, (n, w, h))
        assert (px["object"] >= 64 * ((n - 1) // 64)).any()      # (the last chunk's one entry is seen)
    finally:
        cleanup(r, twin, plain)


# ---- 2. more than 64 chunks ---------------------------------------------------------------------------------------------------------------
def test_more_than_64_chunks(pkg):
    """4 100 spheres, 65 chunks: the second trip of the bound-group loop.  Against the unflagged context; a sphere of the 65th chunk owns
    a pixel of the frame."""
    sc = S.field(pkg, 4100, 3)
    px = check_against_twin(pkg, sc, five(pkg), (None,) + Q.RECTS_LARGE, all_pixels(64, 48), "4100 spheres")
    # ... and the second trip contributes: some pixel's owner is an entry of the 65th chunk of the device's own ordered table
    r = renderer(pkg, sc, five(pkg))
    try:
        words = SC.image(sc.arrays())[2]
        table = SC.table_of(r.debug_scene_blob(), words)
        assert words["n_chunks"] == 65 and len(table) == 4100 and len(r.stream_bounds()) == 65 * 64
        assert np.isin(px["object"], table["orig"][64 * 64:]).any()
    finally:
        r.cleanup_update()


# ---- 3. other table shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [False, True], ids=["strict", "fast"])
def test_large_mixed_scene(pkg, fast):
    """Spheres among ellipsoids and planes (the <HAS_GQ = 1, HAS_CUBIC = 0> instantiations), strict and RT_FLAG_FAST: against the
    unflagged context of the same build, with the promises inside one context; the strict build also against the composers on Q.ROWS /
    Q.RECTS_LARGE."""
    from test_query_tables_gpu import large
    c = large(Q.LARGE[2])
    extra = pkg.RT_FLAG_FAST if fast else 0
    r, twin = pair(pkg, c.sc, by_size(pkg) | pkg.RT_FLAG_STREAM | extra)
    try:
        if not fast:
            check_pixel_queries(r, c.osc, Q.ROWS, Q.RECTS_LARGE, Q.LARGE[2])
        rects, xy = (None,) + Q.RECTS_LARGE, all_pixels(64, 48)
        px = pixel_outputs(r, rects, xy)
        assert_same_outputs(px, pixel_outputs(twin, rects, xy), (Q.LARGE[2], fast))
        assert_within_one_context(r, px, xy, (Q.LARGE[2], fast), plane0=not fast)      # (rt_pick_paths is another kernel: its plane 0 is held to rt_pick in the strict build)
        quadric = Q.tables(c.sc.arrays()["coefs"])["quadric"]
        assert np.isin(px["object"], quadric).any() and (px["object"] >= 0).any()      # (a general quadric is seen)
    finally:
        cleanup(r, twin)


@pytest.mark.parametrize("fast", [False, True], ids=["strict", "fast"])
@pytest.mark.parametrize("name", B.BEYOND)
def test_beyond_the_staged_limit(pkg, name, fast):
    """2 562 spheres, 2 625 spheres with mirrors, and 1 050 spheres among 1 050 general quadrics and two planes: streamed by size, without
    RT_FLAG_STREAM; strict and RT_FLAG_FAST.  Against the unflagged context of the same build, with the promises inside one context; the
    strict build also against the composers."""
    c = B.beyond(name)
    rects, xy = (None,) + Q.RECTS_LARGE, all_pixels(64, 48)
    r, twin = pair(pkg, c.sc, by_size(pkg) | (pkg.RT_FLAG_FAST if fast else 0))
    try:
        if not fast:
            check_pixel_queries(r, c.osc, Q.ROWS, Q.RECTS_LARGE, name)
        px = pixel_outputs(r, rects, xy)
        assert_same_outputs(px, pixel_outputs(twin, rects, xy), (name, fast))
        assert_within_one_context(r, px, xy, (name, fast), plane0=not fast)      # (as above)
        assert (px["object"] >= 0).any()
    finally:
        cleanup(r, twin)


@pytest.mark.parametrize("fast", [False, True], ids=["strict", "fast"])
def test_six_cubic_objects_over_a_field(pkg, fast):
    """Six degree-3 objects -- the host's records at the frame's origin for the first four, the per-lane form for the other two -- with the
    65-sphere field appended so that the decision is true: the flagged context against the unflagged one of the same build."""
    c = Q.cubic_case(pkg)
    a, fa = c.sc.arrays(), S.field(pkg, 65, S.FIELD_SEED).arrays()
    cat = {k: np.concatenate([a[k], fa[k]]) for k in ("coefs", "reflection", "albedo")}
    d = pkg.desc_from_arrays(a["width"], a["height"], a["vertical_fov"], a["bg_color"], a["max_reflections"], cat["coefs"], cat["reflection"], cat["albedo"],
                             a["light_is_spherical"], a["light_p"], a["light_color"])
    extra = pkg.RT_FLAG_FAST if fast else 0
    w, h = a["width"], a["height"]
    px = check_against_twin(pkg, d, five(pkg) | extra, (None, Q.RECTS_SMALL[(w, h)]), all_pixels(w, h), ("six cubics", fast), plane0=False)
    cubic = Q.tables(c.coefs)["cubic"]
    assert np.isin(px["object"], cubic[:4]).any() and np.isin(px["object"], cubic[4:]).any()


@pytest.mark.parametrize("with_quadric", [False, True], ids=["cubic", "cubic+quadric"])
@pytest.mark.parametrize("name", ["clebsch", "cayley"])
def test_a_cubic_surface_over_the_field(pkg, name, with_quadric):
    """The HAS_CUBIC instantiations, <0, 1> and <1, 1>, strict and fast: a degree-3 surface over the 65-sphere field.  Degree 3 is held to
    the library's own outputs: the flagged context's equal the unflagged context's of the same build."""
    d = cubic_mirror_and_field(pkg, name, 48, 36, with_quadric)
    for fast in (0, pkg.RT_FLAG_FAST):
        px = check_against_twin(pkg, d, five(pkg) | fast, (None, (5, 4, 40, 30)), all_pixels(48, 36), (name, with_quadric, fast), plane0=False)
        assert (px["object"] == 0).sum() > 50 and (px["object"] > 0).any()      # the surface (object 0) and the field are seen


# ---- 4. within one context, both builds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [False, True], ids=["strict", "fast"])
def test_within_one_context(pkg, fast):
    """rt_pick is the planes' entry and the extents are the planes' reduction, in the contracted build too; and each build's outputs are
    its unflagged context's."""
    extra = pkg.RT_FLAG_FAST if fast else 0
    for case, (w, h) in ((("sphere", 193), (64, 48)), (("sphere", 129), (37, 21))):
        cs = Q.small_case(pkg, case, w, h)
        check_against_twin(pkg, cs.sc, five(pkg) | extra, (None, Q.RECTS_SMALL[(w, h)]), all_pixels(w, h), (case, w, h, fast))


# ---- 5. ranks, cameras, odd spheres, pick counts --------------------------------------------------------------------------------------------
def test_rank_1_of_3_with_bands_of_8(pkg):
    sc = S.field(pkg, 193, S.FIELD_SEED, w=64, h=50)
    r, twin = pair(pkg, sc, five(pkg), rank=1, world=3, band_rows=8)
    try:
        rows = r.row_map()
        assert 0 < len(rows) < 50
        rects = (None, (3, 8, 60, 15), (0, 0, 63, 7))      # the second lies in this rank's first band, the third in rank 0's
        xy = np.stack([np.tile(np.arange(64), len(rows)), np.repeat(rows, 64)], axis=1)
        got, want = {}, {}
        for ctx, out in ((r, got), (twin, want)):
            out["object"], out["t"], out["normal"] = device_planes(ctx)
            out["rt_pick"] = ctx.pick(xy)
            for rect in rects:
                out[("rt_object_extents", rect)] = ctx.object_extents(None, rect)
        assert_same_outputs(got, want, "rank 1 of 3")
        assert got["object"].shape == (len(rows), 64) and (got["object"] >= 0).any()
        assert np.array_equal(got["rt_pick"]["object"], got["object"].reshape(-1))
        assert got[("rt_object_extents", rects[1])]["pixels"].sum() > 0 and got[("rt_object_extents", rects[2])]["pixels"].sum() == 0
    finally:
        cleanup(r, twin)


def test_rotated_and_moved_camera(pkg):
    sc = S.field(pkg, 193, S.FIELD_SEED)
    for cam in (pkg.camera_matrix((0.5, 0.3, -1.0), 88.0, 2.0), pkg.camera_matrix((6.0, 2.0, 4.0), 120.0, -9.0)):
        px = check_against_twin(pkg, sc, five(pkg), (None, Q.RECTS_SMALL[(64, 48)]), all_pixels(64, 48), "camera", cam=cam)
        assert (px["object"] >= 0).any()
        assert np.array_equal(px["rt_pick"]["object"], px["object"].reshape(-1))


def test_spheres_without_a_radius(pkg):
    """A chunk with a member without a radius has the bound +inf: it is always staged."""
    a = raw_scene_with_unbounded_spheres()
    d = pkg.desc_from_arrays(64, 48, np.radians(S.FOV), (0.05, 0.1, 0.2), 0, a["coefs"], a["reflection"], a["albedo"], a["light_is_spherical"], a["light_p"], a["light_color"])
    r, twin = pair(pkg, d, five(pkg))
    plain = pkg.Renderer(d, device=0)
    try:
        b = r.stream_bounds().view(SC.US_DTYPE)
        assert len(b) == 3 and np.isposinf(b["r"][2])
        rects, xy = (None, Q.RECTS_SMALL[(64, 48)]), all_pixels(64, 48)
        px = pixel_outputs(r, rects, xy)
        assert_same_outputs(px, pixel_outputs(twin, rects, xy), "unbounded tail")
        assert_same_outputs(px, pixel_outputs(plain, rects, xy), "unbounded tail, staged")
        assert (px["object"] >= 0).any()
    finally:
        cleanup(r, twin, plain)


def test_prefixes_of_the_pixels(pkg):
    """1, 63, 64, 65 and 257 picked pixels (partial waves, a wave without a pixel, a second workgroup): the same prefix of the full pick."""
    cs = Q.small_case(pkg, ("sphere", 193))
    r, twin = pair(pkg, cs.sc, five(pkg))
    try:
        xy = all_pixels(64, 48)[::5]      # (unrelated pixels)
        full = r.pick(xy)
        assert full.tobytes() == twin.pick(xy).tobytes() and (full["object"] >= 0).any()
        for n in (1, 63, 64, 65, 257):
            assert r.pick(xy[:n]).tobytes() == full[:n].tobytes(), n
    finally:
        cleanup(r, twin)


# ---- 6. scene updates -------------------------------------------------------------------------------------------------------------------------
def test_after_rt_set_scene_the_queries_are_the_moved_scenes(pkg):
    sc, coefs, c = B.moved_beyond(pkg)
    rects, xy = (None,) + Q.RECTS_LARGE, all_pixels(64, 48)
    r, fresh = renderer(pkg, sc, by_size(pkg)), renderer(pkg, c.sc, by_size(pkg) & ~pkg.RT_FLAG_STREAM_CULL_PIXELS, False)
    try:
        before = device_planes(r)[0]
        r.set_scene(coefs=coefs)
        assert r.stream_cull_pixels and r.set_scene_status()["applied"] == 1
        px = pixel_outputs(r, rects, xy)
        assert not np.array_equal(px["object"], before)
        assert_same_outputs(px, pixel_outputs(fresh, rects, xy), "moved")
        check_pixel_queries(r, c.osc, Q.ROWS, Q.RECTS_LARGE, "moved")
    finally:
        cleanup(r, fresh)


def test_one_graph_of_an_update_and_the_pixel_queries(pkg):
    """rt_set_scene, rt_render_gbuffer and rt_object_extents, all with ms == NULL, as a linear chain on one stream: replayed twice, with
    the moved and then with the first coefficients, the graph gives what the uncaptured calls give, and both are what an unflagged
    context gives after the same two updates -- the planes, the extents, and the pick of every pixel behind each replay (rt_pick copies
    from host memory and waits, so it cannot be part of a graph: it is called behind the replay).  For the moved scene that is also what
    a fresh unflagged context of it gives."""
    import torch
    sc, moved, c = B.moved_beyond(pkg)
    first = sc.arrays()["coefs"].copy()
    r = renderer(pkg, sc, by_size(pkg))
    s = torch.cuda.Stream()
    n, w, h = n_objects(r), r.width, r.height
    xy = all_pixels(w, h)
    # the unflagged context after the same updates, in the same order: moved, first, (the replays:) moved, first
    twin = renderer(pkg, sc, by_size(pkg) & ~pkg.RT_FLAG_STREAM_CULL_PIXELS, False)
    try:
        unflagged = []
        for coefs in (moved, first, moved, first):
            twin.set_scene(coefs=coefs)
            o, t, nrm = device_planes(twin)
            unflagged.append(([o.tobytes(), t.tobytes(), nrm.tobytes(), twin.object_extents().tobytes()], twin.pick(xy).tobytes()))
        assert twin.set_scene_status()["applied"] == 4 and unflagged[0] == unflagged[2] and unflagged[1] == unflagged[3] and unflagged[0] != unflagged[1]
    finally:
        twin.cleanup_update()
    try:
        with torch.cuda.stream(s):
            d_coefs = torch.from_numpy(moved.copy()).to("cuda:0")
            po, pt = torch.zeros((h, w), dtype=torch.int32, device="cuda:0"), torch.zeros((h, w), dtype=torch.float64, device="cuda:0")
            pn = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
            ext = torch.zeros((n * 5,), dtype=torch.int64, device="cuda:0")
        outs = (po, pt, pn, ext)
        torch.cuda.synchronize()

        def chain():
            r.set_scene_into(coefs=d_coefs.data_ptr(), stream=s.cuda_stream)
            r.gbuffer_into(None, po.data_ptr(), pt.data_ptr(), pn.data_ptr(), stream=s.cuda_stream, timed=False)
            r.object_extents_into(None, None, ext.data_ptr(), stream=s.cuda_stream, timed=False)

        plain, picks = [], []
        for coefs in (moved, first):   # the uncaptured calls, on the same stream
            with torch.cuda.stream(s):
                d_coefs.copy_(torch.from_numpy(coefs.copy()))
            chain()
            s.synchronize()
            plain.append([o.cpu().numpy().tobytes() for o in outs])
            picks.append(r.pick(xy).tobytes())
        assert all(a != b for a, b in zip(*plain))
        for k in range(2):
            assert (plain[k], picks[k]) == unflagged[k], ("uncaptured against the unflagged context", k)
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
            assert r.pick(xy).tobytes() == picks[k], ("pick behind replay", k)
            assert (plain[k], picks[k]) == unflagged[2 + k], ("replay against the unflagged context after the same update", k)
        del g
    finally:
        torch.cuda.synchronize()
        r.cleanup_update()
    fresh = renderer(pkg, c.sc, by_size(pkg) & ~pkg.RT_FLAG_STREAM_CULL_PIXELS, False)
    try:
        o, t, nrm = device_planes(fresh)
        assert plain[0][0] == o.tobytes() and plain[0][1] == t.tobytes() and plain[0][2] == nrm.tobytes()
        assert plain[0][3] == fresh.object_extents().tobytes() and picks[0] == fresh.pick(xy).tobytes()
    finally:
        fresh.cleanup_update()


# ---- 7. other front ends ------------------------------------------------------------------------------------------------------------------------
def test_host_forms(pkg):
    """rt_object_extents_host (Renderer.object_extents) and rt_object_extents into device memory go through the two launch sites: equal
    to each other and to the unflagged context's."""
    import torch
    cs = Q.small_case(pkg, ("sphere", 193))
    r, twin = pair(pkg, cs.sc, five(pkg))
    try:
        n = n_objects(r)
        for rect in (None, Q.RECTS_SMALL[(64, 48)]):
            host = r.object_extents(None, rect)
            dev = torch.zeros((n * 5,), dtype=torch.int64, device="cuda:0")
            ms = r.object_extents_into(None, rect, dev.data_ptr())
            torch.cuda.synchronize()
            assert ms is not None and ms >= 0.0
            assert dev.cpu().numpy().tobytes() == host.tobytes() == twin.object_extents(None, rect).tobytes(), rect
            assert host["pixels"].sum() > 0
    finally:
        cleanup(r, twin)


def test_multi_renderer(pkg):
    cs = Q.small_case(pkg, ("sphere", 193))
    xy = all_pixels(64, 48)
    one = renderer(pkg, cs.sc, five(pkg) & ~pkg.RT_FLAG_STREAM_CULL_PIXELS, False)
    try:
        want_planes, want_ext, want_pick = device_planes(one), one.object_extents(), one.pick(xy)
    finally:
        one.cleanup_update()
    m = pkg.MultiRenderer(cs.sc, [0, 0], band_rows=8, parts=2, flags=five(pkg))
    try:
        assert m.stream_cull_pixels is True and m.query.streamed_queries
        o, t, n, _ = m.gbuffer()
        m.wait()
        for a, b in zip((o.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy()), want_planes):
            assert a.tobytes() == b.tobytes(), "rt_render_gbuffer_multi"
        assert_extents(m.object_extents(), want_ext, "rt_object_extents_multi_host")
        assert m.pick(xy).tobytes() == want_pick.tobytes(), "rt_pick on rt_multi_query_ctx"
    finally:
        m.cleanup_update()
    m = pkg.MultiRenderer(cs.sc, [0, 0], band_rows=8, parts=2, flags=five(pkg) & ~pkg.RT_FLAG_STREAM_CULL)
    try:
        assert m.stream_cull_pixels is False
    finally:
        m.cleanup_update()


ADAPTER = r"""
import ctypes as C, os, re, subprocess, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "tools"))
import __graft_entry__ as g
import extents_ref, gbuffer_ref, query_table_scenes as Q, rays_ref
pkg = g.load_package()
c = Q.small_case(pkg, ("sphere", 193))
row = 20
ref = gbuffer_ref.compose(c.osc, rows=np.array([row]))
whole = gbuffer_ref.compose(c.osc)
upd = C.CDLL(pkg.UPDATE_LIB_PATH)
names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
update = getattr(upd, re.search(r"\b(_Z\d+updateRKN3glm3matI\S*)\b", names).group(1))
cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
update.argtypes, update.restype = [C.c_void_p], C.c_float
upd.mi355rt_update_context.restype = C.c_void_p
upd.mi355rt_update_pick.argtypes = [C.c_uint, C.c_uint, C.c_void_p]
upd.mi355rt_update_extents.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
cam = np.ascontiguousarray(pkg.IDENTITY, dtype=np.float64)
init(7, c.sc._h)
update(cam.ctypes.data)
on = C.c_uint32(9)
rc_on = pkg.lib().rt_get_stream_cull_pixels(C.c_void_p(upd.mi355rt_update_context()), C.byref(on))
got = np.zeros(c.osc.width, dtype=rays_ref.HIT_DTYPE)
rcs = [upd.mi355rt_update_pick(x, row, C.c_void_p(got[x:].ctypes.data)) for x in range(c.osc.width)]
n = len(c.osc.objects)
ext = np.zeros(n, dtype=extents_ref.DTYPE)
rc_ext = upd.mi355rt_update_extents(None, C.c_void_p(ext.ctypes.data), n)
cleanup()
want = np.zeros(c.osc.width, dtype=rays_ref.HIT_DTYPE)
want["t"], want["object"], want["point"], want["normal"] = ref["t"][0], ref["object"][0], ref["point"][0], ref["normal"][0][:, :3]
want_ext = extents_ref.reduce_planes(whole["object"], whole["t"], n, np.arange(c.osc.width), np.arange(c.osc.height), None)
print("pixels", rc_on, on.value, sorted(set(rcs)), bool(rays_ref.same_records(got, want)), int((want["object"] >= 0).sum()) > 0, rc_ext, ext.tobytes() == want_ext.tobytes())
"""


def test_init_update_with_the_environment_switch():
    """The reference's back-end contract in a fresh process, on the 193-sphere field: with all four switches the adapter's context culls
    its pixel hooks' chunks, and mi355rt_update_pick / mi355rt_update_extents return the composers' records; without MI355RT_STREAM_CULL the
    switch is simply nothing."""
    def run(**env):
        return subprocess.run([sys.executable, "-c", ADAPTER, ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))
    out = run(MI355RT_STREAM="1", MI355RT_STREAM_QUERIES="1", MI355RT_STREAM_CULL="1", MI355RT_STREAM_CULL_PIXELS="1")
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "pixels 0 1 [0] True True 0 True", out.stdout
    out = run(MI355RT_STREAM="1", MI355RT_STREAM_QUERIES="1", MI355RT_STREAM_CULL_PIXELS="1")
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "pixels 0 0 [0] True True 0 True", out.stdout
    out = run(MI355RT_STREAM_CULL_PIXELS="yes")
    assert out.returncode != 0 and "mi355rt: MI355RT_STREAM_CULL_PIXELS: expected 0 or 1" in out.stderr, (out.stdout, out.stderr)


# ---- 8. the adaptive G pass ---------------------------------------------------------------------------------------------------------------------
def test_adaptive_frame_with_the_geometric_term(pkg):
    """The G pass of an RT_FLAG_SSAA_GEOMETRY frame keeps the streamed kernels: the frame and its refined count are those of the context
    without the new flag.  (Supersampling contexts refuse the G-buffer family as before, so the decision is not observable there but
    through the getter.)"""
    sc = S.field(pkg, 193, S.FIELD_SEED, mirrors=True, depth=1)
    f = pkg
    base = five(pkg) | f.RT_FLAG_SSAA2 | f.RT_FLAG_SSAA_ADAPTIVE | f.RT_FLAG_SSAA_GEOMETRY | f.RT_FLAG_STREAM_ADAPTIVE
    got = []
    for flags in (base, base & ~f.RT_FLAG_STREAM_CULL_PIXELS):
        r = pkg.Renderer(sc, device=0, flags=flags)
        try:
            assert r.streamed_adaptive and r.stream_cull and r.stream_cull_pixels == bool(flags & f.RT_FLAG_STREAM_CULL_PIXELS)
            r.update()
            got.append((r.download().copy(), r.refined))
            with pytest.raises(pkg.RtError):
                r.gbuffer()
        finally:
            r.cleanup_update()
    assert got[0][1] == got[1][1] > 0 and got[0][0].tobytes() == got[1][0].tobytes()


# ---- 9. the decision ------------------------------------------------------------------------------------------------------------------------------
def decision_cases(pkg):
    f = pkg
    c193, c64 = Q.small_case(pkg, ("sphere", 193)), Q.small_case(pkg, ("sphere", 64))
    return [("without RT_FLAG_STREAM_CULL", c193, five(pkg) & ~f.RT_FLAG_STREAM_CULL),
            ("without RT_FLAG_STREAM_QUERIES", c193, five(pkg) & ~f.RT_FLAG_STREAM_QUERIES),
            ("with RT_FLAG_NOCULL", c193, five(pkg) | f.RT_FLAG_NOCULL),
            ("one chunk", c64, five(pkg)),
            ("a small scene with RT_FLAG_STREAM_QUERIES alone", c193, f.RT_FLAG_STREAM_QUERIES | f.RT_FLAG_STREAM_CULL_PIXELS)]


@pytest.mark.parametrize("case", range(5))
def test_decision_false_is_the_context_without_the_flag(pkg, monkeypatch, case):
    """The getter says 0, rt_debug_stream_cull_pixels is refused, the blob and the bounds are the unflagged context's and so is every output."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    what, c, flags = decision_cases(pkg)[case]
    r, p = renderer(pkg, c.sc, flags, False), renderer(pkg, c.sc, flags & ~pkg.RT_FLAG_STREAM_CULL_PIXELS, False)
    try:
        assert r.stream_cull == p.stream_cull and r.streamed == p.streamed and r.streamed_queries == p.streamed_queries, what
        with pytest.raises(pkg.RtError) as e:
            r.stream_cull_pixels_stats()
        assert e.value.code == -1 and "rt_debug_stream_cull_pixels" in e.value.message and "MI355RT_STREAM_CULL_STATS" in e.value.message
        assert r.debug_scene_blob().tobytes() == p.debug_scene_blob().tobytes(), what
        if r.stream_cull:
            assert np.ascontiguousarray(r.stream_bounds()).tobytes() == np.ascontiguousarray(p.stream_bounds()).tobytes(), what
        rects, xy = (None, Q.RECTS_SMALL[(64, 48)]), all_pixels(64, 48)
        assert_same_outputs(pixel_outputs(r, rects, xy), pixel_outputs(p, rects, xy), what)
    finally:
        cleanup(r, p)


def test_decision_true_otherwise(pkg):
    c = Q.small_case(pkg, ("sphere", 65))
    for flags in (five(pkg), five(pkg) | pkg.RT_FLAG_FAST, five(pkg) | pkg.RT_FLAG_NOLEAN, five(pkg) | pkg.RT_FLAG_STREAM_CULL_RAYS | pkg.RT_FLAG_STREAM_CULL_BOUNCE):
        renderer(pkg, c.sc, flags).cleanup_update()


def test_without_the_environment_switch_there_are_no_work_words(pkg, monkeypatch):
    monkeypatch.delenv("MI355RT_STREAM_CULL_STATS", raising=False)
    c = Q.small_case(pkg, ("sphere", 129))
    r = renderer(pkg, c.sc, five(pkg))
    try:
        device_planes(r)
        with pytest.raises(pkg.RtError) as e:
            r.stream_cull_pixels_stats()
        assert e.value.code == -1 and "MI355RT_STREAM_CULL_STATS" in e.value.message
    finally:
        r.cleanup_update()


# ---- 10. statistics ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expectation():
    import __graft_entry__ as graft
    pkg = graft.load_package()
    return PL.expectation(pkg, SC.cluster_scene(pkg))


def test_statistics(pkg, monkeypatch):
    """stream_cull_lab's 320 clustered spheres (5 chunks), 64 x 48, 48 blocks.  After one rt_render_gbuffer: [0] == 48 x n_chunks exactly;
    [0] - [1] >= the host's skipped count (211 of 240); [1] is word [1] of rt_debug_stream_cull after one rt_render of the same scene and
    camera on an RT_FLAG_STREAM | RT_FLAG_STREAM_CULL context -- the same predicate, blocks and bounds, device against device --;
    [3] <= [2] <= 64 x [1]; the words double with a second call; the extents of the whole frame add the same [0] and [1]; a pick of 64
    pixels is one wave whose cone culls nothing: [1] == [0] == n_chunks."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    e = expectation()
    assert e["skipped"] >= 48 * e["n_chunks"] / 4
    sc = SC.cluster_scene(pkg)
    r, twin = pair(pkg, sc, five(pkg))
    frame = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL)
    try:
        assert r.stream_cull_pixels_stats() == [0] * 8
        planes = device_planes(r)
        w = r.stream_cull_pixels_stats()
        print("work words of rt_render_gbuffer", w, "expected", e)
        assert w[0] == 48 * e["n_chunks"], w
        assert w[0] - w[1] >= e["skipped"], w
        assert frame.stream_cull
        frame.update()
        fw = frame.stream_cull_stats()
        assert fw[0] == w[0] and w[1] == fw[1], (w, fw)
        assert 0 < w[3] <= w[2] <= 64 * w[1] and w[4:] == [0, 0, 0, 0], w
        assert all(a.tobytes() == b.tobytes() for a, b in zip(planes, device_planes(twin))) and (planes[0] >= 0).any()
        device_planes(r)
        assert r.stream_cull_pixels_stats() == [2 * x for x in w]      # cumulative
        ext = r.object_extents()
        w2 = r.stream_cull_pixels_stats()
        assert [w2[i] - 2 * w[i] for i in range(8)] == w, (w, w2)      # (one nearest call per block, the same blocks)
        assert ext.tobytes() == twin.object_extents().tobytes()
        xy = all_pixels(64, 48)[::48][:64]
        rec = r.pick(xy)
        w3 = r.stream_cull_pixels_stats()
        print("work words of a pick of 64 pixels", [a - b for a, b in zip(w3, w2)])
        assert w3[0] - w2[0] == e["n_chunks"] == w3[1] - w2[1] and w3[2] - w2[2] == 320 == w3[3] - w2[3], (w2, w3)
        assert rec.tobytes() == twin.pick(xy).tobytes()
    finally:
        cleanup(r, twin, frame)
