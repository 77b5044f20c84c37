"""Grouped chunk bounds on the GPU (RT_FLAG_STREAM_CULL_GROUPS; csrc/rt_stream_cull_groups.hip).  The frame is the
frame of the same context without the flag by definition: every frame here is compared bit for bit with the RT_FLAG_STREAM |
RT_FLAG_STREAM_CULL context (both formats), and every strict frame of degree <= 2 with the CPU oracle.  The host-side conditions (the
group bounds in 50 digits, the predicates about group bounds, the statistics scene's quarter of skips) are in
tests/test_stream_cull_groups_host.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import group_cull_lab as G  # noqa: E402
import raw_desc_scenes as R  # noqa: E402
import ssaa_ref  # noqa: E402
import stream_cull_lab as SC  # noqa: E402
import stream_scenes as S  # noqa: E402
from test_raw_descriptor_gpu import rgba8_of  # noqa: E402
from test_stream_cull_groups_host import unbounded_tail_arrays  # noqa: E402
from test_stream_gpu import MOVED  # noqa: E402

pytestmark = pytest.mark.gpu

F32, U8 = 0, 1


@pytest.fixture(autouse=True)
def the_feature(pkg):
    assert pkg.RT_FLAG_STREAM_CULL_GROUPS == 16777216 and hasattr(pkg.Renderer, "stream_groups")


def four(pkg):
    return pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_GROUPS


def gframe(pkg, sc, cam=None, expect=True, **kw):
    """One frame of a context, whose group decision must be `expect` (and whose group table is there exactly then)."""
    r = pkg.Renderer(sc, device=0, **kw)
    try:
        assert r.stream_groups == expect, (r.stream_groups, r.stream_cull, r.streamed)
        assert (r.debug_stream_group_bounds().size > 0) == expect
        r.update(cam)
        return r.download()
    finally:
        r.cleanup_update()


def check(pkg, sc, want, what, cam=None, flags=None, expect=True, **kw):
    """Flagged == the same context without RT_FLAG_STREAM_CULL_GROUPS, both formats; and, where `want` is given, == the oracle (RGBA8: its
    quantisation)."""
    flags = four(pkg) if flags is None else flags
    groups = pkg.RT_FLAG_STREAM_CULL_GROUPS
    assert flags & groups
    got = gframe(pkg, sc, cam, expect, flags=flags, **kw)
    assert R.same(got, gframe(pkg, sc, cam, False, flags=flags & ~groups, **kw)), what
    got8 = gframe(pkg, sc, cam, expect, flags=flags, fmt=pkg.RT_FMT_RGBA8, **kw)
    assert R.same(got8, gframe(pkg, sc, cam, False, flags=flags & ~groups, fmt=pkg.RT_FMT_RGBA8, **kw)), what
    if want is not None:
        assert np.all(got[..., 3] == 1.0) and R.same_as_oracle(got[..., :3], want), (what, R.n_diff(got[..., :3], want))
        q, ok = rgba8_of(want)
        assert got8.dtype == np.uint8 and not ((got8 != q)[..., :3] & ok).any() and np.all(got8[..., 3] == 255), what
    return got


# ---- frames against the unflagged context and the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4097, 8193])
def test_field(pkg, n):
    """4 097 spheres: two groups, the second one chunk of one entry; 8 193: three groups."""
    sc = S.field(pkg, n, S.FIELD_SEED)
    check(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), n)
    r = pkg.Renderer(sc, device=0, flags=four(pkg))
    try:
        g = r.debug_stream_group_bounds()
        assert g.size == 64 * ((n + 4095) // 4096) and R.same(g, G.group_image(r.stream_bounds()))
    finally:
        r.cleanup_update()


def test_one_group_is_the_context_without_the_flag(pkg, monkeypatch):
    """4 096 spheres: one group, decision false -- no group table, no group words, the unflagged context's words and frame."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    sc = S.field(pkg, 4096, S.FIELD_SEED)
    r, p = pkg.Renderer(sc, device=0, flags=four(pkg)), pkg.Renderer(sc, device=0, flags=four(pkg) & ~pkg.RT_FLAG_STREAM_CULL_GROUPS)
    try:
        assert r.stream_cull and r.stream_groups is False and r.debug_stream_group_bounds().size == 0
        with pytest.raises(pkg.RtError) as e:
            r.debug_stream_groups()
        assert e.value.code == -1 and "rt_debug_stream_groups: the context keeps no work words" in e.value.message
        assert R.same(r.debug_scene_blob(), p.debug_scene_blob()) and R.same(r.stream_bounds(), p.stream_bounds())
        for _ in range(2):
            r.update()
            p.update()
        assert R.same(r.download(), p.download()) and r.stream_cull_stats() == p.stream_cull_stats()
        assert R.same_as_oracle(r.download()[..., :3], S.oracle_of(pkg, sc).render(nthreads=8))
    finally:
        r.cleanup_update()
        p.cleanup_update()
    assert gframe(pkg, sc, None, False, flags=pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL_GROUPS) is not None      # (the flag without RT_FLAG_STREAM_CULL: simply false)


# ---- two clusters -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [(4096, 4096), (4000, 4193)], ids=["a group each", "a group straddles both"])
def test_two_clusters(pkg, counts):
    sc = G.two_clusters(pkg, counts)
    got = check(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), counts)
    assert (got[..., :3] != np.array([0.05, 0.1, 0.2], np.float32)).any()      # (the camera sees a cluster)
    a = sc.arrays()
    blob, bounds, w = SC.image(a)
    owner = SC.table_of(blob, w)["orig"] >= counts[0]
    assert not owner[:counts[0]].any() and owner[counts[0]:].all()      # the sort puts the first cluster in front: group 0 is 4 096 entries of ...
    g = G.group_image(bounds).view(SC.US_DTYPE)
    assert len(g) == (sum(counts) + 4095) // 4096 and np.isfinite(g["r"]).all()      # (4 000 + 4 193: a third group of one entry)
    if counts[0] == 4096:
        assert g["r"][0] < 8.0 and g["r"][1] < 8.0      # ... one cluster each (a cluster lies within 2.42 of its centre; a bound of bounds around box middles: < 3 x that)
    else:
        assert g["r"][0] > 20.0 and g["r"][1] < 8.0     # ... or of both: its bound spans the gap of 49


# ---- bounce rays ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounce", [False, True], ids=["full sweep", "culled per ray"])
def test_bounce_rays(pkg, bounce):
    """mixed_large with mirrors at depth 2: 4 100 unit spheres (two groups) among ellipsoids and planes.  With RT_FLAG_STREAM_CULL_BOUNCE the
    bounce rays ask the group bounds per ray; without it they keep sq_query."""
    sc = S.mixed_large(pkg, 8200, S.MIXED_SEED, depth=2)
    flags = four(pkg) | (pkg.RT_FLAG_STREAM_CULL_BOUNCE if bounce else 0)
    check(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), ("mixed", bounce), flags=flags)
    r = pkg.Renderer(sc, device=0, flags=flags)
    try:
        assert r.stream_groups and r.stream_cull_bounce == bounce
    finally:
        r.cleanup_update()


# ---- other modes --------------------------------------------------------------------------------------------------------------------------------
def test_spheres_without_a_radius(pkg):
    a = unbounded_tail_arrays(pkg)
    d = pkg.desc_from_arrays(64, 48, np.radians(S.FOV), (0.05, 0.1, 0.2), 0, a["coefs"], a["reflection"], a["albedo"], a["light_is_spherical"], a["light_p"], a["light_color"])
    osc = S.O.Scene(64, 48, 0.0, 0, (0.05, 0.1, 0.2))
    osc.vertical_fov = float(np.radians(S.FOV))
    for i in range(len(a["reflection"])):
        osc.add_object(a["coefs"][i], a["albedo"][i], a["reflection"][i])
    for i in range(2):
        osc.lights.append(R.stored_light(a["light_is_spherical"][i], a["light_p"][i], a["light_color"][i]))
    check(pkg, d, osc.render(nthreads=8), "unbounded tail")
    r = pkg.Renderer(d, device=0, flags=four(pkg))
    try:
        g = r.debug_stream_group_bounds().view(SC.US_DTYPE)
        assert len(g) == 2 and np.isfinite(g["r"][0]) and np.isposinf(g["r"][1]) and g["inv_r"][1] == 0.0
    finally:
        r.cleanup_update()


def test_fast_variant_is_its_unflagged_twin(pkg):
    """RT_FLAG_FAST, held to the flag's own rule, device against device: bit for bit the FAST frame of the context without the flag."""
    f = pkg
    for sc, extra in ((S.field(pkg, 4097, S.FIELD_SEED), 0), (S.mixed_large(pkg, 8200, S.MIXED_SEED, depth=2), f.RT_FLAG_STREAM_CULL_BOUNCE)):
        got = gframe(pkg, sc, flags=four(pkg) | extra | f.RT_FLAG_FAST)
        assert R.same(got, gframe(pkg, sc, None, False, flags=f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_CULL | extra | f.RT_FLAG_FAST))
        assert R.same(got, gframe(pkg, sc, None, False, flags=f.RT_FLAG_STREAM | f.RT_FLAG_FAST))


@pytest.mark.parametrize("fmt", [F32, U8], ids=["rgba32f", "rgba8"])
def test_supersampling(pkg, fmt):
    w, h = 40, 30
    sc = S.field(pkg, 4097, S.FIELD_SEED, w=w, h=h)
    want = ssaa_ref.resolve(S.oracle_of(pkg, sc).with_size(2 * w, 2 * h).render(nthreads=8), 2)
    want = ssaa_ref.quantise(want) if fmt == U8 else want
    got = gframe(pkg, sc, flags=four(pkg) | pkg.RT_FLAG_SSAA2, fmt=fmt)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert R.same(got, gframe(pkg, sc, None, False, flags=(four(pkg) | pkg.RT_FLAG_SSAA2) & ~pkg.RT_FLAG_STREAM_CULL_GROUPS, fmt=fmt))


def test_rank_1_of_3_with_bands_of_8(pkg):
    sc = S.field(pkg, 4097, S.FIELD_SEED, w=64, h=50)
    want = S.oracle_of(pkg, sc).render(nthreads=8)
    out = []
    for flags in (four(pkg), four(pkg) & ~pkg.RT_FLAG_STREAM_CULL_GROUPS):
        r = pkg.Renderer(sc, device=0, rank=1, world=3, band_rows=8, flags=flags)
        try:
            assert r.stream_groups == bool(flags & pkg.RT_FLAG_STREAM_CULL_GROUPS)
            r.update()
            rows = r.row_map()
            out.append(r.download().copy())
            assert 0 < len(rows) < 50 and R.same_as_oracle(out[-1][..., :3], want[rows])
        finally:
            r.cleanup_update()
    assert R.same(out[0], out[1])


def test_moved_camera(pkg):
    sc = S.field(pkg, 4097, S.FIELD_SEED)
    for cam in (pkg.camera_matrix(*MOVED), pkg.camera_matrix((6.0, 2.0, 4.0), 120.0, -9.0)):
        check(pkg, sc, S.oracle_of(pkg, sc).render(cam=cam, nthreads=8), "moved", cam=cam)


def test_multi_renderer(pkg):
    sc = S.field(pkg, 4097, S.FIELD_SEED)
    want = S.oracle_of(pkg, sc).render(nthreads=8)
    m = pkg.MultiRenderer(sc, [0, 0], band_rows=8, parts=2, flags=four(pkg))
    try:
        assert m.stream_groups is True
        for _ in range(2):
            m.update()
        assert R.same_as_oracle(m.download()[..., :3], want)
    finally:
        m.cleanup_update()
    m = pkg.MultiRenderer(sc, [0, 0], band_rows=8, parts=2, flags=four(pkg) & ~pkg.RT_FLAG_STREAM_CULL)
    try:
        assert m.stream_groups is False
    finally:
        m.cleanup_update()


ADAPTER = r"""
import ctypes as C, os, re, subprocess, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "tools"))
import __graft_entry__ as g
import stream_scenes as S
pkg = g.load_package()
sc = S.field(pkg, 4097, S.FIELD_SEED)
want = S.oracle_of(pkg, sc).render(nthreads=8)
a = sc.arrays()
upd = C.CDLL(pkg.UPDATE_LIB_PATH)
names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
update = getattr(upd, re.search(r"\b(_Z\d+updateRKN3glm3matI\S*)\b", names).group(1))
cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
update.argtypes, update.restype = [C.c_void_p], C.c_float
upd.mi355rt_update_download.argtypes = [C.c_void_p, C.c_size_t]
cam = np.ascontiguousarray(pkg.IDENTITY, dtype=np.float64)
init(7, sc._h)
ms = update(cam.ctypes.data)
out = np.zeros((a["height"], a["width"], 4), np.float32)
rc = upd.mi355rt_update_download(out.ctypes.data_as(C.c_void_p), out.nbytes)
cleanup()
print("frame", rc, ms > 0.0, bool(np.array_equal(out[..., :3].view(np.uint32), want.view(np.uint32))), bool(np.all(out[..., 3] == 1.0)))
"""


def test_init_update_with_the_environment_switch():
    """The reference's back-end contract on a fresh process: MI355RT_STREAM_CULL_GROUPS=1 beside the switches it builds on draws the oracle's
    frame of the 4 097-sphere field; any other value but 0 is refused by name."""
    def adapter(**env):
        return subprocess.run([sys.executable, "-c", ADAPTER, ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))
    out = adapter(MI355RT_STREAM="1", MI355RT_STREAM_CULL="1", MI355RT_STREAM_CULL_GROUPS="1")
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "frame 0 True True True", out.stdout
    out = adapter(MI355RT_STREAM="1", MI355RT_STREAM_CULL="1", MI355RT_STREAM_CULL_GROUPS="yes")
    assert out.returncode != 0 and "mi355rt: MI355RT_STREAM_CULL_GROUPS: expected 0 or 1" in out.stderr, (out.stdout, out.stderr)


# ---- work words -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stats_scene():
    import __graft_entry__ as graft
    pkg = graft.load_package()
    sc = G.two_clusters(pkg, mirrors=True, depth=1)
    return sc, G.primary_expectation(S.oracle_of(pkg, sc), sc.arrays())


def one_frame(r, read):
    before = read()
    r.update()
    return [y - x for x, y in zip(before, read())]


def words_of_a_frame(pkg, sc, flags):
    """(frame, rt_debug_stream_cull's words, rt_debug_stream_cull_bounce's or None, rt_debug_stream_groups' or None) of one frame."""
    r = pkg.Renderer(sc, device=0, flags=flags)
    try:
        bounce, groups = r.stream_cull_bounce, r.stream_groups
        b0 = r.stream_cull_bounce_stats() if bounce else None
        g0 = r.debug_stream_groups() if groups else None
        if groups:
            assert g0 == [0] * 8
        cull = one_frame(r, r.stream_cull_stats)
        b = [y - x for x, y in zip(b0, r.stream_cull_bounce_stats())] if bounce else None
        g = [y - x for x, y in zip(g0, r.debug_stream_groups())] if groups else None
        return r.download().copy(), cull, b, g
    finally:
        r.cleanup_update()


def held_to_the_identity(with_groups, without):
    """The words of a frame with the group flag against those of the same context without it: the same chunks are staged ([1], [3]), the same
    entries decided and swept ([4], [5]), the same queries unculled ([6]); no more chunk verdicts asked ([0], [2]); the bounce queries stage
    the same chunks ([1])."""
    (f1, c1, b1, g1), (f0, c0, b0, g0) = with_groups, without
    assert g0 is None and g1 is not None
    assert R.same(f1, f0)
    assert [c1[i] for i in (1, 3, 4, 5, 6)] == [c0[i] for i in (1, 3, 4, 5, 6)], (c1, c0)
    assert c1[0] <= c0[0] and c1[2] <= c0[2] and c1[7] == c0[7] == 0, (c1, c0)
    assert (b1 is None) == (b0 is None)
    if b1 is not None:
        assert b1[1] == b0[1] and b1[3] == b0[3] and b1[4] == b0[4] and b1[0] <= b0[0] and b1[2] <= b0[2], (b1, b0)
    assert g1[6] == g1[7] == 0 and g1[1] <= g1[0] and g1[3] <= g1[2] and g1[5] <= g1[4], g1


def test_work_words(pkg, monkeypatch):
    """Two clusters of 4 096 spheres (every third a mirror, one bounce), one group each.  The lab's exact counts from the numpy cone predicate
    asked about the group bounds: [0] and [1] of rt_debug_stream_groups, and [0] of rt_debug_stream_cull = the chunks of the entered
    groups.  Everything staged is what the context without the flag stages."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    sc, e = stats_scene()
    assert e["asked"] - e["entered"] >= e["asked"] / 4, e      # (the input's condition, before any device value is read)
    f = pkg
    base = f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_CULL | f.RT_FLAG_STREAM_CULL_BOUNCE
    with_groups, without = words_of_a_frame(pkg, sc, base | f.RT_FLAG_STREAM_CULL_GROUPS), words_of_a_frame(pkg, sc, base)
    print("expected", e, "\nwith groups", with_groups[1:], "\nwithout", without[1:])
    held_to_the_identity(with_groups, without)
    _, cull, bounce, groups = with_groups
    assert groups[0] == e["asked"] and groups[1] == e["entered"], (groups, e)
    assert cull[0] == e["chunks_asked"] and cull[1] == e["staged"] and without[1][0] == e["blocks"] * e["n_chunks"], (cull, without[1], e)
    assert groups[2] > 0 and groups[3] < groups[2]      # the shadow rays pass the other cluster by
    assert bounce is not None and groups[4] > 0 and 0 < groups[5] < groups[4] and bounce[1] < bounce[0]
    # ... and without culled bounce rays: the same identities, no bounce words
    plain = f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_CULL
    with_groups, without = words_of_a_frame(pkg, sc, plain | f.RT_FLAG_STREAM_CULL_GROUPS), words_of_a_frame(pkg, sc, plain)
    held_to_the_identity(with_groups, without)
    assert with_groups[3][:2] == [e["asked"], e["entered"]] and with_groups[3][4] == with_groups[3][5] == 0


def test_without_the_environment_switch_there_are_no_work_words(pkg, monkeypatch):
    monkeypatch.delenv("MI355RT_STREAM_CULL_STATS", raising=False)
    r = pkg.Renderer(S.field(pkg, 4097, S.FIELD_SEED), device=0, flags=four(pkg))
    try:
        assert r.stream_groups
        r.update()
        with pytest.raises(pkg.RtError) as e:
            r.debug_stream_groups()
        assert e.value.code == -1 and "rt_debug_stream_groups: the context keeps no work words (they exist where rt_get_stream_groups says 1 and " \
                                      "MI355RT_STREAM_CULL_STATS=1 was set at rt_create)" in e.value.message
        with pytest.raises(pkg.RtError):
            r.stream_cull_stats()
    finally:
        r.cleanup_update()


# ---- updates ------------------------------------------------------------------------------------------------------------------------------------
SWAPPED = (G.CENTRES[1], G.CENTRES[0])


def r_off(a):
    return SC.image(a)[2]["off_us"]


def held_to_the_lab(pkg, r, coefs, a):
    """The device's blob, chunk bounds and group bounds == what the host packs for the new scene under the context's order."""
    got = r.debug_scene_blob()
    t = got[r_off(a):r_off(a) + 64 * len(a["reflection"])].view(SC.US_DTYPE)
    blob, bounds, w = SC.image(dict(a, coefs=coefs), slot_orig=t["orig"])
    assert R.same(got[:blob.size], blob) and R.same(r.stream_bounds(), bounds)
    assert R.same(r.debug_stream_group_bounds(), G.group_image(bounds))


def test_set_scene_and_reorder(pkg):
    """rt_set_scene exchanges the clusters: the group bounds are the host's image of the new scene under the context's order.  After
    rt_reorder_scene they are a fresh context's, byte for byte; the frames are the unflagged context's throughout."""
    f = pkg
    sc, moved = G.two_clusters(pkg), G.two_clusters(pkg, centres=SWAPPED)
    a, coefs = sc.arrays(), moved.arrays()["coefs"]
    flags = four(pkg) | f.RT_FLAG_STREAM_CULL_REORDER
    want = gframe(pkg, moved, None, False, flags=f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_CULL)
    fresh = pkg.Renderer(moved, device=0, flags=flags)
    try:
        fresh_groups, fresh_bounds = fresh.debug_stream_group_bounds().copy(), fresh.stream_bounds().copy()
    finally:
        fresh.cleanup_update()
    r = pkg.Renderer(sc, device=0, flags=flags)
    try:
        assert r.stream_groups and r.stream_cull_reorder
        r.update()
        before, old_groups = r.download().copy(), r.debug_stream_group_bounds().copy()
        held_to_the_lab(pkg, r, a["coefs"], a)
        r.set_scene(coefs=coefs)
        held_to_the_lab(pkg, r, coefs, a)
        assert not R.same(r.debug_stream_group_bounds(), old_groups)
        r.update()
        stale = r.download().copy()
        r.reorder_scene()
        assert R.same(r.debug_stream_group_bounds(), fresh_groups) and R.same(r.stream_bounds(), fresh_bounds)
        r.update()
        after = r.download().copy()
        assert r.set_scene_status()["applied"] == 1
    finally:
        r.cleanup_update()
    assert not R.same(before, stale) and R.same(stale, want) and R.same(after, want)


def test_set_scene_reorder_and_frame_in_one_graph_replayed_twice(pkg):
    import torch
    f = pkg
    sc, moved = G.two_clusters(pkg), G.two_clusters(pkg, centres=SWAPPED)
    a = sc.arrays()
    steps = [moved.arrays()["coefs"], a["coefs"]]
    flags = four(pkg) | f.RT_FLAG_STREAM_CULL_REORDER
    want = [gframe(pkg, s, None, False, flags=f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_CULL) for s in (moved, sc)]
    assert not R.same(want[0], want[1])
    fresh = []
    for s in (moved, sc):
        x = pkg.Renderer(s, device=0, flags=flags)
        try:
            fresh.append(x.debug_stream_group_bounds().copy())
        finally:
            x.cleanup_update()
    r = pkg.Renderer(sc, device=0, flags=flags)
    s = torch.cuda.Stream()
    try:
        r.update(stream=s.cuda_stream, timed=False)
        with torch.cuda.stream(s):
            arr = torch.from_numpy(steps[0].copy()).to("cuda:0")
            buf = torch.empty((r.local_rows, r.width, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            r.set_scene_into(coefs=arr.data_ptr(), stream=s.cuda_stream, reorder=True)
            r.update(dev_fb=buf.data_ptr(), stream=s.cuda_stream, timed=False)
        for rep in range(2):
            with torch.cuda.stream(s):
                arr.copy_(torch.from_numpy(steps[rep].copy()))
                buf.view(torch.int32).fill_(0x7FC00000)
                g.replay()
            s.synchronize()
            assert R.same(buf.cpu().numpy(), want[rep]), rep
            assert R.same(r.debug_stream_group_bounds(), fresh[rep]), rep
        assert r.set_scene_status()["applied"] == 2
        del g
    finally:
        torch.cuda.synchronize()
        r.cleanup_update()


# ---- beyond 64 groups -----------------------------------------------------------------------------------------------------------------------------
def test_the_second_trip_of_the_group_loop(pkg, monkeypatch):
    """262 145 unit spheres at 16 x 16: 4 097 chunks, 65 groups -- lane 0 of the second block of 64 groups holds the last one.  Device against
    device: the flagged frame and words against the culled unflagged context's."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    d, _ = G.big_field(pkg, 262145, 5)
    f = pkg
    base = f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_CULL
    r = pkg.Renderer(d, device=0, flags=base | f.RT_FLAG_STREAM_CULL_GROUPS)
    try:
        assert r.stream_groups and r.debug_stream_group_bounds().size == 65 * 64 and r.stream_bounds().size == 4097 * 64
    finally:
        r.cleanup_update()
    with_groups, without = words_of_a_frame(pkg, d, base | f.RT_FLAG_STREAM_CULL_GROUPS), words_of_a_frame(pkg, d, base)
    print("with groups", with_groups[1:], "\nwithout", without[1:])
    held_to_the_identity(with_groups, without)
    assert with_groups[3][0] == 4 * 65 and without[1][0] == 4 * 4097 and with_groups[1][1] > 0
    assert (with_groups[0][..., :3] != with_groups[0][0, 0, :3]).any()


# ---- untouched paths ----------------------------------------------------------------------------------------------------------------------------
def test_queries_and_adaptive_frames_on_a_groups_context(pkg):
    """One pixel query, one ray query and a streamed adaptive frame of a groups context equal the unflagged context's: those kernels keep
    their chunk loops."""
    f = pkg
    sc = S.field(pkg, 4097, S.FIELD_SEED, mirrors=True, depth=1)
    rng = np.random.default_rng(3)
    o = np.zeros((300, 3)) + rng.normal(scale=0.05, size=(300, 3))
    d = np.stack([rng.uniform(-0.6, 0.6, 300), rng.uniform(-0.45, 0.45, 300), np.ones(300)], axis=1)
    base = f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_CULL | f.RT_FLAG_STREAM_QUERIES | f.RT_FLAG_STREAM_CULL_RAYS | f.RT_FLAG_STREAM_CULL_PIXELS
    out = []
    for flags in (base | f.RT_FLAG_STREAM_CULL_GROUPS, base):
        r = pkg.Renderer(sc, device=0, flags=flags)
        try:
            assert r.stream_groups == bool(flags & f.RT_FLAG_STREAM_CULL_GROUPS) and r.stream_cull_rays and r.stream_cull_pixels
            r.update()
            rec = {"frame": r.download().copy(), "pick": r.pick([(x, y) for y in range(0, 48, 5) for x in range(0, 64, 7)]), "trace": r.trace(o, d)}
            out.append(rec)
        finally:
            r.cleanup_update()
    for key in out[0]:
        x, y = np.ascontiguousarray(out[0][key]), np.ascontiguousarray(out[1][key])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), key
    assert (out[0]["trace"]["object"] >= 0).any()
    base = f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_CULL | f.RT_FLAG_SSAA2 | f.RT_FLAG_SSAA_ADAPTIVE | f.RT_FLAG_STREAM_ADAPTIVE
    got = []
    for flags in (base | f.RT_FLAG_STREAM_CULL_GROUPS, base):
        r = pkg.Renderer(sc, device=0, flags=flags)
        try:
            assert r.stream_groups == bool(flags & f.RT_FLAG_STREAM_CULL_GROUPS) and r.streamed_adaptive and r.stream_cull_adaptive
            r.update()
            got.append((r.download().copy(), r.refined))
        finally:
            r.cleanup_update()
    assert got[0][1] == got[1][1] > 0 and R.same(got[0][0], got[1][0])


# ---- the instantiation that is not built ----------------------------------------------------------------------------------------------------------
def cubic_quadric_and_field(pkg, w=48, h=36):
    """A shipped degree-3 scene made a mirror, one reflecting ellipsoid with cross terms and the mirrored 4 097-sphere field: the kernels for
    general quadrics AND degree 3, two groups, culled bounce rays."""
    a = pkg.Scene.load_from_file(scene_path("clebsch")).set_size(w, h).arrays()
    fl = S.field(pkg, 4097, S.FIELD_SEED, w=w, h=h, mirrors=True, depth=2).arrays()
    coefs = np.concatenate([a["coefs"], fl["coefs"], S.ellipsoid(np.array([3.0, 2.0, 18.0]), np.array([1.5, 0.8, 1.1]), np.array([0.3, -0.2, 0.1]))[None, :]])
    refl = np.concatenate([np.full(len(a["reflection"]), 0.5, np.float32), fl["reflection"], np.array([0.3], np.float32)]).astype(np.float32)
    alb = np.concatenate([a["albedo"], fl["albedo"], np.array([[0.9, 0.6, 0.3]], np.float32)]).astype(np.float32)
    return pkg.desc_from_arrays(w, h, a["vertical_fov"], a["bg_color"], 2, coefs, refl, alb, a["light_is_spherical"], a["light_p"], a["light_color"])


def test_general_quadrics_plus_degree_3(pkg, monkeypatch):
    """The <1, 1> instantiations, strict and fast, with and without culled bounce rays: the frames are the unflagged contexts'.  The kernel
    that counts AND culls bounce rays for this pair is not built: with the work words asked for the decision is false, and the context is
    the one without the flag, words included."""
    f = pkg
    d = cubic_quadric_and_field(pkg)
    monkeypatch.delenv("MI355RT_STREAM_CULL_STATS", raising=False)
    for extra in (0, f.RT_FLAG_STREAM_CULL_BOUNCE, f.RT_FLAG_STREAM_CULL_BOUNCE | f.RT_FLAG_FAST):
        got = gframe(pkg, d, flags=four(pkg) | extra)
        assert R.same(got, gframe(pkg, d, None, False, flags=(four(pkg) | extra) & ~f.RT_FLAG_STREAM_CULL_GROUPS)), extra
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    counted = words_of_a_frame(pkg, d, four(pkg))      # (no culled bounce rays: the counting kernel exists)
    assert counted[3] is not None and counted[3][0] > 0
    r = pkg.Renderer(d, device=0, flags=four(pkg) | f.RT_FLAG_STREAM_CULL_BOUNCE)
    try:
        assert r.stream_cull_bounce and r.stream_groups is False and r.debug_stream_group_bounds().size == 0
        r.update()
        assert r.stream_cull_stats()[0] > 0 and r.stream_cull_bounce_stats()[0] > 0
        assert R.same(r.download(), counted[0])
    finally:
        r.cleanup_update()
