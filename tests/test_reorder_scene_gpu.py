"""rt_reorder_scene on the GPU (RT_FLAG_STREAM_CULL_REORDER; csrc/rt_reorder_scene.hip).  A context created on S0 and
moved to S1 by rt_set_scene holds S1's entries in S0's slots (the existing rule); after rt_reorder_scene its blob and chunk bounds are,
byte for byte, what a fresh rt_create of S1 uploads (stream_cull_lab.image), and every frame and query is bit for bit what it was.  The
host-side conditions (the stale order really is worse on these scenes) are in tests/test_reorder_scene_host.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, compare

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import raw_desc_scenes as R  # noqa: E402
import reorder_lab as RL  # noqa: E402
from test_raw_descriptor_gpu import rgba8_of  # noqa: E402

SC, S = RL.SC, RL.S
pytestmark = pytest.mark.gpu

F32, U8 = 0, 1
# The switches of csrc/rt_reorder_scene.hip, one n_us on each side (test_past_the_internal_switches):
TILE = 2048            # RO_TILE: one workgroup ranks 2048 items per pass -> 2048 is one tile, 2049 two
SCAN_LEVELS = 16384    # 8 tiles x 256 digits = RO_SCAN_CHUNK table entries: one scan level up to here, two from 16385
ORIG_BYTES = 256       # n_obj - 1 fits one byte up to 256 objects: one pass over orig, two from 257 (65 537 would take three: the bench's 100 000 does)
# ... and with MI355RT_REORDER_MAX_GRID=1 every grid is ONE workgroup that loops: the second trip of the per-entry grids starts at 257 entries
# (permute: 65), of the per-tile grids at 2049, of the bounds grid at 4097 (64 chunks a workgroup), of the scan-chunk grid at 16385
ONE_WORKGROUP_SIZES = (257, 2049, 4097, 16385)


@pytest.fixture(autouse=True)
def the_feature(pkg):
    assert pkg.RT_FLAG_STREAM_CULL_REORDER == 8388608 and hasattr(pkg.Renderer, "reorder_scene")


def flags3(pkg):
    return pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_REORDER


@functools.lru_cache(maxsize=None)
def pair(n, mirrors=False, depth=0):
    """(S0, its arrays, S1's coefficients) of the mix at n spheres."""
    import __graft_entry__ as graft
    pkg = graft.load_package()
    ub = RL.UNBOUNDED_AT if n == 320 else ()
    sc = RL.base_scene(pkg, n, ub, mirrors=mirrors, depth=depth)
    a = sc.arrays()
    return sc, a, RL.mix(a["coefs"], unbounded=ub)


def device_image(r, blob_bytes):
    return r.debug_scene_blob()[:blob_bytes], r.stream_bounds()


def held_to(r, image, what):
    blob, bounds, w = image
    got, got_bounds = device_image(r, blob.size)
    assert R.same(SC.table_of(got, w)["orig"], SC.table_of(blob, w)["orig"]), (what, "orig column")
    assert R.same(got, blob), (what, "blob")
    assert R.same(got_bounds, bounds), (what, "bounds")


def bytes_before_and_after(pkg, sc, a, coefs, what, check_stale=True):
    """create on S0, set_scene(S1): the stale image and not the fresh one; reorder_scene(): the fresh image; again: nothing changes."""
    stale, fresh = RL.stale(a, coefs), RL.fresh(a, coefs)
    assert not R.same(stale[0], fresh[0]), what
    r = pkg.Renderer(sc, device=0, flags=flags3(pkg))
    try:
        assert r.stream_cull and r.stream_cull_reorder
        r.set_scene(coefs=coefs)
        if check_stale:
            held_to(r, stale, (what, "stale"))
        assert not R.same(device_image(r, fresh[0].size)[0], fresh[0]), what
        r.reorder_scene()
        held_to(r, fresh, (what, "reordered"))
        r.reorder_scene()
        held_to(r, fresh, (what, "reordered twice"))
        assert r.set_scene_status()["applied"] == 1
    finally:
        r.cleanup_update()


# ---- 1. bytes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RL.SIZES)
def test_bytes(pkg, n):
    sc, a, coefs = pair(n)
    if n == 320:
        t = SC.table_of(*RL.fresh(a, coefs)[::2])
        assert (~np.isfinite(t["r"])).sum() == 3 and sorted(t["orig"][-3:].tolist()) == sorted(RL.UNBOUNDED_AT)
    bytes_before_and_after(pkg, sc, a, coefs, n)


# ---- 2. ties and flat boxes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["two", "plane", "identical"])
def test_ties_and_flat_boxes(pkg, kind):
    sc, a, _ = pair(65)
    bytes_before_and_after(pkg, sc, a, RL.ties(a["coefs"], kind), kind)


# ---- 3. frames -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast,fmt", [(False, F32), (True, F32), (False, U8)], ids=["strict-rgba32f", "fast-rgba32f", "strict-rgba8"])
def test_frames(pkg, fast, fmt):
    """The frame after the reorder == a fresh context's on S1 == the stale frame before the reorder, bit for bit; and the oracle's: strict frames
    bit for bit (same_as_oracle; RGBA8: the oracle's quantisation), RT_FLAG_FAST frames to that build's own bar (1e-5 relative, at most
    max(2, 0.2 % of the pixels) beyond it: a contracted build is not defined as the oracle's bits)."""
    sc, a, coefs = pair(129, True, 2)
    s1 = RL.scene_with(pkg, sc, coefs)
    flags = flags3(pkg) | (pkg.RT_FLAG_FAST if fast else 0)
    want = S.oracle_of(pkg, s1).render(nthreads=8)
    f = pkg.Renderer(s1, device=0, flags=flags, fmt=fmt)
    try:
        f.update()
        fresh = f.download().copy()
    finally:
        f.cleanup_update()
    r = pkg.Renderer(sc, device=0, flags=flags, fmt=fmt)
    try:
        r.update()
        first = r.download().copy()
        r.set_scene(coefs=coefs)
        r.update()
        stale = r.download().copy()
        r.reorder_scene()
        r.update()
        after = r.download().copy()
        held_to(r, RL.fresh(a, coefs), "frames")
    finally:
        r.cleanup_update()
    assert not R.same(first, stale)
    assert R.same(after, fresh) and R.same(after, stale)
    if fmt == U8:
        q, ok = rgba8_of(want)
        assert after.dtype == np.uint8 and not ((after != q)[..., :3] & ok).any() and np.all(after[..., 3] == 255)
    elif fast:
        c = compare(after[..., :3], want)
        print("RT_FLAG_FAST against the oracle:", c, "bit-equal:", R.same_as_oracle(after[..., :3], want))
        assert c["n_bad_pixels"] <= max(2, int(0.002 * RL.W * RL.H)), c
    else:
        assert R.same_as_oracle(after[..., :3], want), R.n_diff(after[..., :3], want)


# ---- 4. work words -----------------------------------------------------------------------------------------------------------------------------
def test_work_words(pkg, monkeypatch):
    """One frame's words after the reorder == a fresh context's on S1, exactly; chunks staged for primary rays [1] and for shadow rays [3]
    strictly below the stale context's."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    sc, a, coefs = pair(257)
    s1 = RL.scene_with(pkg, sc, coefs)

    def one_frame(r):
        before = r.stream_cull_stats()
        r.update()
        return [y - x for x, y in zip(before, r.stream_cull_stats())]

    f = pkg.Renderer(s1, device=0, flags=flags3(pkg))
    try:
        fresh = one_frame(f)
    finally:
        f.cleanup_update()
    r = pkg.Renderer(sc, device=0, flags=flags3(pkg))
    try:
        r.update()
        r.set_scene(coefs=coefs)
        stale = one_frame(r)
        r.reorder_scene()
        after = one_frame(r)
    finally:
        r.cleanup_update()
    print("work words: stale", stale, "reordered", after, "fresh", fresh)
    assert after == fresh
    assert after[1] < stale[1] and after[3] < stale[3]       # fewer chunks staged, for primary and for shadow rays


# ---- 5. graph ------------------------------------------------------------------------------------------------------------------------------------
def test_set_scene_reorder_and_frame_in_one_graph_replayed_twice(pkg):
    import torch
    sc, a, coefs = pair(129)
    steps = [coefs, a["coefs"]]
    fresh_frames = []
    for c in steps:
        f = pkg.Renderer(RL.scene_with(pkg, sc, c), device=0, flags=flags3(pkg))
        try:
            f.update()
            fresh_frames.append(f.download().copy())
        finally:
            f.cleanup_update()
    assert not R.same(fresh_frames[0], fresh_frames[1])
    r = pkg.Renderer(sc, device=0, flags=flags3(pkg))
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
            assert R.same(buf.cpu().numpy(), fresh_frames[rep]), rep
            held_to(r, RL.fresh(a, steps[rep]), ("graph", rep))
        assert r.set_scene_status()["applied"] == 2
        del g
    finally:
        torch.cuda.synchronize()
        r.cleanup_update()


# ---- 6. every consumer of the order -------------------------------------------------------------------------------------------------------------
def as_bytes(x):
    if isinstance(x, (tuple, list)):
        return b"|".join(as_bytes(v) for v in x)
    if isinstance(x, dict):
        return b"|".join(as_bytes(x[k]) for k in sorted(x))
    if x is None or isinstance(x, (int, float)):
        return repr(x).encode()
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    x = np.ascontiguousarray(x)
    return str((x.shape, x.dtype)).encode() + x.tobytes()


def consumer_records(r):
    rng = np.random.default_rng(3)
    o = np.zeros((300, 3)) + rng.normal(scale=0.05, size=(300, 3))
    d = np.stack([rng.uniform(-0.6, 0.6, 300), rng.uniform(-0.45, 0.45, 300), np.ones(300)], axis=1)
    xy = [(x, y) for y in range(0, RL.H, 5) for x in range(0, RL.W, 7)]
    rec = {}
    rec["trace"] = r.trace(o, d)
    rec["occluded"] = r.occluded(o, d, timed=False)[0]
    rec["shade"] = r.shade(o, d)
    rec["paths"] = r.paths(o, d)
    rec["gbuffer"] = r.gbuffer(timed=False)[:3]
    rec["pick"] = r.pick(xy)
    rec["object_extents"] = r.object_extents()
    r.update()
    rec["frame"] = r.download().copy()
    return rec


def test_every_consumer_of_the_order(pkg):
    """129 spheres, every culling flag and streamed queries: after set_scene + reorder each call == the same call on a fresh context."""
    sc, a, coefs = pair(129, True, 2)
    s1 = RL.scene_with(pkg, sc, coefs)
    every = (flags3(pkg) | pkg.RT_FLAG_STREAM_QUERIES | pkg.RT_FLAG_STREAM_CULL_BOUNCE | pkg.RT_FLAG_STREAM_CULL_RAYS | pkg.RT_FLAG_STREAM_CULL_PIXELS)
    adaptive = every | pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA_ADAPTIVE | pkg.RT_FLAG_STREAM_ADAPTIVE
    for flags, what in ((every, "queries and the mirrored frame"), (adaptive, "one adaptive frame")):
        out = []
        for scene, moved in ((sc, True), (s1, False)):
            r = pkg.Renderer(scene, device=0, flags=flags)
            try:
                assert r.stream_cull and r.stream_cull_reorder
                if flags == every:
                    assert r.stream_cull_bounce and r.stream_cull_rays and r.stream_cull_pixels and r.streamed_queries
                else:
                    assert r.stream_cull_adaptive
                if moved:
                    r.update()
                    r.set_scene(coefs=coefs, reorder=True)
                    held_to(r, RL.fresh(a, coefs), what)
                if flags == every:
                    out.append(consumer_records(r))
                else:
                    r.update()
                    out.append(dict(frame=r.download().copy(), refined=int(r.refined)))
            finally:
                r.cleanup_update()
        if flags == every:
            assert (out[0]["trace"]["object"] >= 0).any() and np.asarray(out[0]["occluded"].cpu()).any()
        else:
            assert out[0]["refined"] > 0
        for key in out[0]:
            assert as_bytes(out[0][key]) == as_bytes(out[1][key]), (what, key)


# ---- 7. decision false ---------------------------------------------------------------------------------------------------------------------------
def test_decision_false_is_the_context_without_the_flag(pkg):
    """The flag without RT_FLAG_STREAM_CULL, and on three cullable spheres (culling is off below four): nothing differs from the unflagged context."""
    cases = ((pair(129)[0], pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL_REORDER, pkg.RT_FLAG_STREAM),
             (RL.base_scene(pkg, 3), flags3(pkg), pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL))
    for sc, flags, plain in cases:
        coefs = RL.mix(sc.arrays()["coefs"])
        r, p = pkg.Renderer(sc, device=0, flags=flags), pkg.Renderer(sc, device=0, flags=plain)
        try:
            assert r.stream_cull_reorder is False and p.stream_cull_reorder is False and r.stream_cull is False
            assert r.stream_bounds().size == 0
            for x in (r, p):
                x.update()
                x.set_scene(coefs=coefs)
            before = r.debug_scene_blob().copy()
            assert R.same(before, p.debug_scene_blob())
            r.reorder_scene()
            assert R.same(r.debug_scene_blob(), before)
            for x in (r, p):
                x.update()
            assert R.same(r.download(), p.download())
        finally:
            r.cleanup_update()
            p.cleanup_update()


# ---- 8. past the internal switches ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big(n):
    """(S0, arrays, S1's coefficients) of a field of n spheres: dense, so few pixels a sphere -- only bytes are asked of these."""
    import __graft_entry__ as graft
    pkg = graft.load_package()
    sc = S.field(pkg, n, S.FIELD_SEED, px=0.6)
    a = sc.arrays()
    return sc, a, RL.mix(a["coefs"])


@pytest.mark.parametrize("n", [TILE, TILE + 1, SCAN_LEVELS, SCAN_LEVELS + 1])
def test_past_the_internal_switches(pkg, n):
    """RO_TILE (2048 | 2049: one tile | two) and the scan's levels (16384 | 16385: one | two); ORIG_BYTES (256 | 257 objects: one | two passes
    over orig) lies between test_bytes' 129 and 257."""
    sc, a, coefs = big(n)
    bytes_before_and_after(pkg, sc, a, coefs, n, check_stale=False)


@pytest.mark.parametrize("n", ONE_WORKGROUP_SIZES)
def test_grids_of_one_workgroup_loop(pkg, monkeypatch, n):
    """MI355RT_REORDER_MAX_GRID=1: every grid is one workgroup that takes the second trip of its loop at these sizes (the grid caps)."""
    monkeypatch.setenv("MI355RT_REORDER_MAX_GRID", "1")
    sc, a, coefs = pair(n) if n == 257 else big(n)
    bytes_before_and_after(pkg, sc, a, coefs, n, check_stale=False)


def test_ten_thousand_spheres(pkg):
    """Bytes and one frame at 10 000 spheres."""
    sc, a, coefs = big(RL.MANY)
    fresh = RL.fresh(a, coefs)
    f = pkg.Renderer(RL.scene_with(pkg, sc, coefs), device=0, flags=flags3(pkg))
    try:
        f.update()
        want = f.download().copy()
    finally:
        f.cleanup_update()
    r = pkg.Renderer(sc, device=0, flags=flags3(pkg))
    try:
        r.set_scene(coefs=coefs)
        assert not R.same(device_image(r, fresh[0].size)[0], fresh[0])
        r.reorder_scene()
        held_to(r, fresh, RL.MANY)
        r.update()
        assert R.same(r.download(), want)
    finally:
        r.cleanup_update()


# ---- 9. multi ------------------------------------------------------------------------------------------------------------------------------------------
_MULTI_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "tools"))
import numpy as np
import __graft_entry__ as graft
import reorder_lab as RL
pkg = graft.load_package()
flags = pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_REORDER
sc = RL.base_scene(pkg, 129)
a = sc.arrays()
coefs = RL.mix(a["coefs"])
one = pkg.Renderer(sc, device=0, flags=flags)
one.update()
one.set_scene(coefs=coefs, reorder=True)
one.update()
want = one.download().copy()
one.cleanup_update()
m = pkg.MultiRenderer(sc, [0], band_rows=8, parts=2, flags=flags | pkg.RT_MULTI_SELF_EXCHANGE)
assert m.transport == "rccl", m.transport
m.update()
m.set_scene(coefs=coefs)
m.reorder_scene()
m.update()
got = m.download()
assert m.set_scene_status()["applied"] == 1
blob, bounds, w = RL.fresh(a, coefs)
assert m.query.stream_cull_reorder and np.array_equal(m.query.debug_scene_blob()[:blob.size], blob) and np.array_equal(m.query.stream_bounds(), bounds)
assert got.tobytes() == want.tobytes()
m.cleanup_update()
print("multi reorder ok")
"""


def test_multi_renderer_with_self_exchange(pkg):
    """rt_set_scene_multi + rt_reorder_scene_multi on one device exchanging with itself (a child process of its own, like the other RCCL tests):
    the frame is the single context's, and the root's context holds the fresh image."""
    p = subprocess.run([sys.executable, "-c", _MULTI_CHILD, ROOT], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "multi reorder ok" in p.stdout
