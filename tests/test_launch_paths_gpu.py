"""Which launcher does an entry point reach?  Every table path of a query returns the same bits, so parity cannot say;
the work words can: a culled launcher adds to its own family's eight words and to no other's.  One scene of three chunks, one context with every
culling flag and MI355RT_STREAM_CULL_STATS=1: after each entry point exactly its families' words have advanced.  Every output equals, bit for
bit, the output of the same context without the culling flags.  The source-text half is tests/test_launch_paths_host.py."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import stream_cull_lab as SC  # noqa: E402
import stream_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 64, 48
N_SPHERES = 130      # ceil(130 / 64) = 3 chunks: every decision needs at least two
FAMILIES = ("stream_cull", "stream_cull_bounce", "stream_cull_adaptive", "stream_cull_rays", "stream_cull_pixels")
# 256 pixels spread over the frame; their primary rays are the 256 caller-supplied rays
XY = np.array([(2 + 4 * i, 1 + 3 * j) for j in range(16) for i in range(16)], dtype=np.uint32)


def scene(pkg):
    """130 unit spheres on a jittered 13 x 10 grid that fills the view at depths 20 .. 30, a mirror wall behind them, one point light; one bounce."""
    rng = np.random.default_rng(35)
    sc = pkg.Scene.new(W, H, S.FOV, 1, (0.05, 0.1, 0.2))
    for k in range(N_SPHERES):
        c = [(k % 13 - 6) * 2.3 + rng.uniform(-0.1, 0.1), (k // 13 - 4.5) * 2.3 + rng.uniform(-0.1, 0.1), rng.uniform(20.0, 30.0)]
        sc.add_object(pkg.surface_make("sphere", c, [1.0]), rng.uniform(0.2, 1.0, 3), 0.0)
    sc.add_object(pkg.surface_make("plane", [0.0, 0.0, 40.0], [0.0, 0.0, -1.0]), (0.6, 0.6, 0.6), 0.5)
    sc.add_light("spherical", [4.0, 30.0, 2.0], (0.8, 0.9, 1.0), 500.0)
    return sc


@functools.lru_cache(maxsize=None)
def rays_and_their_chunks():
    """On the CPU: the primary rays of XY (the oracle's), and the chunks of the context's ordered unit-sphere table (the library's own host
    functions, tests/tools/stream_cull_lab.py) that hold the spheres the oracle says those rays hit."""
    import __graft_entry__ as graft
    pkg = graft.load_package()
    sc = scene(pkg)
    own = S.Owners(S.oracle_of(pkg, sc))
    blob, _, words = SC.image(sc.arrays())
    assert words["n_us"] == N_SPHERES and words["n_chunks"] == 3 and words["cull"]
    chunk_of = {int(orig): slot // SC.CHUNK for slot, orig in enumerate(SC.table_of(blob, words)["orig"])}
    owners = [own.owner(int(x), int(y)) for x, y in XY]
    dirs = np.array([own.dirs[int(y), int(x)] for x, y in XY])
    return dirs, sorted({chunk_of[k] for k in owners if 0 <= k < N_SPHERES}), sum(k == N_SPHERES for k in owners)


def flags_of(pkg, fast):
    plain = pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_QUERIES | (pkg.RT_FLAG_FAST if fast else 0)
    culls = pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_BOUNCE | pkg.RT_FLAG_STREAM_CULL_RAYS | pkg.RT_FLAG_STREAM_CULL_PIXELS
    return plain, culls


def words(pkg, r):
    """The work words of all five families; None for a family that keeps none."""
    out = {}
    for name in FAMILIES:
        try:
            out[name] = getattr(r, name + "_stats")()
        except pkg.RtError:
            out[name] = None
    return out


def advanced(before, after):
    """The families whose words grew; no word of any family may shrink, and a family keeps its words or keeps none."""
    grown = set()
    for name in FAMILIES:
        assert (before[name] is None) == (after[name] is None), name
        if before[name] is not None:
            assert all(a >= b for a, b in zip(after[name], before[name])), (name, before[name], after[name])
            if after[name] != before[name]:
                grown.add(name)
    return grown


def entry_points(pkg, dirs):
    """(name, the families it belongs to, call) for every entry point; a call returns the bytes of everything it produced."""
    import torch
    origin = np.zeros(3)

    def planes(r):
        o, t, n, _ = r.gbuffer()
        return b"".join(p.cpu().numpy().tobytes() for p in (o, t, n))

    def extents_device(r):
        out = torch.zeros((N_SPHERES + 1) * 5, dtype=torch.int64, device="cuda")      # 40 bytes per record
        r.object_extents_into(None, None, out.data_ptr())
        return out.cpu().numpy().tobytes()

    def frame(r):
        r.update()
        return r.download().tobytes()

    pixels, rays = {"stream_cull_pixels"}, {"stream_cull_rays"}
    return [("rt_render", {"stream_cull", "stream_cull_bounce"}, frame),
            ("rt_render_gbuffer", pixels, planes),
            ("rt_pick", pixels, lambda r: r.pick(XY).tobytes()),
            ("rt_object_extents_host", pixels, lambda r: r.object_extents().tobytes()),
            ("rt_object_extents", pixels, extents_device),
            ("rt_trace_rays", rays, lambda r: r.trace(origin, dirs).tobytes()),
            ("rt_occluded_rays", rays, lambda r: r.occluded(origin, dirs)[0].cpu().numpy().tobytes()),
            ("rt_shade_rays", rays, lambda r: r.shade(origin, dirs).tobytes()),
            ("rt_trace_paths", rays, lambda r: b"".join(a.tobytes() for a in r.paths(origin, dirs))),
            ("rt_pick_paths", rays, lambda r: b"".join(a.tobytes() for a in r.pick_paths(XY)))]


@pytest.mark.parametrize("fast", [False, True], ids=["strict", "fast"])
def test_every_entry_point_advances_exactly_its_own_families(pkg, monkeypatch, fast):
    dirs, chunks_hit, on_the_mirror = rays_and_their_chunks()
    assert len(chunks_hit) >= 2 and on_the_mirror > 0, (chunks_hit, on_the_mirror)      # (otherwise the words' advance proves nothing)
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    plain, culls = flags_of(pkg, fast)
    sc = scene(pkg)
    r, twin = pkg.Renderer(sc, device=0, flags=plain | culls), pkg.Renderer(sc, device=0, flags=plain)
    try:
        assert r.streamed and r.streamed_queries and r.stream_cull and r.stream_cull_bounce and r.stream_cull_rays and r.stream_cull_pixels and not r.stream_cull_adaptive
        assert twin.streamed and twin.streamed_queries and not any(getattr(twin, name) for name in FAMILIES)
        assert all(v is None for v in words(pkg, twin).values())
        before = words(pkg, r)
        assert before == dict({name: [0] * 8 for name in FAMILIES}, stream_cull_adaptive=None)
        for name, families, call in entry_points(pkg, dirs):
            got = call(r)
            after = words(pkg, r)
            print(name, {k: v for k, v in after.items() if v != before[k]})
            assert advanced(before, after) == families, (name, before, after)
            assert got == call(twin), name
            before = after
    finally:
        r.cleanup_update()
        twin.cleanup_update()


@pytest.mark.parametrize("fast", [False, True], ids=["strict", "fast"])
def test_the_g_pass_of_an_adaptive_frame_is_streamed_not_culled(pkg, monkeypatch, fast):
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    plain, culls = flags_of(pkg, fast)
    plain |= pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA_ADAPTIVE | pkg.RT_FLAG_SSAA_GEOMETRY | pkg.RT_FLAG_STREAM_ADAPTIVE
    sc = scene(pkg)
    r, twin = pkg.Renderer(sc, device=0, flags=plain | culls), pkg.Renderer(sc, device=0, flags=plain)
    try:
        assert r.streamed_adaptive and all(getattr(r, name) for name in FAMILIES)
        assert twin.streamed_adaptive and not any(getattr(twin, name) for name in FAMILIES)
        before = words(pkg, r)
        assert before == {name: [0] * 8 for name in FAMILIES}
        r.update()
        frame, refined = r.download().tobytes(), r.refined
        after = words(pkg, r)
        print("adaptive frame", {k: v for k, v in after.items() if v != before[k]}, "refined", refined)
        assert refined > 0
        assert advanced(before, after) == {"stream_cull", "stream_cull_bounce", "stream_cull_adaptive"}, after      # the pixels family's words stand: the G pass did not cull
        twin.update()
        assert frame == twin.download().tobytes() and refined == twin.refined
    finally:
        r.cleanup_update()
        twin.cleanup_update()
