"""The two counters behind a context's frame-to-frame state start over late in its life: the tile-word tag at 0x1FFFFFF0 (the 5th hour
at 29 600 frames/s) and the frame number of the split tiles' "entered by" words at 0xFFFFFFF0 (about 40 hours in); both clear their
words first.  MI355RT_DEBUG_TAG0 / MI355RT_DEBUG_FRAME0 start a context just in front of a restart.  Expected frames are those of
tests/test_graph_replay_gpu.py: a context without frame state, held to the oracle there; every comparison is bit for bit."""
import numpy as np
import pytest

from test_graph_replay_gpu import COUNTER_KEYS, Replayed, expected, new_buffer, oracle_counters, poison, same, scene_case

pytestmark = pytest.mark.gpu

KEY = "20spheres"   # at 640 x 360: the size at which tiles are split
TAG_LIMIT, FRAME_LIMIT = 0x1FFFFFF0, 0xFFFFFFF0


def cut_frames(pkg):
    """Eight frames of cuts between the three views of camera_cut_sequence; a context that starts three short of a restart takes it
    with frame 3: between a full view and an empty one."""
    away, front, side = scene_case(pkg, KEY)[1][3:6]
    return [front, front, front, away, front, side, away, front]


def late_renderer(pkg, monkeypatch, tag0=None, frame0=None, **kw):
    """A context that starts at tile-word tag `tag0` / frame number `frame0`; the variables are read by rt_create only."""
    if tag0 is not None:
        monkeypatch.setenv("MI355RT_DEBUG_TAG0", hex(tag0))
    if frame0 is not None:
        monkeypatch.setenv("MI355RT_DEBUG_FRAME0", str(frame0))
    try:
        return pkg.Renderer(scene_case(pkg, KEY)[0], device=0, **kw)
    finally:
        monkeypatch.delenv("MI355RT_DEBUG_TAG0", raising=False)
        monkeypatch.delenv("MI355RT_DEBUG_FRAME0", raising=False)


def render_into_poison(r, cam):
    """One frame into a poisoned buffer of its own (a tile nobody wrote shows)."""
    import torch
    buf = new_buffer(r)
    poison([buf])
    r.update(cam, dev_fb=buf.data_ptr(), timed=False)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


# ---- 1. the tag restart ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["rgba32f", "rgba8", "rank1of2"])
def test_tag_restart(pkg, monkeypatch, variant):
    monkeypatch.delenv("MI355RT_LEAN", raising=False)
    fmt = pkg.RT_FMT_RGBA8 if variant == "rgba8" else pkg.RT_FMT_RGBA32F
    kw = dict(rank=1, world=2) if variant == "rank1of2" else {}
    r = late_renderer(pkg, monkeypatch, tag0=TAG_LIMIT - 3, fmt=fmt, **kw)
    rows = r.row_map() if kw else slice(None)
    for i, cam in enumerate(cut_frames(pkg)):
        assert same(render_into_poison(r, cam), expected(pkg, KEY, cam, fmt)[rows]), f"frame {i}"
    r.cleanup_update()


# ---- 2. the restart of the split tiles' frame number -----------------------------------------------------------------------------
def test_ord_frame_restart(pkg, monkeypatch):
    """Default flags, so that tiles are split; stepped alongside a RT_FLAG_NOSPLIT context, as test_half_tiles_do_not_change_the_frame
    does, and against the stateless frames."""
    monkeypatch.delenv("MI355RT_LEAN", raising=False)
    ra = late_renderer(pkg, monkeypatch, frame0=FRAME_LIMIT - 3)
    rb = pkg.Renderer(scene_case(pkg, KEY)[0], device=0, flags=pkg.RT_FLAG_NOSPLIT)
    for i, cam in enumerate(cut_frames(pkg)):
        a, b = render_into_poison(ra, cam), render_into_poison(rb, cam)
        assert same(a, b), f"frame {i}: with and without half tiles"
        assert same(a, expected(pkg, KEY, cam)), f"frame {i}"
    ra.cleanup_update()
    rb.cleanup_update()


def test_counters_on_the_full_view_after_the_ord_frame_restart(pkg, oracle, monkeypatch):
    monkeypatch.delenv("MI355RT_LEAN", raising=False)
    frames = cut_frames(pkg)
    r = late_renderer(pkg, monkeypatch, frame0=FRAME_LIMIT - 3, flags=pkg.RT_FLAG_COUNT)
    for cam in frames[:5]:   # frame 3 restarts the number, frame 4 is the next full view
        r.update(cam)
    cnt = r.counters()
    r.cleanup_update()
    ocnt = oracle_counters(oracle, KEY, 640, 360, None, frames[4].tobytes())
    got = {k: cnt[k] for k in COUNTER_KEYS}
    want = {k: ocnt["normals" if k == "hits" else k] for k in COUNTER_KEYS}
    assert got == want


# ---- 3. both restarts in one context ---------------------------------------------------------------------------------------------
def test_both_restarts_in_one_context(pkg, monkeypatch):
    monkeypatch.delenv("MI355RT_LEAN", raising=False)
    away, front, side = scene_case(pkg, KEY)[1][3:6]
    r = late_renderer(pkg, monkeypatch, tag0=TAG_LIMIT - 3, frame0=FRAME_LIMIT - 3)
    for i, cam in enumerate([front, side, front, away, front, side]):   # three frames on each side of the restarts
        assert same(render_into_poison(r, cam), expected(pkg, KEY, cam)), f"frame {i}"
    r.cleanup_update()


# ---- 4. a restart inside a captured graph ----------------------------------------------------------------------------------------
def test_tag_restart_inside_a_captured_graph(pkg, monkeypatch):
    """The uncaptured first frame and captured frames 0 and 1 take the last three tags; captured frame 2 restarts the tag, so its
    clearing memset is a node of the graph."""
    monkeypatch.delenv("MI355RT_LEAN", raising=False)
    start, o5, o6, away, front, side = scene_case(pkg, KEY)[1]
    cams = [front, o5, away, side]
    monkeypatch.setenv("MI355RT_DEBUG_TAG0", hex(TAG_LIMIT - 3))
    c = Replayed(pkg, KEY, start)
    monkeypatch.delenv("MI355RT_DEBUG_TAG0")
    try:
        g, bufs = c.capture(cams)
        for rep in range(3):
            c.replay_and_check(g, cams, bufs, f"replay {rep}")
        c.update_and_check(o6, "the frame after the replays")
    finally:
        c.close()


# ---- 5. the lean schedule across the tag restart ---------------------------------------------------------------------------------
def test_lean_schedule_across_the_tag_restart(pkg, monkeypatch):
    monkeypatch.setenv("MI355RT_LEAN", "always")
    r = late_renderer(pkg, monkeypatch, tag0=TAG_LIMIT - 3)
    for i, cam in enumerate(cut_frames(pkg)):
        assert same(render_into_poison(r, cam), expected(pkg, KEY, cam)), f"frame {i}"
    r.cleanup_update()
