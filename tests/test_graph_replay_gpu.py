"""Replaying captured frames: the frame-to-frame state of a context (tile words tagged per frame, the three launch-order
generations, the "entered by" words of split tiles, the host-mapped census) must change the time, never the image -- also when a
captured graph is launched again and again, so that frame tags and generations repeat, generations are appended to without having
been cleared, and the split-tile election finds its own frame number already stored.

Every expected frame comes from a context that carries no frame state at all (RT_FLAG_STATIC_ORDER | RT_FLAG_NOSCAN |
RT_FLAG_NOSPLIT | RT_FLAG_NOLEAN, rendered uncaptured); for one pose per scene that frame is itself held to the CPU oracle.  All
scenes are of degree <= 2 and every comparison is bit for bit: there is no tolerance in this file.  Before every replay every
buffer is filled with a poison pattern, so that a tile nobody wrote shows."""
import functools

import numpy as np
import pytest

from conftest import scene_path
from test_gpu_parity import _orbit_pose, camera_cut_sequence, mixed_scene, oracle_from, random_walk, render_cpu

pytestmark = pytest.mark.gpu

RT_ERR_INVALID = -1
SCENES = ["20spheres", "walk2", "walk3", "mixed3", "mixed8", "reflection"]
COUNTER_KEYS = ("primary_rays", "shadow_rays", "reflect_rays", "tests", "hits")


def stateless_flags(pkg):
    return pkg.RT_FLAG_STATIC_ORDER | pkg.RT_FLAG_NOSCAN | pkg.RT_FLAG_NOSPLIT | pkg.RT_FLAG_NOLEAN


def cam_looks_away(cam):
    """random_walk's empty frames: yaw -90, the camera's z axis is the world's -z (the spheres lie at z >= 10)."""
    return cam[10] < 0.0


@functools.lru_cache(maxsize=None)
def scene_case(pkg, key):
    """(scene, cameras, oracle scene factory): the cameras are distinct, cameras[0] is the pose held to the oracle."""
    if key == "20spheres":
        sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(640, 360)
        away, front, side = camera_cut_sequence(pkg)[2]
        cams = [pkg.IDENTITY.copy(), _orbit_pose(pkg, 5), _orbit_pose(pkg, 6), away, front, side]
        return sc, cams, lambda oracle: oracle.load_scene(scene_path("20spheres")).with_size(640, 360)
    if key.startswith("walk"):   # few tiles with hits: the lists stay in use; mirrors on the odd seed
        sc, walk = random_walk(pkg, int(key[4:]))
        a = sc.arrays()
        sc.set_size(min(a["width"], 320), min(a["height"], 200))
        cams, seen = [], set()
        for cam in walk:
            if cam.tobytes() not in seen:
                seen.add(cam.tobytes())
                cams.append(cam)
        while cam_looks_away(cams[0]):   # (start with a view of the scene; the views that look away stay in the sequence)
            cams = cams[1:] + cams[:1]
        return sc, cams, lambda oracle: oracle_from(pkg, oracle, sc)
    if key.startswith("mixed"):  # general quadrics: launch-order lists, no tile words
        sc = mixed_scene(pkg, int(key[5:]))
        cams = [pkg.camera_matrix(pos=(0.3 * k - 0.6, 0.2 * (k % 3), -1.0 * k), yaw_deg=90.0 + 2.0 * k - 3.0, pitch_deg=k - 2.0) for k in range(5)]
        return sc, cams, lambda oracle: oracle_from(pkg, oracle, sc)
    assert key == "reflection"
    sc = pkg.Scene.load_from_file(scene_path("reflection_test")).set_size(256, 160).set_max_reflections(4)
    cams = [pkg.IDENTITY.copy()] + [pkg.camera_matrix(pos=(0.4 * k - 0.5, 0.3 * k, -0.6 * k), yaw_deg=90.0 + 4.0 * k, pitch_deg=2.0 * k - 3.0) for k in range(1, 5)]
    return sc, cams, lambda oracle: oracle.load_scene(scene_path("reflection_test")).with_size(256, 160, 4)


@functools.lru_cache(maxsize=None)
def stateless_renderer(pkg, key, fmt, fast):
    return pkg.Renderer(scene_case(pkg, key)[0], device=0, flags=stateless_flags(pkg) | (pkg.RT_FLAG_FAST if fast else 0), fmt=fmt)


@functools.lru_cache(maxsize=None)
def _expected(pkg, key, fmt, fast, cam_bytes):
    r = stateless_renderer(pkg, key, fmt, fast)
    r.update(np.frombuffer(cam_bytes, dtype=np.float64))
    out = r.download().copy()
    out.setflags(write=False)
    return out


def expected(pkg, key, cam, fmt=0, fast=False):
    """The whole frame of `key` under `cam` as a context without frame state renders it; computed once, never changed."""
    return _expected(pkg, key, fmt, fast, np.ascontiguousarray(cam, dtype=np.float64).tobytes())


def same(a, b):
    """Bit for bit (NaN poison included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def new_buffer(r, rows=None):
    import torch
    rows = r.local_rows if rows is None else rows
    return torch.empty((rows, r.width, 4), dtype=torch.uint8 if r.fmt else torch.float32, device="cuda:0")


def poison(bufs):
    """NaN bits into RGBA32F buffers, 0xA5 bytes into everything else; on the current stream."""
    import torch
    for b in bufs:
        if b.dtype == torch.float32:
            b.view(torch.int32).fill_(0x7FC00000)
        else:
            b.fill_(0xA5)


class Replayed:
    """A context on a stream of its own: one uncaptured frame, then graphs of captured frames, every frame into a buffer of its own."""

    def __init__(self, pkg, key, first_cam, fmt=0, fast=False, rows=None, **kw):
        import torch
        self.pkg, self.key, self.fmt, self.fast, self.rows = pkg, key, fmt, fast, rows
        self.r = pkg.Renderer(scene_case(pkg, key)[0], device=0, fmt=fmt, **kw)
        self.s = torch.cuda.Stream()
        self.r.update(first_cam, stream=self.s.cuda_stream, timed=False)   # (first call on this stream before the capture)
        torch.cuda.synchronize()
        self.graphs = []

    def want(self, cam):
        full = expected(self.pkg, self.key, cam, self.fmt, self.fast)
        return full if self.rows is None else full[self.rows]

    def capture(self, cams):
        import torch
        bufs = [new_buffer(self.r) for _ in cams]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self.s):
            for cam, buf in zip(cams, bufs):
                self.r.update(cam, dev_fb=buf.data_ptr(), stream=self.s.cuda_stream, timed=False)
        self.graphs.append(g)
        return g, bufs

    def replay_and_check(self, g, cams, bufs, what):
        import torch
        with torch.cuda.stream(self.s):
            poison(bufs)
            g.replay()
        self.s.synchronize()
        for k, (cam, buf) in enumerate(zip(cams, bufs)):
            assert same(buf.cpu().numpy(), self.want(cam)), f"{what}, captured frame {k}"

    def update_and_check(self, cam, what):
        """One uncaptured frame on the context's stream, into a poisoned buffer."""
        import torch
        buf = new_buffer(self.r)
        with torch.cuda.stream(self.s):
            poison([buf])
            self.r.update(cam, dev_fb=buf.data_ptr(), stream=self.s.cuda_stream, timed=False)
        self.s.synchronize()
        assert same(buf.cpu().numpy(), self.want(cam)), what

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.graphs.clear()
        self.r.cleanup_update()


def graph_cameras(pkg, key, k):
    """k distinct cameras for one graph.  20spheres: K = 3 is the cut empty view -> full view -> partial view, K = 7 starts with it."""
    cams = scene_case(pkg, key)[1]
    if key == "20spheres":
        start, o5, o6, away, front, side = cams
        return {1: [start], 2: [o5, o6], 3: [away, front, side], 4: [start, o5, away, o6], 7: [away, front, side, start, o5, o6, pkg.camera_matrix((1.0, 0.5, -2.0), 80.0, 4.0)]}[k]
    assert len(cams) >= k, (key, len(cams))
    return cams[:k]


# ---- the expected frames themselves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SCENES)
def test_stateless_frame_equals_the_oracle(pkg, oracle, key):
    sc, cams, osc = scene_case(pkg, key)
    got = expected(pkg, key, cams[0])
    assert np.all(got[..., 3] == 1.0)
    assert np.array_equal(got[..., :3], osc(oracle).render(cam=cams[0], nthreads=8))
    assert np.any(got[..., :3] != np.asarray(sc.arrays()["bg_color"], dtype=np.float32)), "the pose sees nothing of the scene"
    if key == "20spheres":   # the cut really goes through an empty view, a full one and a partial one
        away, front, side = cams[3:6]
        bg = expected(pkg, key, away)[0, 0]
        hit = [np.any(expected(pkg, key, c) != bg, axis=-1).mean() for c in (away, front, side)]
        assert hit[0] == 0.0 and hit[1] > 0.0 and 0.0 < hit[2] != hit[1], hit


# ---- 1. K frames, R replays ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,k", [("20spheres", k) for k in (1, 2, 3, 4, 7)] + [(key, k) for key in SCENES[1:] for k in (1, 4)])
def test_k_frames_replayed_four_times(pkg, key, k):
    cams = graph_cameras(pkg, key, k)
    c = Replayed(pkg, key, scene_case(pkg, key)[1][0])
    try:
        g, bufs = c.capture(cams)
        for rep in range(4):
            c.replay_and_check(g, cams, bufs, f"{key} K={k} replay {rep}")
    finally:
        c.close()


# ---- 2. uncaptured frames between and after the replays --------------------------------------------------------------------------
@pytest.mark.parametrize("key,k", [("20spheres", 1), ("20spheres", 3), ("walk3", 2), ("mixed3", 2), ("reflection", 1)])
def test_uncaptured_frames_between_replays(pkg, key, k):
    all_cams = scene_case(pkg, key)[1]
    cams = graph_cameras(pkg, key, k)
    others = [cam for cam in all_cams if not any(cam.tobytes() == g.tobytes() for g in cams)]   # cameras that are not in the graph
    assert others
    c = Replayed(pkg, key, all_cams[0])
    try:
        g, bufs = c.capture(cams)
        c.replay_and_check(g, cams, bufs, "replay 0")
        c.update_and_check(others[0], "the frame after replay 0")
        c.replay_and_check(g, cams, bufs, "replay 1")
        c.update_and_check(others[-1], "first frame after replay 1")
        c.update_and_check(others[0], "second frame after replay 1")
        c.replay_and_check(g, cams, bufs, "replay 2")
        c.update_and_check(cams[0], "the frame after replay 2")
    finally:
        c.close()


# ---- 3. two graphs from one context ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["20spheres", "walk2", "mixed8"])
def test_two_graphs_of_one_context(pkg, key):
    all_cams = scene_case(pkg, key)[1]
    a, b = ([all_cams[1]], [all_cams[0]]) if key == "20spheres" else ([all_cams[0]], [all_cams[1]])
    c = Replayed(pkg, key, all_cams[0])
    try:
        g1, bufs1 = c.capture(a)
        g2, bufs2 = c.capture(b)
        for n, which in enumerate((1, 2, 1, 1, 2)):
            if which == 1:
                c.replay_and_check(g1, a, bufs1, f"launch {n} (g1)")
            else:
                c.replay_and_check(g2, b, bufs2, f"launch {n} (g2)")
    finally:
        c.close()


# ---- 4. what the frame after the replays reads -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_counters(oracle, name, w, h, depth, cam_bytes=None):
    cam = None if cam_bytes is None else np.frombuffer(cam_bytes, dtype=np.float64)
    return render_cpu(oracle, name, w, h, depth, cam=cam, counters=True)[1]


@pytest.mark.parametrize("name,depth,schedule", [("20spheres", None, "general"), ("20spheres", None, "lean"), ("reflection_test", 4, None), ("clebsch", None, None)])
def test_counters_of_the_frame_after_four_replays(pkg, oracle, monkeypatch, name, depth, schedule):
    """The keys and scenes of test_gpu_parity.test_counters_match_oracle.  The generation the frame reads was appended to four times
    without having been cleared: no tile may be counted twice.  20spheres is the one scene the lean instantiation renders; it
    executes fewer unit-sphere tests than the general one (test_counters_fuzz_gpu.py) and a context chooses between them from the
    frames before, so both contexts are held to one schedule, each in turn."""
    import torch
    monkeypatch.delenv("MI355RT_LEAN", raising=False)
    if schedule == "lean":
        monkeypatch.setenv("MI355RT_LEAN", "always")
    extra = pkg.RT_FLAG_NOLEAN if schedule == "general" else 0
    w, h = 480, 270
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
    if depth is not None:
        sc.set_max_reflections(depth)
    ocnt = oracle_counters(oracle, name, w, h, depth)
    fresh = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_COUNT | extra)
    fresh.update()
    first = fresh.counters_detail()
    fresh.cleanup_update()
    r = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_COUNT | extra)
    s = torch.cuda.Stream()
    r.update(stream=s.cuda_stream, timed=False)
    torch.cuda.synchronize()
    buf = new_buffer(r)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r.update(dev_fb=buf.data_ptr(), stream=s.cuda_stream, timed=False)
    with torch.cuda.stream(s):
        for rep in range(4):
            g.replay()
    s.synchronize()
    r.update(stream=s.cuda_stream, timed=False)
    s.synchronize()
    d = r.counters_detail()
    del g
    r.cleanup_update()
    print(name, {k: (d[k], ocnt.get(k)) for k in COUNTER_KEYS})
    for k in ("primary_rays", "shadow_rays", "reflect_rays"):
        assert d[k] == ocnt[k], (name, k, d[k], ocnt[k])
    if name != "clebsch":
        assert d["tests"] == ocnt["tests"], (name, d["tests"], ocnt["tests"])
        assert d["hits"] == ocnt["normals"], (name, d["hits"], ocnt["normals"])
    # ... and the detail counters that do not describe the schedule equal a fresh counting context's first frame
    for k in ("executed_by_class", "solves_by_class", "hit_lights_shaded", "shadow_rays_traced"):
        assert d[k] == first[k], (name, k, d[k], first[k])


def read_message(msg, cap):
    """(count, overflow, ids) of one sparse message (device tensor of bytes)."""
    words = msg.cpu().numpy().view(np.uint32)
    n = int(words[0])
    return n, int(words[1]), words[4:4 + min(n, cap)].copy()


@pytest.mark.parametrize("fmt", [0, 1], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("key", ["20spheres", "walk3", "mixed3"])
def test_sparse_message_of_the_frame_after_four_replays(pkg, key, fmt):
    import torch
    cam = scene_case(pkg, key)[1][0]
    c = Replayed(pkg, key, cam, fmt=fmt)
    try:
        r = c.r
        cap = ((r.width + 15) // 16) * ((r.local_rows + 15) // 16)
        g, bufs = c.capture([cam])
        for rep in range(4):
            c.replay_and_check(g, [cam], bufs, f"replay {rep}")
        msg = torch.empty((r.sparse_msg_bytes(cap),), dtype=torch.uint8, device="cuda:0")
        full = new_buffer(r, r.height)
        with torch.cuda.stream(c.s):
            poison([msg, full])
            r.update_sparse(msg.data_ptr(), cap, cam, stream=c.s.cuda_stream, timed=False)
            r.assemble_sparse(msg.data_ptr(), cap, full.data_ptr(), stream=c.s.cuda_stream)
        c.s.synchronize()
        n, overflow, ids = read_message(msg, cap)
        assert overflow == 0 and n <= cap, (n, overflow, cap)
        assert len(set(ids.tolist())) == n, f"{n - len(set(ids.tolist()))} tiles are in the message twice"
        # the same tiles as rt_render + rt_pack_sparse of a fresh context
        fresh = pkg.Renderer(scene_case(pkg, key)[0], device=0, fmt=fmt)
        fresh.update(cam)
        msg2 = torch.empty_like(msg)
        poison([msg2])
        fresh.pack_sparse(msg2.data_ptr(), cap)
        torch.cuda.synchronize()
        n2, overflow2, ids2 = read_message(msg2, cap)
        fresh.cleanup_update()
        assert overflow2 == 0 and sorted(ids.tolist()) == sorted(ids2.tolist())
        assert n > 0
        assert same(full.cpu().numpy(), c.want(cam))
    finally:
        c.close()


# ---- 5. schedules and flags ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["lean_always", "nolean", "noscan", "plain_order", "rgba8", "fast", "rank1of3"])
def test_three_frames_three_replays_in_every_schedule(pkg, monkeypatch, variant):
    key = "20spheres"
    cams = graph_cameras(pkg, key, 3)
    kw, fmt, fast, rows = {}, 0, False, None
    if variant == "lean_always":
        monkeypatch.setenv("MI355RT_LEAN", "always")
    else:
        monkeypatch.delenv("MI355RT_LEAN", raising=False)
    if variant == "nolean":
        kw["flags"] = pkg.RT_FLAG_NOLEAN
    elif variant == "noscan":
        kw["flags"] = pkg.RT_FLAG_NOSCAN
    elif variant == "plain_order":
        kw["flags"] = pkg.RT_FLAG_PLAIN_ORDER
    elif variant == "rgba8":
        fmt = pkg.RT_FMT_RGBA8
    elif variant == "fast":
        kw["flags"], fast = pkg.RT_FLAG_FAST, True   # (expected frames: a stateless RT_FLAG_FAST context)
    elif variant == "rank1of3":
        kw.update(rank=1, world=3, band_rows=5)
        rows = pkg.band_rows_of_rank(360, 5, 3, 1)
    c = Replayed(pkg, key, scene_case(pkg, key)[1][0], fmt=fmt, fast=fast, rows=rows, **kw)
    try:
        if rows is not None:
            assert np.array_equal(c.r.row_map(), rows)
        g, bufs = c.capture(cams)
        for rep in range(3):
            c.replay_and_check(g, cams, bufs, f"{variant} replay {rep}")
    finally:
        c.close()


# ---- 6. captured rt_render_sparse ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [0, 1], ids=["rgba32f", "rgba8"])
def test_captured_sparse_frames_replayed(pkg, fmt):
    import torch
    key = "20spheres"
    cams = graph_cameras(pkg, key, 2)
    c = Replayed(pkg, key, scene_case(pkg, key)[1][0], fmt=fmt)
    try:
        r = c.r
        cap = ((r.width + 15) // 16) * ((r.local_rows + 15) // 16)
        msgs = [torch.empty((r.sparse_msg_bytes(cap),), dtype=torch.uint8, device="cuda:0") for _ in cams]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=c.s):
            for cam, msg in zip(cams, msgs):
                r.update_sparse(msg.data_ptr(), cap, cam, stream=c.s.cuda_stream, timed=False)
        c.graphs.append(g)
        full = new_buffer(r, r.height)
        for rep in range(3):
            with torch.cuda.stream(c.s):
                poison(msgs)
                g.replay()
            c.s.synchronize()
            for k, (cam, msg) in enumerate(zip(cams, msgs)):
                n, overflow, ids = read_message(msg, cap)
                assert overflow == 0 and 0 < n <= cap, (rep, k, n, overflow)
                with torch.cuda.stream(c.s):
                    poison([full])
                    r.assemble_sparse(msg.data_ptr(), cap, full.data_ptr(), stream=c.s.cuda_stream)
                c.s.synchronize()
                assert same(full.cpu().numpy(), c.want(cam)), f"replay {rep}, captured frame {k}"
    finally:
        c.close()


# ---- 7. the documented refusal still holds after replays -------------------------------------------------------------------------
def test_other_stream_is_still_refused_after_replays(pkg):
    import torch
    key = "20spheres"
    cams = graph_cameras(pkg, key, 2)
    c = Replayed(pkg, key, scene_case(pkg, key)[1][0])
    try:
        g, bufs = c.capture(cams)
        for rep in range(2):
            c.replay_and_check(g, cams, bufs, f"replay {rep}")
        other = torch.cuda.Stream()
        for stream in (other.cuda_stream, None):
            with pytest.raises(pkg.RtError) as e:
                c.r.update(cams[0], stream=stream, timed=False)
            assert e.value.code == RT_ERR_INVALID and "captured" in e.value.message
        c.replay_and_check(g, cams, bufs, "replay after the refusals")   # the refused calls changed nothing
    finally:
        c.close()
