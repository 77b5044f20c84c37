"""The multi-GPU layer beyond frames, on the GPU (csrc/rt_multi.cpp, csrc/rt_planes.hip): rt_set_scene_multi and its
status, the query context, rt_render_gbuffer_multi, rt_object_extents_multi, the two rank-level helpers underneath them
(rt_assemble_planes, rt_merge_object_extents) and the update.h adapter with several devices.

Everything is bit for bit; there is no tolerance in this file.  The reference of a multi-GPU answer is the single context's answer on the
same scene (strict contexts, surfaces of degree <= 2) and, where the arithmetic is the device's own (degree 3, RT_FLAG_FAST), the
rank-level contexts' answers placed by rt_row_map / merged by tests/tools/extents_ref.  The helpers alone are compared with their numpy
restatements (tests/test_multi_queries_host.py).  Frames are at most 129 x 31 or 96 x 72 pixels; the one-GPU box rehearses every layout
with one device repeated."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import extents_ref  # noqa: E402
from test_multi_queries_host import assemble_planes_ref, merge_ref  # noqa: E402
from test_set_scene_gpu import KEYS, base_scene, changed, desc, fresh_frame, oracle_scene, same, sphere, update_of  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 96, 72
MOVED = ((0.4, 0.3, -1.5), 84.0, -3.0)   # the moved camera of tests/test_gbuffer_gpu.py
SELF, BANDWISE, SPARSE = 0x10000, 0x20000, 0x40000
# devices, parts per device, band rows, flags, frame size; "ten" has ten contexts for eight bands: the last band is short (3 rows), two
# contexts own no row, and the width is odd
LAYOUTS = {
    "3x1": dict(devices=[0, 0, 0], parts=1, band_rows=8, flags=0, size=(W, H)),
    "2x2": dict(devices=[0, 0], parts=2, band_rows=16, flags=0, size=(W, H)),
    "1x3": dict(devices=[0], parts=3, band_rows=16, flags=0, size=(W, H)),
    "self": dict(devices=[0], parts=1, band_rows=16, flags=SELF, size=(W, H)),
    "ten": dict(devices=[0, 0], parts=5, band_rows=4, flags=0, size=(129, 31)),
}
NAMES = list(LAYOUTS)


def multi(pkg, scene, layout, flags=0):
    L = LAYOUTS[layout]
    return pkg.MultiRenderer(scene, L["devices"], band_rows=L["band_rows"], parts=L["parts"], flags=L["flags"] | flags)


def world_of(layout):
    return len(LAYOUTS[layout]["devices"]) * LAYOUTS[layout]["parts"]


def sized(a, layout):
    w, h = LAYOUTS[layout]["size"]
    return changed(a, width=w, height=h)


def frame(m, cam=None):
    m.update(cam)
    return m.download().copy()


_fresh = {}


def fresh(pkg, a, cam=None):
    """The frame of a fresh single context on the scene dictionary `a`, computed once per scene."""
    key = (a["width"], a["height"], tuple(a[k].tobytes() for k in KEYS), None if cam is None else np.asarray(cam).tobytes())
    if key not in _fresh:
        _fresh[key] = fresh_frame(pkg, a, pkg.IDENTITY if cam is None else cam)
    return _fresh[key]


def tiny_scene(pkg, w, h, n=1):
    sc = pkg.Scene.new(w, h, 50.0, 1, (0.1, 0.2, 0.3))
    for i in range(n):
        sc.add_object(pkg.surface_make("sphere", (0.3 * i, 0.0, 6.0 + i), [1.0]), (0.8, 0.5, 0.2))
    sc.add_light("directional", [0.2, -1.0, 0.4])
    return sc


# ---- 1. the helpers alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_assemble_planes_on_random_bytes(pkg, world):
    """Every elem_bytes x height x band x width for this world: a slot stride larger than a slot (three elements more), a sentinel behind
    `full`.  Rank 0 does the reassembly, as on the root."""
    import torch
    rng = np.random.default_rng(100 + world)
    for height in (1, 7, 31, 37):
        for width in (1, 3, 129):
            sc = tiny_scene(pkg, width, height)
            for band in (1, 4, 5, 8):
                r = pkg.Renderer(sc, device=0, rank=0, world=world, band_rows=band)
                assert r.max_local_rows == pkg.max_local_rows(height, band, world)
                for elem in (4, 8, 16):
                    slot_elems = r.max_local_rows * width + 3
                    host = rng.integers(0, 256, (world * slot_elems, elem), dtype=np.uint8)
                    g = torch.from_numpy(host).to("cuda:0")
                    full = torch.full((height * width * elem + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
                    r.assemble_planes(g.data_ptr(), slot_elems * elem, full.data_ptr(), elem)
                    torch.cuda.synchronize()
                    got = full.cpu().numpy()
                    want = assemble_planes_ref(pkg, host, slot_elems, width, height, band, world)
                    assert np.array_equal(got[:-64].reshape(height, width, elem), want), (world, height, width, band, elem)
                    assert np.all(got[-64:] == 0xA5), (world, height, width, band, elem)
                r.cleanup_update()


def random_records(rng, n_parts, n_obj, identity_share):
    parts = np.zeros((n_parts, n_obj), dtype=extents_ref.DTYPE)
    parts["pixels"] = rng.integers(1, 1 << 40, (n_parts, n_obj))
    for f in ("x_min", "y_min", "x_max", "y_max"):
        parts[f] = rng.integers(0, 1 << 32, (n_parts, n_obj), dtype=np.uint64).astype(np.uint32)
    parts["t_min"] = 10.0 ** rng.uniform(-7, 6, (n_parts, n_obj))
    parts["t_max"] = 10.0 ** rng.uniform(-7, 6, (n_parts, n_obj))
    blank = rng.random((n_parts, n_obj)) < identity_share
    parts[blank] = extents_ref.identity(1)[0]
    return parts


@pytest.mark.parametrize("n_obj", [1, 20, 300])   # 300: more than one workgroup of 256 lanes
def test_merge_object_extents_on_random_records(pkg, n_obj):
    import torch
    rng = np.random.default_rng(n_obj)
    r = pkg.Renderer(tiny_scene(pkg, 32, 24, n_obj), device=0)
    for n_parts, share in ((1, 0.3), (2, 0.5), (7, 0.6), (3, 1.0)):   # (share 1.0: all identities in, identities out, bit for bit)
        parts = random_records(rng, n_parts, n_obj, share)
        d = torch.from_numpy(parts.view(np.uint8).reshape(-1)).to("cuda:0")
        out = torch.full((n_obj * 40 + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
        r.merge_object_extents(d.data_ptr(), n_parts, out.data_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        want = merge_ref(parts)
        assert got[:-64].tobytes() == want.tobytes(), (n_obj, n_parts)
        assert np.all(got[-64:] == 0xA5)
        if share == 1.0:
            assert got[:-64].tobytes() == extents_ref.identity(n_obj).tobytes()
    r.cleanup_update()


def test_helper_refusals(pkg):
    import torch
    sc = tiny_scene(pkg, 33, 21, 4)
    r = pkg.Renderer(sc, device=0, rank=0, world=2, band_rows=4)   # bands 0..5, rank 0 owns 0, 2, 4: 12 rows
    slot8 = r.max_local_rows * 33 * 8
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    g, full = buf.data_ptr(), buf.data_ptr() + (1 << 15)

    def refused(fn, *args, text):
        with pytest.raises(pkg.RtError) as e:
            fn(*args)
        assert e.value.code == -1 and text in e.value.message, e.value.message

    refused(r.assemble_planes, None, slot8, full, 8, text="rt_assemble_planes: null argument")
    refused(r.assemble_planes, g, slot8, None, 8, text="rt_assemble_planes: null argument")
    for elem in (0, 1, 2, 3, 12, 32):
        refused(r.assemble_planes, g, slot8, full, elem, text="elem_bytes")
    refused(r.assemble_planes, g, slot8 - 8, full, 8, text="slot stride")        # smaller than one slot
    refused(r.assemble_planes, g, slot8 + 4, full, 8, text="slot stride")        # not a multiple of elem_bytes
    refused(r.assemble_planes, g + 4, slot8, full, 8, text="aligned")
    refused(r.assemble_planes, g, slot8 * 2, full + 8, 16, text="aligned")
    refused(r.assemble_planes, g, slot8, g + slot8, 8, text="overlaps")           # full starts inside rank 1's slot
    refused(r.assemble_planes, g + 21 * 33 * 8 - 8, slot8, g, 8, text="overlaps")  # gathered starts inside full's last element
    r.assemble_planes(g, slot8, g + 2 * slot8, 8)                                # adjacent is not overlapping
    refused(r.merge_object_extents, None, 1, full, text="rt_merge_object_extents: null argument")
    refused(r.merge_object_extents, g, 1, None, text="rt_merge_object_extents: null argument")
    refused(r.merge_object_extents, g, 0, full, text="n_parts is 0")
    refused(r.merge_object_extents, g + 4, 1, full, text="8-byte aligned")
    refused(r.merge_object_extents, g, 1, full + 4, text="8-byte aligned")
    refused(r.merge_object_extents, g, 3, g + 2 * 4 * 40, text="overlaps")
    r.merge_object_extents(g, 3, g + 3 * 4 * 40)
    r.cleanup_update()
    ss = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_SSAA2)
    refused(ss.assemble_planes, g, 21 * 33 * 8, full, 8, text="rt_assemble_planes: not available for contexts created with RT_FLAG_SSAA2")
    ss.cleanup_update()
    # a scene without objects: RT_OK, nothing enqueued, nothing written
    empty = pkg.Scene.new(40, 30, 50.0, 2, (0.3, 0.6, 0.9))
    empty.add_light("directional", [0, -1, 0])
    e = pkg.Renderer(empty, device=0)
    out = torch.full((256,), 0x5A, dtype=torch.uint8, device="cuda:0")
    e.merge_object_extents(g, 4, out.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    e.cleanup_update()


# ---- 2. scene updates --------------------------------------------------------------------------------------------------------------------
def scene_steps(pkg, s0, s1, layout_flags=0, layout="2x2", reject=None):
    """S0 -> S1 -> S1 with other light colours -> (a rejected update) -> two updates back to back with a frame behind each."""
    import torch
    s2 = changed(s1, light_color=(s1["light_color"] * np.float32(0.5) + np.float32(0.125)).astype(np.float32))
    m = multi(pkg, desc(pkg, s0), layout, layout_flags)
    try:
        assert same(frame(m), fresh(pkg, s0))
        m.set_scene(**{k: s1[k] for k in KEYS})
        got = frame(m)
        assert same(got, fresh(pkg, s1)) and not same(got, fresh(pkg, s0))
        assert m.set_scene_status() == dict(applied=1, rejected=0, reason=0, index=0)
        m.set_scene(light_color=s2["light_color"])                      # a partial update: the other four arrays stay
        got = frame(m)
        assert same(got, fresh(pkg, s2)) and not same(got, fresh(pkg, s1))
        assert m.set_scene_status() == dict(applied=2, rejected=0, reason=0, index=0)
        if reject is not None:
            bad, reason, index = reject
            m.set_scene(**{k: bad[k] for k in KEYS})                    # enqueue-only: the verdict is on the devices
            assert m.set_scene_status() == dict(applied=2, rejected=1, reason=reason, index=index)
            assert same(frame(m), fresh(pkg, s2))
        # ordering: two updates with no wait in between, an enqueue-only frame behind each, into a buffer of its own
        w, h = s0["width"], s0["height"]
        b1 = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
        b2 = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        m.set_scene(**{k: s1[k] for k in KEYS})
        m.update(None, full_ptr=b1.data_ptr(), timed=False)
        m.set_scene(**{k: s2[k] for k in KEYS})
        m.update(None, full_ptr=b2.data_ptr(), timed=False)
        m.wait()
        assert same(b1.cpu().numpy(), fresh(pkg, s1)), "buffer 1 shows scene 1"
        assert same(b2.cpu().numpy(), fresh(pkg, s2)), "buffer 2 shows scene 2"
        assert m.set_scene_status()["applied"] == 4
    finally:
        m.cleanup_update()


@pytest.mark.parametrize("layout", NAMES)
def test_scene_updates(pkg, layout):
    s0, s1 = sized(base_scene(pkg, "mixed"), layout), sized(update_of(pkg, "mixed", "moved"), layout)
    bad = changed(s1)
    bad["coefs"] = bad["coefs"].copy()
    bad["coefs"][3][10] = 2.0                                            # a sphere turned into an ellipsoid
    scene_steps(pkg, s0, s1, layout=layout, reject=(bad, pkg.RT_SCENE_REJECT_CLASS, 3))


@pytest.mark.parametrize("flag", [BANDWISE, SPARSE])
def test_scene_updates_under_the_other_transports(pkg, flag):
    scene_steps(pkg, base_scene(pkg, "20spheres"), update_of(pkg, "20spheres", "moved"), layout_flags=flag)


def moved_shipped(pkg, name):
    """A shipped scene and a class-preserving change of it: spheres translated, albedos permuted, lights turned and dimmed; reflection
    ratios stay (a mirror must stay a mirror)."""
    a = pkg.Scene.load_from_file(scene_path(name)).set_size(W, H).arrays()
    b = changed(a)
    for i, q in enumerate(b["coefs"]):
        if np.all(q[:10] == 0) and np.all(q[10:13] == 1) and np.all(q[13:16] == 0):
            c = -0.5 * q[16:19]
            b["coefs"][i] = sphere(c + np.array([0.3, -0.2, 0.5]), float(np.sqrt(np.dot(c, c) - q[19])))
    b["albedo"] = np.ascontiguousarray(b["albedo"][:, ::-1])
    b["light_p"] = b["light_p"] + np.array([0.1, -0.05, 0.2])
    b["light_color"] = (b["light_color"] * np.float32(0.75)).astype(np.float32)
    return a, b


@pytest.mark.parametrize("name", ["reflection_test", "quadratic"])
def test_scene_updates_of_shipped_scenes(pkg, name):
    a, b = moved_shipped(pkg, name)
    if name == "reflection_test":
        assert (a["reflection"] > 1e-7).any() and np.array_equal(a["reflection"], b["reflection"])
    scene_steps(pkg, a, b)


# ---- 3. queries after an update ------------------------------------------------------------------------------------------------------------
def test_queries_after_an_update_equal_the_single_renderer(pkg):
    s0, s1 = base_scene(pkg, "mixed"), update_of(pkg, "mixed", "moved")
    cam = pkg.camera_matrix(*MOVED)
    rng = np.random.default_rng(3)
    xy = np.stack([rng.integers(0, W, 40), rng.integers(0, H, 40)], axis=1)
    o = rng.uniform([-2, -2, -2], [2, 2, 2], (300, 3))
    d = rng.normal(size=(300, 3)) + np.array([0, 0, 2.0])

    def answers(r):
        blocked, _ = r.occluded(o, d)
        seg, ends = r.pick_paths(xy, cam)
        pseg, plast, pends = r.paths(o, d)
        return [r.pick(xy, cam), seg, ends, r.trace(o, d), blocked.cpu().numpy(), r.shade(o, d), pseg, plast, pends]

    m, f = multi(pkg, desc(pkg, s0), "2x2"), pkg.Renderer(desc(pkg, s1), device=0)
    try:
        stale = answers(m)
        m.set_scene(**{k: s1[k] for k in KEYS})      # enqueue-only: the queries run behind it on the root's stream
        got, want = answers(m), answers(f)
        for i, (g, w_) in enumerate(zip(got, want)):
            assert same(g, w_), i
        assert not all(same(g, s) for g, s in zip(got, stale))
        view = m.query
    finally:
        m.cleanup_update()
        f.cleanup_update()
    assert view._h is None   # the borrowed view died with the object, without destroying the context a second time


# ---- 4. G-buffer ---------------------------------------------------------------------------------------------------------------------------
_planes = {}


def single_planes(pkg, name, size, cam_key):
    key = (name, size, cam_key)
    if key not in _planes:
        sc = pkg.Scene.load_from_file(scene_path(name)).set_size(*size)
        r = pkg.Renderer(sc, device=0)
        o, t, n, _ = r.gbuffer(None if cam_key == "start" else pkg.camera_matrix(*MOVED))
        _planes[key] = (o.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy())
        r.cleanup_update()
    return _planes[key]


def numpy_planes(res):
    return tuple(None if p is None else p.cpu().numpy() for p in res[:3])


@pytest.mark.parametrize("layout", NAMES)
def test_gbuffer_equals_the_single_context(pkg, layout):
    size = LAYOUTS[layout]["size"]
    hits = 0
    for name in ("20spheres", "quadratic", "reflection_test"):
        sc = pkg.Scene.load_from_file(scene_path(name)).set_size(*size)
        m = multi(pkg, sc, layout)
        try:
            for cam_key in ("start", "moved"):
                cam = None if cam_key == "start" else pkg.camera_matrix(*MOVED)
                res = m.gbuffer(cam)
                m.wait()
                assert res[3] is not None and res[3] >= 0.0
                for g, w_ in zip(numpy_planes(res), single_planes(pkg, name, size, cam_key)):
                    assert same(g, w_), (layout, name, cam_key)
                hits += int((numpy_planes(res)[0] >= 0).sum())
        finally:
            m.cleanup_update()
    assert hits > 0


@pytest.mark.parametrize("layout,name,flags", [("3x1", "clebsch", 0), ("ten", "clebsch", 0), ("2x2", "20spheres", 1), ("self", "quadratic", 1)])
def test_gbuffer_of_device_arithmetic_is_the_scatter_of_the_rank_level_planes(pkg, layout, name, flags):
    """Degree 3 and RT_FLAG_FAST (flags = 1): row y is the row rt_render_gbuffer writes on a context of that rank, world and band size."""
    L = LAYOUTS[layout]
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(*L["size"])
    w, h = L["size"]
    cam = pkg.camera_matrix((0.3, 0.2, -4.0), 90.0, 0.0) if name == "clebsch" else pkg.camera_matrix(*MOVED)
    want = [np.zeros((h, w), np.int32), np.zeros((h, w), np.float64), np.zeros((h, w, 4), np.float32)]
    world = world_of(layout)
    for q in range(world):
        r = pkg.Renderer(sc, device=0, rank=q, world=world, band_rows=L["band_rows"], flags=flags)
        if r.local_rows:
            rows = r.row_map()
            for k, p in enumerate(numpy_planes(r.gbuffer(cam))):
                want[k][rows] = p
        r.cleanup_update()
    m = multi(pkg, sc, layout, flags)
    try:
        got = numpy_planes(m.gbuffer(cam))
    finally:
        m.cleanup_update()
    for g, w_ in zip(got, want):
        assert same(g, w_), (layout, name)
    assert (got[0] >= 0).any()


@pytest.mark.parametrize("layout", ["2x2", "self", "ten"])
def test_gbuffer_subsets_sentinels_timing_and_frames(pkg, layout):
    import torch
    L = LAYOUTS[layout]
    w, h = L["size"]
    sc = pkg.Scene.load_from_file(scene_path("quadratic")).set_size(w, h)
    cam = pkg.camera_matrix(*MOVED)
    want = single_planes(pkg, "quadratic", (w, h), "moved")
    dts, shapes = (torch.int32, torch.float64, torch.float32), ((h, w), (h, w), (h, w, 4))
    guard = 32   # elements behind each plane
    m = multi(pkg, sc, layout)
    try:
        before = frame(m, cam)

        def run(ask, timed):
            bufs = []
            for dt, shape in zip(dts, shapes):
                n = int(np.prod(shape))
                b = torch.empty(n + guard, dtype=dt, device="cuda:0")
                b.view(torch.uint8).fill_(0xC3)   # every element prefilled with a sentinel no plane holds everywhere
                bufs.append(b)
            torch.cuda.synchronize()
            ms = m.gbuffer_into(cam, *[b.data_ptr() if a else None for b, a in zip(bufs, ask)], timed=timed)
            assert (ms is not None) == timed
            m.wait()
            out = []
            for b, a, shape, ref in zip(bufs, ask, shapes, want):
                host = b.cpu().numpy()
                n = int(np.prod(shape))
                assert np.all(host[n:].view(np.uint8) == 0xC3), "the guard behind a plane"
                if a:
                    assert same(host[:n].reshape(shape), ref)   # hence every element was written: the reference holds no sentinel plane
                else:
                    assert np.all(host.view(np.uint8) == 0xC3), "a plane that was not asked for"
                out.append(host[:n].copy())
            return out

        timed = run((True, True, True), True)
        plain = run((True, True, True), False)
        assert all(same(a, b) for a, b in zip(timed, plain))
        assert same(frame(m, cam), before), "a frame between two passes"
        for k in range(3):
            run(tuple(i == k for i in range(3)), False)
        assert same(frame(m, cam), before)
        with pytest.raises(pkg.RtError) as e:
            m.gbuffer_into(cam, None, None, None)
        assert e.value.code == -1 and "rt_render_gbuffer_multi: all three planes are null" in e.value.message
        run((True, False, True), False)   # ... and the refusal left the object usable
    finally:
        m.cleanup_update()


# ---- 5. extents ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", NAMES)
def test_object_extents_equal_the_single_context_and_the_merge_of_the_ranks(pkg, layout):
    import torch
    L = LAYOUTS[layout]
    w, h = L["size"]
    B, world = L["band_rows"], world_of(layout)
    cam = pkg.camera_matrix(*MOVED)
    # NULL; a rectangle across bands; one inside a single band (band 1: every other context contributes identities)
    rects = (None, (w // 8, 1, w - w // 8, h - 2), (3, B, w - 4, 2 * B - 1))
    for name in ("20spheres", "quadratic"):
        sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
        single = pkg.Renderer(sc, device=0)
        ranks = [pkg.Renderer(sc, device=0, rank=q, world=world, band_rows=B) for q in range(world)]
        m = multi(pkg, sc, layout)
        n = sc.desc().n_objects
        try:
            for rect in rects:
                got = m.object_extents(cam, rect)
                want = single.object_extents(cam, rect)
                assert got.tobytes() == want.tobytes(), (layout, name, rect)
                parts = np.stack([r.object_extents(cam, rect) for r in ranks])
                assert got.tobytes() == merge_ref(parts).tobytes(), (layout, name, rect)
                if rect is not None and rect[1] == B:
                    owner = 1 % world
                    assert all(parts[q].tobytes() == extents_ref.identity(n).tobytes() for q in range(world) if q != owner)
                # the device form, timed and enqueue-only, with a guard behind the records
                for timed in (True, False):
                    out = torch.full((n * 40 + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    ms = m.object_extents_into(cam, rect, out.data_ptr(), timed=timed)
                    assert (ms is not None) == timed
                    m.wait()
                    host = out.cpu().numpy()
                    assert host[:-64].tobytes() == want.tobytes() and np.all(host[-64:] == 0xA5)
            # objects nobody sees keep the exact identity record: some of them under a rectangle inside one band, all of them from a
            # camera that looks the other way
            band = m.object_extents(cam, rects[2])
            unseen = band["pixels"] == 0
            assert unseen.any() and (~unseen).any(), (layout, name)
            assert band[unseen].tobytes() == extents_ref.identity(int(unseen.sum())).tobytes()
            if name == "20spheres":   # (quadratic has unbounded surfaces: something is in view whichever way the camera looks)
                away = pkg.camera_matrix((0.0, 0.0, 0.0), -90.0, 0.0)
                assert int(single.object_extents(away)["pixels"].sum()) == 0
                assert m.object_extents(away).tobytes() == extents_ref.identity(n).tobytes()
        finally:
            m.cleanup_update()
            single.cleanup_update()
            for r in ranks:
                r.cleanup_update()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_supersampling_objects_refuse_with_the_contexts_message(pkg):
    sc = pkg.Scene.load_from_file(scene_path("quadratic")).set_size(64, 48)
    m = multi(pkg, sc, "2x2", pkg.RT_FLAG_SSAA2)
    try:
        with pytest.raises(pkg.RtError) as e:
            m.gbuffer()
        assert e.value.code == -1 and "rt_render_gbuffer: not available for contexts created with RT_FLAG_SSAA2" in e.value.message
        with pytest.raises(pkg.RtError) as e:
            m.object_extents()
        assert e.value.code == -1 and "rt_object_extents: not available for contexts created with RT_FLAG_SSAA2" in e.value.message
        single = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_SSAA2)
        single.update()
        want = single.download().copy()
        single.cleanup_update()
        assert same(frame(m), want)   # a refusal with nothing enqueued leaves the object usable
    finally:
        m.cleanup_update()


def test_a_failed_object_refuses_further_calls(pkg, monkeypatch):
    """MI355RT_DEBUG_MULTI_FAIL=1: rt_set_scene_multi fails on the host in front of context 1, with context 0 already enqueued -- the
    contexts hold different scenes from then on, and every later call says so."""
    s0, s1 = base_scene(pkg, "20spheres"), update_of(pkg, "20spheres", "moved")
    m = multi(pkg, desc(pkg, s0), "2x2")
    try:
        frame(m)
        monkeypatch.setenv("MI355RT_DEBUG_MULTI_FAIL", "1")
        with pytest.raises(pkg.RtError) as e:
            m.set_scene(**{k: s1[k] for k in KEYS})
        assert e.value.code == -3 and "MI355RT_DEBUG_MULTI_FAIL" in e.value.message
        monkeypatch.delenv("MI355RT_DEBUG_MULTI_FAIL")
        for call, who in ((lambda: m.set_scene(albedo=s1["albedo"]), "rt_set_scene_multi"), (m.set_scene_status, "rt_multi_set_scene_status"),
                          (m.gbuffer, "rt_render_gbuffer_multi"), (m.object_extents, "rt_object_extents_multi_host"),
                          (lambda: m.object_extents_into(None, None, 8, timed=False), "rt_object_extents_multi"), (m.update, "rt_render_multi")):
            with pytest.raises(pkg.RtError) as e:
                call()
            assert e.value.code == -3 and who + ":" in e.value.message and "destroy it and create a new one" in e.value.message, e.value.message
    finally:
        m.cleanup_update()


# ---- 7. the update.h adapter with several devices ----------------------------------------------------------------------------------------
ADAPTER = r"""
import ctypes as C, json, os, re, subprocess, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as g
pkg = g.load_package()
w, h = 96, 72

def build(spheres, lights, squash=None):
    sc = pkg.Scene.new(w, h, 60.0, 2, (0.0, 0.1, 0.2))
    for i, (c, rad, col) in enumerate(spheres):
        q = pkg.surface_make("sphere", c, [rad])
        if squash == i:
            q[10] = 2.0
        sc.add_object(q, col, 0.4 if i == 1 else 0.0)
    sc.add_object(pkg.surface_make("plane", [0, -4, 0], [0, 1, 0]), (0.5, 0.5, 0.5))
    for kind, v, col in lights:
        sc.add_light(kind, v, col, 1.0 if kind == "directional" else 300.0)
    return sc

spheres = [((-3 + 1.5 * i, 0.5 * i - 1, 12.0 + i), 0.8, (0.9, 0.2 * i, 0.3)) for i in range(5)]
lights = [("directional", (0.3, -1.0, 0.4), (1, 1, 1)), ("spherical", (2.0, 6.0, 3.0), (1, 0.9, 0.8))]
moved = [((c[0] + 0.7, c[1] - 0.3, c[2] + 1.0), rad * 1.3, (col[2], col[0], col[1])) for c, rad, col in spheres]
moved_lights = [("directional", (-0.2, -0.9, 0.5), (0.8, 0.9, 1)), ("spherical", (-2.0, 5.0, 4.0), (0.7, 1, 0.9))]
sc, new, bad = build(spheres, lights), build(moved, moved_lights), build(moved, moved_lights, squash=3)
upd = C.CDLL(pkg.UPDATE_LIB_PATH)
names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
update = getattr(upd, re.search(r"\b(_Z\d+updateRKN3glm3matI\S*)\b", names).group(1))
cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
update.argtypes, update.restype = [C.c_void_p], C.c_float
upd.mi355rt_update_scene.argtypes = [C.c_void_p]
upd.mi355rt_update_download.argtypes = [C.c_void_p, C.c_size_t]
upd.mi355rt_update_pick.argtypes = [C.c_uint, C.c_uint, C.c_void_p]
upd.mi355rt_update_pick_path.argtypes = [C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p]
upd.mi355rt_update_trace.argtypes = [C.c_void_p, C.c_uint, C.c_void_p]
upd.mi355rt_update_shade.argtypes = [C.c_void_p, C.c_uint, C.c_void_p]
cam = np.ascontiguousarray(pkg.camera_matrix((0.4, 0.3, -1.5), 84.0, -3.0), dtype=np.float64)
err = lambda: pkg.lib().rt_last_error().decode()
rng = np.random.default_rng(5)
rays = pkg.Renderer.rays(rng.uniform([-2, -2, -2], [2, 2, 2], (64, 3)), rng.normal(size=(64, 3)) + np.array([0, 0, 2.0]))
pixels = [(48, 36), (10, 60), (70, 20), (95, 71), (0, 0), (33, 30)]
out = {}
single = not os.environ.get("MI355RT_DEVICES")

def drawn():
    update(cam.ctypes.data)
    f = np.zeros((h, w, 4), np.float32)
    assert upd.mi355rt_update_download(f.ctypes.data_as(C.c_void_p), f.nbytes) == 0, err()
    return f

def queries():
    # mi355rt_update_pick keeps its refusal with several devices (tests/test_gbuffer_gpu.py pins it): plane 0 of the path is its record
    picks, segs, ends = np.zeros(len(pixels), pkg.HIT_DTYPE), np.zeros((len(pixels), 3), pkg.HIT_DTYPE), np.zeros(len(pixels), pkg.PATH_END_DTYPE)
    for i, (x, y) in enumerate(pixels):
        if single:
            assert upd.mi355rt_update_pick(x, y, picks[i:].ctypes.data) == 0, err()
        else:
            assert upd.mi355rt_update_pick(x, y, picks[i:].ctypes.data) == -1 and "several devices" in err(), err()
        assert upd.mi355rt_update_pick_path(x, y, segs[i].ctypes.data, 3, ends[i:].ctypes.data) == 0, err()
    if single:
        assert picks.tobytes() == segs[:, 0].tobytes()
    else:
        picks = segs[:, 0].copy()
    hits, rgba = np.zeros(len(rays), pkg.HIT_DTYPE), np.zeros((len(rays), 4), np.float32)
    assert upd.mi355rt_update_trace(rays.ctypes.data, len(rays), hits.ctypes.data) == 0, err()
    assert upd.mi355rt_update_shade(rays.ctypes.data, len(rays), rgba.ctypes.data) == 0, err()
    return [picks.tobytes().hex(), segs.tobytes().hex(), ends.tobytes().hex(), hits.tobytes().hex(), rgba.tobytes().hex()]

init(7, sc._h)
out["frame0"] = drawn().tobytes().hex()
out["queries0"] = queries()
out["bad"] = [upd.mi355rt_update_scene(bad._h), err()]
out["frame_after_bad"] = drawn().tobytes().hex()
out["moved"] = [upd.mi355rt_update_scene(new._h), err()]
out["frame1"] = drawn().tobytes().hex()
out["queries1"] = queries()
cleanup()
json.dump(out, open(sys.argv[2], "w"))
"""


@pytest.fixture(scope="module")
def adapter_runs(tmp_path_factory):
    """The same script twice, in fresh processes for the environment: one device, and MI355RT_DEVICES=0,0,0."""
    d = tmp_path_factory.mktemp("adapter")
    (d / "run.py").write_text(ADAPTER)
    res = {}
    for key, extra in (("single", {}), ("multi", dict(MI355RT_DEVICES="0,0,0"))):
        env = {k: v for k, v in os.environ.items() if not k.startswith("MI355RT_")}
        env.update(extra)
        p = subprocess.run([sys.executable, str(d / "run.py"), ROOT, str(d / (key + ".json"))], capture_output=True, text=True, timeout=180, env=env)
        assert p.returncode == 0, p.stderr[-3000:]
        res[key] = json.load(open(d / (key + ".json")))
    return res


def test_adapter_queries_with_several_devices_equal_the_single_device_answers(adapter_runs):
    """mi355rt_update_pick_path / _trace / _shade, and mi355rt_update_pick's record as plane 0 of the path (the hook itself keeps the refusal
    an existing test pins; the single-device run holds plane 0 to the hook's own answer)."""
    single, many = adapter_runs["single"], adapter_runs["multi"]
    for k in ("queries0", "queries1"):
        assert many[k] == single[k], k
    assert many["queries0"] != many["queries1"]
    assert many["frame0"] == single["frame0"] and many["frame1"] == single["frame1"]


def test_adapter_scene_update_with_several_devices(pkg, oracle, adapter_runs):
    many = adapter_runs["multi"]
    assert many["bad"][0] == -2 and "reason 1 at index 3:" in many["bad"][1], many["bad"]
    assert many["frame_after_bad"] == many["frame0"]
    assert many["moved"][0] == 0, many["moved"]
    got = np.frombuffer(bytes.fromhex(many["frame1"]), dtype=np.float32).reshape(H, W, 4)
    # the oracle's frame of the new scene: the script's `moved` scene, built here again
    spheres = [((-3 + 1.5 * i, 0.5 * i - 1, 12.0 + i), 0.8, (0.9, 0.2 * i, 0.3)) for i in range(5)]
    sc = pkg.Scene.new(W, H, 60.0, 2, (0.0, 0.1, 0.2))
    for i, (c, rad, col) in enumerate(spheres):
        sc.add_object(pkg.surface_make("sphere", (c[0] + 0.7, c[1] - 0.3, c[2] + 1.0), [rad * 1.3]), (col[2], col[0], col[1]), 0.4 if i == 1 else 0.0)
    sc.add_object(pkg.surface_make("plane", [0, -4, 0], [0, 1, 0]), (0.5, 0.5, 0.5))
    sc.add_light("directional", (-0.2, -0.9, 0.5), (0.8, 0.9, 1), 1.0)
    sc.add_light("spherical", (-2.0, 5.0, 4.0), (0.7, 1, 0.9), 300.0)
    want = oracle_scene(oracle, sc.arrays()).render(cam=pkg.camera_matrix(*MOVED), nthreads=8)
    assert np.array_equal(got[..., :3], want)
    assert many["frame1"] != many["frame0"]
