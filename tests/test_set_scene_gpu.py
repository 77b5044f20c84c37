"""rt_set_scene: a context whose scene was rewritten on the device must be indistinguishable from a context created from the new scene.

Everything here is bit for bit: the scene as the device holds it (rt_debug_scene_blob: the blob, DevLight[] and LightK[], which also
holds the derived values no image shows -- own_lo / own_hi, inv_r, len_u, s_* -- to rt_create), frames, G-buffer, picks, ray queries
and counters are compared with a FRESH context on the updated descriptor, and frames of degree <= 2 scenes with the CPU oracle on that
descriptor too.  There is no tolerance in this file.  Frames are 96x72 (64x48 where bands are involved)."""
import functools

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

KEYS = ("coefs", "reflection", "albedo", "light_p", "light_color")
W, H = 96, 72
REJECT_CLASS, REJECT_BOUND, REJECT_MIRROR, REJECT_CUBIC, REJECT_LIGHT = 1, 2, 3, 4, 5


# ---- scenes as dictionaries of descriptor arrays ------------------------------------------------------------------------------------
def sphere(c, r):
    c = np.asarray(c, dtype=np.float64)
    q = np.zeros(20)
    q[10:13] = 1.0
    q[16:19] = -2.0 * c
    q[19] = float(np.dot(c, c)) - r * r
    return q


def plane(p, n):
    p, n = np.asarray(p, dtype=np.float64), np.asarray(n, dtype=np.float64)
    q = np.zeros(20)
    q[16:19] = n
    q[19] = -float(np.dot(n, p))
    return q


def scene_dict(w, h, fov_deg, max_refl, bg, objects, lights):
    """objects: (coefs, albedo, reflection); lights: (is_spherical, p, colour)."""
    return dict(width=w, height=h, vertical_fov=float(np.radians(fov_deg)), bg_color=np.asarray(bg, np.float32), max_reflections=max_refl,
                coefs=np.array([o[0] for o in objects], np.float64).reshape(-1, 20), albedo=np.array([o[1] for o in objects], np.float32).reshape(-1, 3),
                reflection=np.array([o[2] for o in objects], np.float32), light_is_spherical=np.array([l[0] for l in lights], np.uint8),
                light_p=np.array([l[1] for l in lights], np.float64).reshape(-1, 3), light_color=np.array([l[2] for l in lights], np.float32).reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def base_scene(pkg, key, w=W, h=H):
    if key == "20spheres":   # unit spheres only, no mirror: tile words, the lean path, the own-sphere rule
        a = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(w, h).arrays()
    elif key == "mixed":     # every class of degree <= 2, a mirror, both kinds of light; five bounded spheres, so culling is on
        objs = [(sphere((-4 + 2.0 * i, -1.0 + 0.7 * i, 14.0 + i), 0.8 + 0.1 * i), (0.9 - 0.1 * i, 0.3 + 0.1 * i, 0.5), 0.0) for i in range(5)]
        objs[2] = (objs[2][0], objs[2][1], 0.5)                                                    # a mirror
        objs.append((plane((0, -4, 0), (0.05, 1.0, 0.02)), (0.5, 0.5, 0.5), 0.0))                  # 5: a plane
        q = np.zeros(20)
        q[10:13] = (1.0, 2.0, 0.5)
        q[13] = 0.25
        c = np.array([3.0, 2.0, 12.0])
        q[16:19] = -2.0 * q[10:13] * c
        q[19] = float(np.dot(q[10:13], c * c)) - 3.0
        objs.append((q, (0.2, 0.7, 0.9), 0.0))                                                     # 6: a general quadric
        lights = [(0, (0.3, -1.0, 0.4), (0.9, 0.9, 0.8)), (1, (2.0, 8.0, 2.0), (300.0, 280.0, 260.0)), (0, (-0.5, -0.6, 0.3), (0.3, 0.3, 0.4))]
        a = scene_dict(w, h, 55.0, 3, (0.1, 0.2, 0.3), objs, lights)
    else:                    # "cubic": one degree-3 surface, frozen; its neighbours, the materials and the lights move
        assert key == "cubic"
        q = np.zeros(20)
        q[0], q[4], q[10:13], q[19] = 0.3, -0.2, (1.0, 0.8, 1.2), -4.0
        objs = [(q, (0.8, 0.8, 0.8), 0.0), (sphere((1.5, 0.5, 2.0), 0.7), (0.9, 0.3, 0.2), 0.0), (plane((0, -3, 0), (0, 1, 0)), (0.4, 0.5, 0.4), 0.0)]
        lights = [(0, (0.3, -1.0, 0.5), (1.5, 1.5, 1.5)), (1, (2.0, 4.0, -6.0), (300.0, 270.0, 240.0))]
        a = scene_dict(w, h, 40.0, 2, (0.05, 0.1, 0.15), objs, lights)
    for v in a.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return a


def camera(pkg, key):
    return pkg.camera_matrix(pos=(0.5, 1.0, -9.0), yaw_deg=92.0, pitch_deg=-4.0) if key == "cubic" else pkg.IDENTITY.copy()


def changed(a, **kw):
    """A copy of the scene dictionary with writable arrays; kw replaces whole arrays."""
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    b.update(kw)
    return b


def desc(pkg, a):
    return pkg.desc_from_arrays(a["width"], a["height"], a["vertical_fov"], a["bg_color"], a["max_reflections"], a["coefs"], a["reflection"], a["albedo"],
                                a["light_is_spherical"], a["light_p"], a["light_color"])


def renderer(pkg, a, **kw):
    return pkg.Renderer(desc(pkg, a), device=0, **kw)


def oracle_scene(oracle, a):
    o = oracle.Scene(a["width"], a["height"], 0.0, a["max_reflections"], a["bg_color"])
    o.vertical_fov = a["vertical_fov"]
    for i in range(len(a["reflection"])):
        o.add_object(a["coefs"][i], a["albedo"][i], a["reflection"][i])
    for i in range(len(a["light_is_spherical"])):
        l = oracle.OrcLight()
        l.is_spherical = int(a["light_is_spherical"][i])
        for k in range(3):
            l.p[k] = float(a["light_p"][i][k])
            l.color[k] = float(a["light_color"][i][k])
        o.lights.append(l)
    return o


def same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def frame(r, cam):
    r.update(cam)
    return r.download().copy()


def fresh_frame(pkg, a, cam, **kw):
    r = renderer(pkg, a, **kw)
    try:
        return frame(r, cam)
    finally:
        r.cleanup_update()


def fresh_blob(pkg, a, **kw):
    r = renderer(pkg, a, **kw)
    try:
        return r.debug_scene_blob()
    finally:
        r.cleanup_update()


def apply(r, a, keys=KEYS):
    r.set_scene(**{k: a[k] for k in keys})


# ---- the updates ---------------------------------------------------------------------------------------------------------------------
def update_of(pkg, key, which):
    a = changed(base_scene(pkg, key))
    rng = np.random.default_rng(7)
    if key == "20spheres":
        n = len(a["reflection"])
        if which == "moved":        # centres, radii, colours, lights
            for i in range(n):
                a["coefs"][i] = sphere(rng.uniform([-9, -7, 11], [9, 7, 22]), float(rng.uniform(0.3, 2.5)))
            a["albedo"][:] = rng.uniform(0, 1, (n, 3))
            a["light_p"][:-1] = rng.normal(size=(len(a["light_p"]) - 1, 3)) + np.array([0, -1.0, 0])
            a["light_p"][-1] = (1.0, 5.0, 3.0)
            a["light_color"][:] = rng.uniform(0, 1, a["light_color"].shape) * a["light_color"].max()
        else:                       # "edges": the inputs whose derived values no image shows
            assert which == "edges"
            a["coefs"][0] = sphere((1.0, 2.0, 4.0), 2.0 ** -20)   # a radius near 0: r^2 = 2^-40 exactly
            a["coefs"][1] = sphere((-3.0, 1.0, 12.0), 1e-3)
            a["coefs"][2] = sphere((0.0, 1.0, 12.0), 1.5)
            a["coefs"][2][16] = 0.0                                 # kx = +0.0: a centre with a -0.0 component
            a["coefs"][3] = sphere((0.0, -2.0, 13.0), 1.0)
            a["coefs"][3][16] = -0.0                                # ... and kx = -0.0: +0.0
            a["coefs"][4] = sphere((1.0, 1.0, 20.0), 2e19)          # (r + 1)^2 = 4e38 is beyond FLT_MAX: own_hi is rounded inwards from +inf
            a["coefs"][5] = sphere((2.0 ** 20, 0.0, 2.0 ** 20), 2.0)  # S^2 dominates own_lo (r^2 = 4 exactly: 2^41 - 4 is a double)
            a["light_p"][0] = (3.2e-4, 0.0, 0.0)                    # |(float) p|^2 = 1.024e-7, just above EPS = 1e-7
            a["light_p"][1] = (0.0, -3.17e-4, 0.0)                  # 1.0049e-7
            assert 1e-7 < float(np.float32(3.17e-4)) ** 2 < 1.01e-7
    elif key == "mixed":
        for i in range(5):
            a["coefs"][i] = sphere(rng.uniform([-6, -3, 10], [6, 4, 20]), float(rng.uniform(0.4, 2.0)))
        a["coefs"][5] = plane((0, -5, 0), (-0.1, 1.0, 0.05))
        a["coefs"][6][10:13] = (0.7, 1.0, 1.8)
        a["coefs"][6][14] = -0.3
        a["coefs"][6][19] += 1.0
        a["albedo"][:] = rng.uniform(0, 1, a["albedo"].shape)
        a["reflection"][2] = 0.3            # still the scene's mirror
        a["light_p"][0] = (-0.2, -0.8, 0.6)
        a["light_p"][1] = (-3.0, 6.0, 5.0)
        a["light_color"][:] *= np.float32(0.7)
    else:
        a["coefs"][1] = sphere((1.0, 1.0, 3.0), 1.1)
        a["coefs"][2] = plane((0, -2.5, 0), (0.1, 1.0, 0.0))
        a["albedo"][:] = rng.uniform(0, 1, a["albedo"].shape)   # the cubic's too
        a["light_p"][0] = (-0.4, -0.9, 0.3)
        a["light_p"][1] = (-2.0, 5.0, -4.0)
        a["light_color"][1] = (200.0, 260.0, 300.0)
    return a


# ---- 1. the device holds what rt_create would have uploaded ------------------------------------------------------------------------------
@pytest.mark.parametrize("key,which", [("20spheres", "moved"), ("20spheres", "edges"), ("mixed", "moved"), ("cubic", "moved")])
def test_blob_equals_a_fresh_context(pkg, key, which):
    old, new = base_scene(pkg, key), update_of(pkg, key, which)
    r = renderer(pkg, old)
    try:
        assert same(r.debug_scene_blob(), fresh_blob(pkg, old))
        assert not same(fresh_blob(pkg, old), fresh_blob(pkg, new)), "the update changes nothing"
        apply(r, new)
        got, want = r.debug_scene_blob(), fresh_blob(pkg, new)
        diff = np.flatnonzero(got != want)
        assert same(got, want), f"{diff.size} bytes differ, the first at offset {diff[0] if diff.size else -1} of {got.size}"
        assert r.set_scene_status() == dict(applied=1, rejected=0, reason=0, index=0)
        apply(r, old)   # and back
        assert same(r.debug_scene_blob(), fresh_blob(pkg, old))
    finally:
        r.cleanup_update()


def test_fast_contexts_get_the_same_scene(pkg):
    """The derived data is the scene's, not the variant's: rt_create forms it without contraction for RT_FLAG_FAST contexts too."""
    new = update_of(pkg, "mixed", "moved")
    r = renderer(pkg, base_scene(pkg, "mixed"), flags=pkg.RT_FLAG_FAST)
    try:
        apply(r, new)
        assert same(r.debug_scene_blob(), fresh_blob(pkg, new, flags=pkg.RT_FLAG_FAST))
        assert same(r.debug_scene_blob(), fresh_blob(pkg, new))
    finally:
        r.cleanup_update()


# ---- 2. frames and queries ---------------------------------------------------------------------------------------------------------
def variants(pkg):
    return [("default", {}), ("nolean", dict(flags=pkg.RT_FLAG_NOLEAN)), ("simple", dict(flags=pkg.RT_FLAG_SIMPLE)), ("nocull", dict(flags=pkg.RT_FLAG_NOCULL)),
            ("rgba8", dict(fmt=pkg.RT_FMT_RGBA8)), ("ssaa2", dict(flags=pkg.RT_FLAG_SSAA2)),
            ("adaptive+geometry", dict(flags=pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA_ADAPTIVE | pkg.RT_FLAG_SSAA_GEOMETRY))]


@pytest.mark.parametrize("key", ["20spheres", "mixed"])
@pytest.mark.parametrize("variant", range(7))
def test_frame_after_update_equals_fresh_context_and_oracle(pkg, oracle, key, variant):
    name, kw = variants(pkg)[variant]
    old, new, cam = base_scene(pkg, key), update_of(pkg, key, "moved"), camera(pkg, key)
    r = renderer(pkg, old, **kw)
    try:
        before = frame(r, cam)   # (a frame of the old scene first: the frame state the update has to live with)
        assert same(before, fresh_frame(pkg, old, cam, **kw))
        apply(r, new)
        got = frame(r, cam)
        assert same(got, fresh_frame(pkg, new, cam, **kw)), name
        assert not same(got, before)
        if not kw:   # one ray per pixel in RGBA32F: the oracle's own frame
            assert np.array_equal(got[..., :3], oracle_scene(oracle, new).render(cam=cam, nthreads=8))
        assert same(frame(r, cam), got), "the second frame after the update"
    finally:
        r.cleanup_update()


def test_cubic_scene_frame_equals_fresh_context(pkg):
    old, new, cam = base_scene(pkg, "cubic"), update_of(pkg, "cubic", "moved"), camera(pkg, "cubic")
    r = renderer(pkg, old)
    try:
        frame(r, cam)
        apply(r, new)
        assert same(frame(r, cam), fresh_frame(pkg, new, cam))
    finally:
        r.cleanup_update()


@pytest.mark.parametrize("key", ["20spheres", "mixed"])
def test_bands_of_rank_1_of_2(pkg, oracle, key):
    old, new = changed(base_scene(pkg, key), width=64, height=48), changed(update_of(pkg, key, "moved"), width=64, height=48)
    cam, kw = camera(pkg, key), dict(rank=1, world=2, band_rows=8)
    r = renderer(pkg, old, **kw)
    try:
        frame(r, cam)
        apply(r, new)
        got = frame(r, cam)
        assert same(got, fresh_frame(pkg, new, cam, **kw))
        assert np.array_equal(got[..., :3], oracle_scene(oracle, new).render(cam=cam, nthreads=8)[r.row_map()])
    finally:
        r.cleanup_update()


@pytest.mark.parametrize("key", ["20spheres", "mixed"])
def test_queries_after_update_equal_fresh_context(pkg, key):
    old, new, cam = base_scene(pkg, key), update_of(pkg, key, "moved"), camera(pkg, key)
    rng = np.random.default_rng(3)
    xy = np.stack([rng.integers(0, W, 40), rng.integers(0, H, 40)], axis=1)
    o = rng.uniform([-2, -2, -2], [2, 2, 2], (300, 3))
    d = rng.normal(size=(300, 3)) + np.array([0, 0, 2.0])

    def answers(r):
        go, gt, gn, _ = r.gbuffer(cam)
        blocked, _ = r.occluded(o, d)
        return [go.cpu().numpy(), gt.cpu().numpy(), gn.cpu().numpy(), r.pick(xy, cam), r.trace(o, d), blocked.cpu().numpy(), r.shade(o, d)]

    r, f = renderer(pkg, old), renderer(pkg, new)
    try:
        stale = answers(r)
        apply(r, new)
        got, want = answers(r), answers(f)
        for i, (g, w_) in enumerate(zip(got, want)):
            assert same(g, w_), i
        assert not all(same(g, s) for g, s in zip(got, stale))
    finally:
        r.cleanup_update()
        f.cleanup_update()


# ---- 3. frame state ------------------------------------------------------------------------------------------------------------------
def stateless_flags(pkg):
    return pkg.RT_FLAG_STATIC_ORDER | pkg.RT_FLAG_NOSCAN | pkg.RT_FLAG_NOSPLIT | pkg.RT_FLAG_NOLEAN


def animation_step(pkg, k):
    """Sphere 0 crosses the frame from left to right (tile words flip between EMPTY and NONEMPTY), sphere 1 grows past its neighbours
    (the tiles' cost order changes)."""
    a = changed(base_scene(pkg, "20spheres"))
    a["coefs"][0] = sphere((-9.0 + 2.6 * k, -4.5, 15.0), 1.0)
    a["coefs"][1] = sphere((6.0, 6.0, 15.0), 0.5 + 0.5 * k)
    return a


COUNTED = ("primary_rays", "shadow_rays", "hits", "tests")   # (tests_executed is left out, as in test_shade_gpu.py)


def test_eight_steps_of_update_and_two_renders(pkg):
    cam = pkg.IDENTITY.copy()
    count = pkg.RT_FLAG_COUNT | pkg.RT_FLAG_NOLEAN   # the counted contexts are pinned to one schedule
    r, rc = renderer(pkg, base_scene(pkg, "20spheres")), renderer(pkg, base_scene(pkg, "20spheres"), flags=count)
    try:
        frame(r, cam)
        frames = []
        for k in range(8):
            a = animation_step(pkg, k)
            want = fresh_frame(pkg, a, cam, flags=stateless_flags(pkg))
            frames.append(want)
            apply(r, a, keys=("coefs",))
            assert same(frame(r, cam), want), f"step {k}, first frame"
            assert same(frame(r, cam), want), f"step {k}, second frame"
            f = renderer(pkg, a, flags=count)
            f.update(cam)
            fc = f.counters()
            f.cleanup_update()
            apply(rc, a, keys=("coefs",))
            for rep in range(2):
                assert same(frame(rc, cam), want)
                c = rc.counters()
                assert {n: c[n] for n in COUNTED} == {n: fc[n] for n in COUNTED}, f"step {k}, frame {rep}"
        assert sum(not same(frames[k], frames[k + 1]) for k in range(7)) == 7
        assert r.set_scene_status()["applied"] == 8
    finally:
        r.cleanup_update()
        rc.cleanup_update()


# ---- 4. partial updates ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["20spheres", "mixed"])
@pytest.mark.parametrize("only", ["light_p", "albedo"])
def test_partial_update_equals_full_update(pkg, key, only):
    old, cam = base_scene(pkg, key), camera(pkg, key)
    new = changed(old, **{only: update_of(pkg, key, "moved")[only]})
    p, f = renderer(pkg, old), renderer(pkg, old)
    try:
        apply(p, new, keys=(only,))
        apply(f, new)   # the other four arrays repeat the old values
        assert same(p.debug_scene_blob(), f.debug_scene_blob())
        assert same(p.debug_scene_blob(), fresh_blob(pkg, new))
        assert same(frame(p, cam), frame(f, cam))
    finally:
        p.cleanup_update()
        f.cleanup_update()


# ---- 5. rejection is all or nothing ------------------------------------------------------------------------------------------------------
def rejected_case(pkg, name):
    """(scene key, the offending scene, reason, index)"""
    if name == "sphere to ellipsoid":
        a = update_of(pkg, "mixed", "moved")
        a["coefs"][3][10] = 2.0
        return "mixed", a, REJECT_CLASS, 3
    if name == "r^2 <= 0":
        a = update_of(pkg, "mixed", "moved")
        a["coefs"][1][19] = float(np.dot(a["coefs"][1][16:19], a["coefs"][1][16:19])) / 4.0 + 1.0
        return "mixed", a, REJECT_BOUND, 1
    if name == "plane gains a square term":
        a = update_of(pkg, "mixed", "moved")
        a["coefs"][5][11] = 0.5
        return "mixed", a, REJECT_CLASS, 5
    if name == "first mirror":
        a = update_of(pkg, "20spheres", "moved")
        a["reflection"][4] = 0.5
        return "20spheres", a, REJECT_MIRROR, 4
    if name == "NaN albedo":
        a = update_of(pkg, "20spheres", "moved")
        a["albedo"][7, 1] = np.nan
        return "20spheres", a, REJECT_LIGHT, 0   # every light's colour is finite: the first light's flags change first
    if name == "zero light direction":
        a = update_of(pkg, "20spheres", "moved")
        a["light_p"][2] = 0.0
        return "20spheres", a, REJECT_LIGHT, 2
    assert name == "cubic coefficient"
    a = update_of(pkg, "cubic", "moved")
    a["coefs"][0][3] += 1e-9
    return "cubic", a, REJECT_CUBIC, 0


@pytest.mark.parametrize("name", ["sphere to ellipsoid", "r^2 <= 0", "plane gains a square term", "first mirror", "NaN albedo", "zero light direction",
                                  "cubic coefficient"])
def test_rejection_is_all_or_nothing(pkg, name):
    import torch
    key, bad, reason, index = rejected_case(pkg, name)
    old, cam = base_scene(pkg, key), camera(pkg, key)
    r = renderer(pkg, old)
    try:
        apply(r, update_of(pkg, key, "moved"))   # (an accepted update first: the scene the refusal must leave alone is not rt_create's)
        blob, before = r.debug_scene_blob(), frame(r, cam)
        with pytest.raises(pkg.SceneException) as e:
            apply(r, bad)
        assert e.value.code == -2 and f"reason {reason} at index {index}:" in e.value.message, e.value.message
        assert r.set_scene_status() == dict(applied=1, rejected=1, reason=reason, index=index)
        assert same(r.debug_scene_blob(), blob)
        assert same(frame(r, cam), before)
        # the device entry point on the same data
        dev = {k: torch.from_numpy(np.ascontiguousarray(bad[k])).to("cuda:0") for k in KEYS}
        torch.cuda.synchronize()
        r.set_scene_into(**{k: t.data_ptr() for k, t in dev.items()})
        assert r.set_scene_status() == dict(applied=1, rejected=2, reason=reason, index=index)
        assert same(r.debug_scene_blob(), blob)
        assert same(frame(r, cam), before)
    finally:
        r.cleanup_update()


def test_losing_the_last_mirror_is_rejected_and_keeping_one_is_not(pkg):
    old = base_scene(pkg, "mixed")
    r = renderer(pkg, old)
    try:
        a = changed(old)
        a["reflection"][2], a["reflection"][4] = 0.0, 0.6   # the mirror moves to another object: the scene keeps one
        apply(r, a)
        assert same(r.debug_scene_blob(), fresh_blob(pkg, a))
        b = changed(a)
        b["reflection"][4] = 0.0
        with pytest.raises(pkg.SceneException):
            apply(r, b)
        st = r.set_scene_status()
        assert (st["reason"], st["index"]) == (REJECT_MIRROR, 4)
        assert same(r.debug_scene_blob(), fresh_blob(pkg, a))
    finally:
        r.cleanup_update()


def test_bad_arguments(pkg):
    import ctypes as C
    import torch
    old = base_scene(pkg, "20spheres")
    r = renderer(pkg, old)
    try:
        lib, buf = pkg.lib(), torch.zeros(4096, dtype=torch.float64, device="cuda:0")
        assert lib.rt_set_scene(r._h, C.byref(pkg.SceneUpdate()), None) == -1 and b"all five" in lib.rt_last_error()
        assert lib.rt_set_scene(r._h, C.byref(pkg.SceneUpdate(coefs=buf.data_ptr() + 4)), None) == -1
        assert lib.rt_set_scene(r._h, C.byref(pkg.SceneUpdate(albedo=buf.data_ptr() + 2)), None) == -1
        assert lib.rt_set_scene_host(r._h, C.byref(pkg.SceneUpdate()), None) == -1
        assert r.set_scene_status() == dict(applied=0, rejected=0, reason=0, index=0)
        no_lights = changed(old, light_is_spherical=np.zeros(0, np.uint8), light_p=np.zeros((0, 3)), light_color=np.zeros((0, 3), np.float32))
        n = renderer(pkg, no_lights)
        try:
            assert lib.rt_set_scene(n._h, C.byref(pkg.SceneUpdate(light_p=buf.data_ptr())), None) == -1 and b"without lights" in lib.rt_last_error()
            apply(n, update_of(pkg, "20spheres", "moved"), keys=("coefs", "albedo"))
            assert same(n.debug_scene_blob(), fresh_blob(pkg, changed(no_lights, coefs=update_of(pkg, "20spheres", "moved")["coefs"],
                                                                        albedo=update_of(pkg, "20spheres", "moved")["albedo"])))
        finally:
            n.cleanup_update()
    finally:
        r.cleanup_update()


# ---- 6. captured into a graph ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("static_order", [True, False])
def test_graph_of_updates_and_renders_replays_from_rewritten_arrays(pkg, static_order):
    import torch
    cam = pkg.IDENTITY.copy()
    flags = pkg.RT_FLAG_COUNT | pkg.RT_FLAG_NOLEAN | (pkg.RT_FLAG_STATIC_ORDER if static_order else 0)
    steps = [animation_step(pkg, k) for k in (1, 4, 6, 2, 7, 3)]
    want = [fresh_frame(pkg, a, cam, flags=stateless_flags(pkg)) for a in steps]
    r = renderer(pkg, base_scene(pkg, "20spheres"), flags=flags)
    s = torch.cuda.Stream()
    try:
        r.update(cam, stream=s.cuda_stream, timed=False)   # (first call on this stream before the capture)
        with torch.cuda.stream(s):
            arrays = [torch.from_numpy(steps[k]["coefs"].copy()).to("cuda:0", non_blocking=False) for k in range(3)]
            bufs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(3)]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for t, b in zip(arrays, bufs):
                r.set_scene_into(coefs=t.data_ptr(), stream=s.cuda_stream)
                r.update(cam, dev_fb=b.data_ptr(), stream=s.cuda_stream, timed=False)
        for launch in range(2):
            with torch.cuda.stream(s):
                for k, t in enumerate(arrays):   # the replay reads the arrays again: rewrite them first
                    t.copy_(torch.from_numpy(steps[3 * launch + k]["coefs"].copy()))
                for b in bufs:
                    b.view(torch.int32).fill_(0x7FC00000)
                g.replay()
            s.synchronize()
            for k, b in enumerate(bufs):
                assert same(b.cpu().numpy(), want[3 * launch + k]), f"launch {launch}, frame {k}"
        assert r.set_scene_status()["applied"] == 6
        # the frame after the replay: the scene of the last update, with correct counters
        r.update(cam, stream=s.cuda_stream, timed=False)
        s.synchronize()
        assert same(r.download(), want[5])
        f = renderer(pkg, steps[5], flags=flags)
        f.update(cam)
        fc, c = f.counters(), r.counters()
        f.cleanup_update()
        assert {n: c[n] for n in COUNTED} == {n: fc[n] for n in COUNTED}
        del g
    finally:
        torch.cuda.synchronize()
        r.cleanup_update()


# ---- 7. streams ------------------------------------------------------------------------------------------------------------------------
def test_update_on_another_stream_is_ordered_behind_the_previous_frame(pkg):
    import torch
    old, new, cam = base_scene(pkg, "mixed"), update_of(pkg, "mixed", "moved"), camera(pkg, "mixed")
    r = renderer(pkg, old)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        first = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        dev = {k: torch.from_numpy(np.ascontiguousarray(new[k])).to("cuda:0") for k in KEYS}
        torch.cuda.synchronize()
        r.update(cam, dev_fb=first.data_ptr(), stream=sa.cuda_stream, timed=False)
        # enqueue only, nothing waits on the host: stream B waits for the frame on stream A (the event behind it), then rewrites the scene
        r.set_scene_into(stream=sb.cuda_stream, **{k: t.data_ptr() for k, t in dev.items()})
        r.update(cam, stream=sb.cuda_stream, timed=False)
        torch.cuda.synchronize()
        assert same(first.cpu().numpy(), fresh_frame(pkg, old, cam)), "the earlier frame is the old scene"
        assert same(r.download(), fresh_frame(pkg, new, cam)), "the later frame is the updated one"
    finally:
        torch.cuda.synchronize()
        r.cleanup_update()



def test_status_and_host_entry_refuse_a_capturing_stream(pkg):
    """rt_set_scene_host allocates and waits, rt_set_scene_status and rt_debug_scene_blob wait: on a capturing stream each says so
    (RT_ERR_INVALID) instead of failing inside the runtime, and the capture goes on."""
    import ctypes as C
    import torch
    old, new, cam = base_scene(pkg, "20spheres"), update_of(pkg, "20spheres", "moved"), pkg.IDENTITY.copy()
    r = renderer(pkg, old)
    s = torch.cuda.Stream()
    try:
        r.update(cam, stream=s.cuda_stream, timed=False)
        dev = torch.from_numpy(new["coefs"].copy()).to("cuda:0")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            r.set_scene_into(coefs=dev.data_ptr(), stream=s.cuda_stream)
            with pytest.raises(pkg.RtError) as e:
                r.set_scene(coefs=new["coefs"], stream=s.cuda_stream)
            assert e.value.code == -1 and "capturing" in e.value.message
            with pytest.raises(pkg.RtError) as e:
                r.set_scene_status()
            assert e.value.code == -1 and "capturing" in e.value.message
            n = C.c_size_t()
            buf = np.zeros(1 << 20, np.uint8)
            assert pkg.lib().rt_debug_scene_blob(r._h, buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(n)) == -1
            r.update(cam, stream=s.cuda_stream, timed=False)
        assert r.set_scene_status()["applied"] == 0   # (captured, not run)
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        assert r.set_scene_status() == dict(applied=1, rejected=0, reason=0, index=0)
        assert same(r.download(), fresh_frame(pkg, changed(old, coefs=new["coefs"]), cam))
        del g
    finally:
        torch.cuda.synchronize()
        r.cleanup_update()


# ---- the update.h adapter ----------------------------------------------------------------------------------------------------------------
def test_update_adapter_moves_the_scene(pkg):
    """mi355rt_update_scene of libmi355rt_update.so (ctypes, as tests/test_shade_gpu.py drives its siblings: init_update receives the
    loaded scene's Scene object, the first member of the rt_scene handle): refused before init_update, with other counts and with
    another light kind; a layout change is RT_ERR_SCENE and leaves the scene alone; an accepted one is what the next update() draws."""
    import ctypes as C
    import re
    import subprocess
    w, h = 96, 72

    def build(spheres, lights, refl=0.0):
        sc = pkg.Scene.new(w, h, 60.0, 2, (0.0, 0.1, 0.2))
        for c, rad, col in spheres:
            sc.add_object(pkg.surface_make("sphere", c, [rad]), col, refl)
        sc.add_object(pkg.surface_make("plane", [0, -4, 0], [0, 1, 0]), (0.5, 0.5, 0.5))
        for kind, v, col in lights:
            sc.add_light(kind, v, col, 1.0 if kind == "directional" else 300.0)
        return sc

    spheres = [((-3 + 1.5 * i, 0.5 * i - 1, 12.0 + i), 0.8, (0.9, 0.2 * i, 0.3)) for i in range(5)]
    lights = [("directional", (0.3, -1.0, 0.4), (1, 1, 1)), ("spherical", (2.0, 6.0, 3.0), (1, 0.9, 0.8))]
    moved = [((c[0] + 0.7, c[1] - 0.3, c[2] + 1.0), rad * 1.3, (col[2], col[0], col[1])) for c, rad, col in spheres]
    moved_lights = [("directional", (-0.2, -0.9, 0.5), (0.8, 0.9, 1)), ("spherical", (-2.0, 5.0, 4.0), (0.7, 1, 0.9))]
    sc, new = build(spheres, lights), build(moved, moved_lights)
    upd = C.CDLL(pkg.UPDATE_LIB_PATH)
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
    update = getattr(upd, re.search(r"\b(_Z\d+updateRKN3glm3matI\S*)\b", names).group(1))
    cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
    init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
    update.argtypes, update.restype = [C.c_void_p], C.c_float
    upd.mi355rt_update_scene.argtypes = [C.c_void_p]
    upd.mi355rt_update_download.argtypes = [C.c_void_p, C.c_size_t]
    cam = np.ascontiguousarray(pkg.IDENTITY, dtype=np.float64)

    def drawn():
        update(cam.ctypes.data)
        out = np.zeros((h, w, 4), np.float32)
        assert upd.mi355rt_update_download(out.ctypes.data_as(C.c_void_p), out.nbytes) == 0
        return out

    def frame_of(scene):
        r = pkg.Renderer(scene, device=0)
        try:
            return frame(r, cam)
        finally:
            r.cleanup_update()

    err = pkg.lib().rt_last_error
    assert upd.mi355rt_update_scene(new._h) == -1 and b"init_update" in err()
    init(7, sc._h)
    try:
        before = drawn()
        assert same(before, frame_of(sc))
        assert upd.mi355rt_update_scene(build(moved[:4], moved_lights)._h) == -1 and b"number of objects" in err()
        assert upd.mi355rt_update_scene(build(moved, moved_lights[:1])._h) == -1
        assert upd.mi355rt_update_scene(build(moved, [moved_lights[0], ("directional", (0, -1, 0), (1, 1, 1))])._h) == -1 and b"kind" in err()
        assert upd.mi355rt_update_scene(build(moved, moved_lights, refl=0.5)._h) == -2 and b"reason 3 at index 0" in err()   # a first mirror
        assert same(drawn(), before)
        assert upd.mi355rt_update_scene(new._h) == 0, err()
        after = drawn()
        assert same(after, frame_of(new)) and not same(after, before)
    finally:
        cleanup()
    assert upd.mi355rt_update_scene(new._h) == -1
