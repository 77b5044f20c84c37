#!/usr/bin/env python3
"""Scenes that only a raw rt_scene_desc can hold (pkg.desc_from_arrays, the documented ABI boundary): directional lights whose
direction is not of unit length (short, zero, long, NaN, inf), light colours / albedos / reflection ratios / background colours that
are not finite or not in [0, 1].  The scene factories (Scene.add_light, orc_light_*, the YAML loader) normalise and validate, so no
scene of theirs reaches the arms the kernels keep for these inputs (rt_capi.cpp, "backface_exact" / LightK.flags / lights_plain;
rt_wavefront.hip, the general light loop of the lean path and phase B of the general instantiation).

Everything here is an oracle Scene whose lights are stored records (never through a factory); `desc(pkg, osc)` hands the same arrays
to the product.  The module imports without the GPU library: the host tests use it too.

* NAMED: name -> (class, layout, oddity); `named(name)` builds (scene, twin, cameras).  The twin is the scene with the oddity
  removed (direction of unit length, ordinary colour ...); tests/test_raw_descriptor_host.py asserts that the oracle's frames of the
  two differ, so a kernel that took the ordinary arm cannot pass the GPU comparison.
* `flags(osc)`: backface_exact and the quadratic-branch bit per directional light and lights_plain per scene, recomputed in numpy by
  the rules of rt_create.
* `scene(seed)`: a seeded generator over the object ranges of fuzz_parity / fuzz_spheres with oddities sprinkled in.
* main(): N seeds through all kernels and the oracle (needs a GPU).  usage: python tests/tools/raw_desc_scenes.py [n_scenes] [first_seed]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

EPS = 1e-7                      # include/surface_impl.h:16: |d|^2 <= EPS takes the linear branch
INF, NAN = float("inf"), float("nan")
BG = (0.2, 0.3, 0.4)
N_SEEDS = 24                    # the sample of scene(seed) the test suites run


# ---- pieces ------------------------------------------------------------------------------------------------------------------
def sphere(c, r):
    out = (C.c_double * 20)()
    O.lib().orc_surface_sphere(O._d3(c), float(r), out)
    return list(out)


def plane(origin, normal):
    out = (C.c_double * 20)()
    O.lib().orc_surface_plane(O._d3(origin), O._d3(normal), out)
    return list(out)


def stored_light(is_spherical, p, color):
    """A light record as stored: p is the (negated) direction or the position, colour already times intensity."""
    l = O.OrcLight()
    l.is_spherical = int(bool(is_spherical))
    for k in range(3):
        l.p[k] = float(p[k])
        l.color[k] = float(np.float32(color[k]))
    return l


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt(np.dot(v, v))


def u2_of(p):
    """|(float) p|^2 as rt_create forms it: the direction's round trip through float, then (xx + yy) + zz in double."""
    f = np.asarray(p, dtype=np.float64).astype(np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return float((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2])


def at_eps(direction, above):
    """`direction` scaled to the float vector whose squared length is the smallest one above EPS (above) or the largest one not
    above it, moving its largest component one float at a time."""
    f = (unit(direction) * np.sqrt(EPS)).astype(np.float32)
    k = int(np.argmax(np.abs(f)))
    away, back = np.float32(np.sign(f[k]) * np.inf), np.float32(0.0)
    while not u2_of(f) > EPS:
        f[k] = np.nextafter(f[k], away)
    while True:
        g = f.copy()
        g[k] = np.nextafter(g[k], back)
        if not u2_of(g) > EPS:
            break
        f = g
    out = f if above else g
    assert (u2_of(out) > EPS) == above
    return out.astype(np.float64)


def copy_scene(s):
    t = O.Scene(s.width, s.height, s.fov_deg, s.max_reflections, np.array(s.bg_color, dtype=np.float32))
    t.vertical_fov = s.vertical_fov
    for o in s.objects:
        t.add_object(list(o.c), list(o.color), o.reflection_ratio)
    for l in s.lights:
        t.lights.append(stored_light(l.is_spherical, list(l.p), list(l.color)))
    return t


def desc(pkg, osc):
    """The rt_scene_desc of an oracle scene: the same arrays, nothing normalised or validated on the way."""
    return pkg.desc_from_arrays(osc.width, osc.height, osc.vertical_fov, osc.bg_color, osc.max_reflections, osc.coefs, osc.reflection,
                                osc.albedo, osc.light_is_spherical, osc.light_p, osc.light_color)


def flags(osc):
    """(bfe [n_lights], quad_l [n_lights], lights_plain, odd): rt_create's backface_exact (directional, its colour and every albedo
    finite), LightK.flags bit 4 (|(float) d|^2 > EPS; fabs(NaN) > EPS is false) per light, lights_plain (every directional light has
    both) and the indices of the directional lights that clear it."""
    alb_ok = bool(np.all(np.isfinite(osc.albedo)))
    sph = osc.light_is_spherical.astype(bool)
    col, p = osc.light_color, osc.light_p
    bfe = np.array([(not sph[i]) and alb_ok and bool(np.all(np.isfinite(col[i]))) for i in range(len(sph))], dtype=bool)
    quad = np.array([abs(u2_of(p[i])) > EPS for i in range(len(sph))], dtype=bool)
    odd = [i for i in range(len(sph)) if not sph[i] and not (bfe[i] and quad[i])]
    return bfe, quad, int(not odd), odd


# ---- scene classes -----------------------------------------------------------------------------------------------------------
CLASSES = ("lean", "lean65", "mirror", "gq", "cubic")
SPHERE_ONLY = ("lean", "lean65")


def _objects(cls):
    """[(coefs, albedo, reflection)], (w, h), depth, cameras"""
    cams = [None, O.camera_matrix((0.6, 0.4, -1.5), 86.0, 3.0)]
    if cls == "lean":      # six spheres, two pairs overlapping, one in front of another (shadows of every light fall on something)
        objs = [(sphere(c, r), a, 0.0) for c, r, a in (((-2.5, 0.3, 10), 1.6, (0.9, 0.3, 0.2)), ((-0.8, -0.2, 9), 1.0, (0.2, 0.9, 0.3)),
                                                        ((1.5, 0.5, 11), 1.8, (0.3, 0.4, 0.9)), ((2.6, -0.6, 8.5), 0.8, (0.9, 0.9, 0.2)),
                                                        ((0.3, 1.8, 10), 0.9, (0.8, 0.8, 0.8)), ((0.0, -3.5, 11), 2.5, (0.6, 0.5, 0.4)))]
        return objs, (64, 48), 2, cams
    if cls == "lean65":    # seventy spheres: two 64-entry groups
        rng = np.random.default_rng(6500)
        objs = [(sphere(rng.uniform([-7, -4.5, 7], [7, 4.5, 20]), float(rng.uniform(0.4, 1.1))), rng.uniform(0.1, 1, 3), 0.0) for _ in range(70)]
        return objs, (96, 64), 2, cams
    if cls == "mirror":
        objs = [(sphere((-2.2, 0.0, 9), 1.7), (0.9, 0.3, 0.2), 0.5), (sphere((1.8, 0.2, 10), 1.9), (0.3, 0.5, 0.9), 0.0),
                (sphere((0.0, -0.9, 6.5), 0.7), (0.9, 0.9, 0.3), 0.0), (sphere((0.2, 2.4, 10), 1.0), (0.8, 0.8, 0.8), 0.35),
                (sphere((0.0, -52.5, 10), 50.0), (0.5, 0.6, 0.5), 0.0)]
        return objs, (64, 48), 3, cams
    if cls == "gq":        # spheres, a plane, an ellipsoid and a quadric with cross terms
        q1 = np.zeros(20); q1[10], q1[11], q1[12], q1[18], q1[19] = 1.0, 4.0, 0.5, -9.0, 36.0
        q2 = np.zeros(20); q2[10:16] = (1.0, 2.0, 1.5, 0.5, -0.3, 0.2); q2[16], q2[18], q2[19] = 4.0, -27.0, 122.0
        objs = [(sphere((-2.6, 0.4, 10), 1.3), (0.9, 0.3, 0.2), 0.0), (list(q1), (0.3, 0.9, 0.3), 0.0), (list(q2), (0.3, 0.3, 0.9), 0.0),
                (plane((0, -2.5, 0), (0.02, 1, 0.03)), (0.6, 0.6, 0.6), 0.0), (sphere((2.4, -1.2, 7.5), 0.9), (0.9, 0.9, 0.2), 0.0)]
        return objs, (64, 48), 2, cams
    if cls == "cubic":     # test_gpu_parity.random_cubic_scene(seed 3): one degree-3 surface next to a sphere and a plane
        rng = np.random.default_rng(503)
        q = np.zeros(20)
        q[:10] = rng.uniform(-1, 1, 10) * (rng.random(10) < 0.6)
        q[10:16], q[16:19], q[19] = rng.uniform(-1, 1, 6), rng.uniform(-2, 2, 3), rng.uniform(-4, 4)
        objs = [(list(q), (0.8, 0.8, 0.8), 0.0), (sphere((1.5, 0.5, 2.0), 0.7), (0.9, 0.3, 0.2), 0.0), (plane((0, -3, 0), (0, 1, 0)), (0.4, 0.5, 0.4), 0.0)]
        return objs, (64, 48), 2, [O.camera_matrix((0.5, 1.0, -9.0), 92.0, -4.0), O.camera_matrix((0.2, 1.4, -8.0), 88.0, -6.0)]
    raise KeyError(cls)


D_T, D_1 = unit((0.35, 1.0, -0.45)), unit((-0.5, 0.8, -0.3))     # light.p of a directional light: towards the light
P_T, P_1 = (3.0, 6.0, 4.0), (-4.0, 5.0, 3.0)


def base(cls, layout, point_target=False):
    """(scene, index of the directional target, index of the point-light target).  Layouts: "first" = the targets lead the list,
    "last" = the target of the oddity's kind ends it, "many" = 40 lights with the targets past the first 32-bit shadow word."""
    objs, (w, h), depth, cams = _objects(cls)
    s = O.Scene(w, h, 50.0, depth, BG)
    for c, a, r in objs:
        s.add_object(c, a, r)
    if cls == "cubic":
        pt, p1 = (2.0, 4.0, -6.0), (-3.0, 5.0, -5.0)
    else:
        pt, p1 = P_T, P_1
    dt, d1 = stored_light(0, D_T, (0.7, 0.6, 0.5)), stored_light(0, D_1, (0.25, 0.3, 0.35))
    lt, l1 = stored_light(1, pt, (40.0, 45.0, 50.0)), stored_light(1, p1, (20.0, 15.0, 12.0))
    if layout == "first":
        s.lights += [dt, lt, d1, l1]
        return s, cams, 0, 1
    if layout == "last":
        s.lights += [d1, l1] + ([dt, lt] if point_target else [lt, dt])
        return s, cams, (2 if point_target else 3), (3 if point_target else 2)
    rng = np.random.default_rng(4000)
    for i in range(38):   # dim, so that the sum stays below the clamp
        if i % 2 == 0:
            s.lights.append(stored_light(0, unit(rng.normal(size=3) + np.array([0, 1.5, -0.5])), rng.uniform(0.0, 0.04, 3)))
        else:
            s.lights.append(stored_light(1, rng.uniform([-9, 2, -2], [9, 9, 8]), rng.uniform(0.0, 2.5, 3)))
    s.lights.insert(33, dt)
    s.lights.insert(35, lt)
    return s, cams, 33, 35


# ---- oddities: name -> (kind, fn(scene, directional target, point target)) ----------------------------------------------------
def _dir(p=None, scale=None, color=None):
    def fn(s, d, _):
        l = s.lights[d]
        v = np.array(list(l.p)) if p is None else np.asarray(p(np.array(list(l.p))), dtype=np.float64)
        if scale is not None:
            v = v * scale
        for k in range(3):
            l.p[k] = float(v[k])
        if color is not None:
            c = color(np.array(list(l.color), dtype=np.float64))
            for k in range(3):
                l.color[k] = float(np.float32(c[k]))
    return fn


def _color(which, fn_c):
    def fn(s, d, p):
        l = s.lights[d if which == "d" else p]
        c = fn_c(np.array(list(l.color), dtype=np.float64))
        for k in range(3):
            l.color[k] = float(np.float32(c[k]))
    return fn


def _albedo(value, everywhere):
    def fn(s, d, p):
        for o in (s.objects if everywhere else s.objects[:1]):
            for k in range(3):
                if value[k] is not None:
                    o.color[k] = value[k]
    return fn


def _bg(value):
    def fn(s, d, p):
        s.bg_color = np.asarray(value, dtype=np.float32)
    return fn


def _refl(value):
    def fn(s, d, p):
        for o in s.objects:
            if o.reflection_ratio > 0:
                o.reflection_ratio = value
                return
    return fn


def _both(*fns):
    def fn(s, d, p):
        for f in fns:
            f(s, d, p)
    return fn


def _set(c, i, v):
    c = c.copy()
    c[i] = v
    return c


def _put(v, i, x):
    v = v.copy()
    v[i] = x
    return v


ODDITIES = {
    # direction length (bit 4 of LightK.flags); the colour keeps the light visible
    "dir_eps_above": _dir(p=lambda v: at_eps(v, True), color=lambda c: c / np.sqrt(EPS)),
    "dir_eps_below": _dir(p=lambda v: at_eps(v, False), color=lambda c: c / np.sqrt(EPS)),
    "dir_1e-5": _dir(scale=1e-5, color=lambda c: c * 1e5),
    "dir_zero": _dir(scale=0.0),
    "dir_100": _dir(scale=100.0, color=lambda c: c / 60.0),
    "dir_nan": _dir(p=lambda v: _put(v, 0, NAN)),
    "dir_nan_inf_color": _dir(p=lambda v: _put(v, 2, NAN), color=lambda c: _set(c, 1, INF)),
    "dir_inf": _dir(p=lambda v: _put(v, 1, INF)),
    "dir_zero_nan_color": _dir(scale=0.0, color=lambda c: _set(c, 0, NAN)),
    # light colours, both kinds
    "dcol_inf": _color("d", lambda c: _set(c, 0, INF)),
    "dcol_nan": _color("d", lambda c: _set(c, 1, NAN)),
    "dcol_neg": _color("d", lambda c: _set(c, 2, -0.8)),
    "dcol_negzero": _color("d", lambda c: _set(_set(c, 0, -0.0), 1, -0.0)),
    "dcol_neginf": _color("d", lambda c: _set(c, 2, -INF)),
    "pcol_inf": _color("p", lambda c: _set(c, 0, INF)),
    "pcol_nan": _color("p", lambda c: _set(c, 1, NAN)),
    "pcol_neg": _color("p", lambda c: _set(c, 2, -60.0)),
    "pcol_negzero": _color("p", lambda c: _set(_set(c, 0, -0.0), 2, -0.0)),
    # albedo: one object, every object
    "alb_inf_one": _albedo((INF, None, None), False),
    "alb_nan_one": _albedo((None, NAN, None), False),
    "alb_neg_one": _albedo((None, None, -0.7), False),
    "alb_mixed_all": _albedo((INF, 0.5, -0.5), True),
    "alb_nan_all": _albedo((None, NAN, None), True),
    # both bits cleared on one light: short direction and a colour / an albedo that is not finite
    "dir_short_inf_color": _both(_dir(scale=1e-5, color=lambda c: c * 1e5), _color("d", lambda c: _set(c, 0, INF))),
    "dir_short_inf_albedo": _both(_dir(scale=1e-5, color=lambda c: c * 1e5), _albedo((INF, None, None), False)),
    # background
    "bg_neg": _bg((-0.25, 0.3, -1.5)),
    "bg_gt1": _bg((1.5, 0.3, 7.0)),
    "bg_negzero": _bg((-0.0, 0.3, -0.0)),
    "bg_nan": _bg((0.2, NAN, 0.4)),
    # reflection ratio (mirror scenes)
    "refl_nan": _refl(NAN),
    "refl_neg": _refl(-0.5),
}
POINT_TARGET = {n for n in ODDITIES if n.startswith("pcol_")}
# one per family for the supersampling and transport tests
FAMILIES = ["lean-first-dir_eps_below", "lean-last-dcol_inf", "gq-first-pcol_neg", "mirror-first-alb_mixed_all", "mirror-first-refl_nan",
            "lean-first-bg_neg", "gq-first-bg_negzero", "lean65-first-bg_nan", "gq-many-dir_short_inf_color"]


def _named():
    out = {}
    for cls in CLASSES:
        for i, odd in enumerate(ODDITIES):
            if odd.startswith("refl_") and cls != "mirror":
                continue
            if odd == "bg_nan" and cls == "cubic":       # (degree <= 2 only: the degree-3 bar is a tolerance)
                continue
            layout = "first" if (i + CLASSES.index(cls)) % 2 == 0 else "last"
            out[f"{cls}-{layout}-{odd}"] = (cls, layout, odd)
    for cls in ("lean", "lean65", "gq", "mirror"):       # one odd light among forty (lights_plain cleared by exactly one light)
        for odd in ("dir_eps_below", "dir_eps_above", "dcol_inf", "dir_short_inf_color", "pcol_nan", "dir_nan_inf_color"):
            out[f"{cls}-many-{odd}"] = (cls, "many", odd)
    for name in FAMILIES:
        cls, layout, odd = name.split("-")
        out[name] = (cls, layout, odd)
    return out


NAMED = _named()


def named(name):
    """(scene, twin, cameras): the twin is the scene without the oddity."""
    cls, layout, odd = NAMED[name]
    twin, cams, d, p = base(cls, layout, odd in POINT_TARGET)
    s = copy_scene(twin)
    ODDITIES[odd](s, d, p)
    return s, twin, cams


def scene_class(osc):
    """The kernel class of a scene, by the rules of rt_create: "lean" / "lean65" (unit spheres only, no mirror), "mirror" (unit
    spheres, some mirror), "gq" (degree <= 2 with a plane or general quadric), "cubic"."""
    co = np.asarray(osc.coefs, dtype=np.float64).reshape(-1, 20)
    if np.any(co[:, :10] != 0):
        return "cubic"
    unit_sq = np.all(co[:, 10:13] == 1.0, axis=1) & np.all(co[:, 13:16] == 0.0, axis=1)
    if not np.all(unit_sq):
        return "gq"
    if np.any(osc.reflection > np.float32(EPS)):
        return "mirror"
    return "lean" if len(co) <= 64 else "lean65"


# ---- the seeded generator ----------------------------------------------------------------------------------------------------
def _odd_color(rng, c, scale=1.0):
    c = np.array(c, dtype=np.float64)
    r = rng.random()
    k = int(rng.integers(0, 3))
    if r < 0.10:
        c[k] = INF if rng.random() < 0.7 else -INF
    elif r < 0.17:
        c[k] = NAN
    elif r < 0.27:
        c[k] = -float(rng.uniform(0.1, 1.0)) * scale
    elif r < 0.33:
        c[k] = -0.0
    return c


def _odd_dir(rng, d):
    """(direction, colour factor)"""
    d = unit(d)
    r = rng.random()
    if r < 0.08:
        return at_eps(d, bool(rng.integers(0, 2))), 1.0 / np.sqrt(EPS)
    if r < 0.15:
        return d * 1e-5, 1e5
    if r < 0.20:
        return d * 0.0, 1.0
    if r < 0.27:
        return d * 100.0, 1.0 / 60.0
    if r < 0.32:
        return _put(d, int(rng.integers(0, 3)), NAN), 1.0
    if r < 0.37:
        return _put(d, int(rng.integers(0, 3)), INF if rng.random() < 0.5 else -INF), 1.0
    return d, 1.0


def scene(seed):
    """(oracle scene, camera): even seeds spheres only (fuzz_spheres' ranges; every fourth seed more than 64 of them), odd seeds the
    mixed degree <= 2 classes of fuzz_parity (spheres, quadrics, planes, mirrors).  Each light direction, each light colour, each
    albedo, the reflection ratios and the background take an oddity with some probability."""
    rng = np.random.default_rng(770000 + seed)
    w, h = int(rng.integers(1, 161)), int(rng.integers(1, 121))
    bg = rng.uniform(0, 1, 3)
    r = rng.random()
    if r < 0.15:
        bg[int(rng.integers(0, 3))] = -float(rng.uniform(0, 2))
    elif r < 0.25:
        bg[int(rng.integers(0, 3))] = float(rng.uniform(1, 9))
    elif r < 0.35:
        bg[int(rng.integers(0, 3))] = -0.0
    elif r < 0.42:
        bg[int(rng.integers(0, 3))] = NAN
    s = O.Scene(w, h, float(rng.uniform(25, 95)), int(rng.integers(0, 4)), bg)
    spheres_only = seed % 2 == 0
    scale = float(10 ** rng.uniform(-1, 2))
    n_obj = (int(rng.integers(65, 90)) if seed % 4 == 0 else int(rng.integers(2, 40))) if spheres_only else int(rng.integers(2, 16))
    odd_albedo = rng.random() < 0.35
    for i in range(n_obj):
        kind = 0 if spheres_only else int(rng.integers(0, 4))
        refl = 0.0
        if not spheres_only and rng.random() < 0.3:
            refl = float(rng.uniform(0.1, 0.9))
            if rng.random() < 0.15:
                refl = NAN if rng.random() < 0.5 else -refl
        col = rng.uniform(0, 1, 3)
        if odd_albedo and rng.random() < 0.4:
            col = _odd_color(rng, col)
        if kind <= 1:
            c = rng.uniform([-12, -8, 4], [12, 8, 40]) * scale
            co = sphere(c, float(10 ** rng.uniform(-1.5, 1.0)) * scale)
        elif kind == 2:
            q = np.zeros(20)
            q[10:13] = rng.uniform(-1.5, 2.0, 3)
            if rng.random() < 0.5:
                q[13:16] = rng.uniform(-0.5, 0.5, 3)
            c = rng.uniform([-6, -4, 8], [6, 4, 25]) * scale
            q[16:19] = -2.0 * q[10:13] * c
            q[19] = float(np.dot(q[10:13], c * c) - rng.uniform(0.5, 6.0) * scale * scale)
            co = list(q)
        else:
            n = rng.normal(size=3)
            co = plane(rng.uniform([-5, -8, 0], [5, -3, 30]) * scale, unit(n) + np.array([0, 1.5, 0]))
        s.add_object(co, col, refl)
    for i in range(int(rng.integers(1, 10)) if seed % 9 else int(rng.integers(33, 48))):
        few = 1.0 if seed % 9 else 0.1
        if rng.random() < 0.6:
            d, f = _odd_dir(rng, rng.normal(size=3) + np.array([0, 1.2, 0]))
            col = rng.uniform(0, 1, 3) * float(rng.uniform(0, 1.5)) * f * few
            s.lights.append(stored_light(0, d, _odd_color(rng, col, f)))
        else:
            p = rng.uniform([-15, -10, -10], [15, 20, 40]) * scale
            inten = float(rng.uniform(1, 900)) * scale * scale * few
            s.lights.append(stored_light(1, p, _odd_color(rng, rng.uniform(0, 1, 3) * inten, inten)))
    cam = O.camera_matrix(tuple(rng.uniform(-3, 3, 3) * scale), float(rng.uniform(60, 120)), float(rng.uniform(-25, 25)))
    return s, cam


# ---- comparing and rendering (the GPU tests and main() below) ----------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    """The same bits (np.array_equal calls -0.0 and 0.0 equal and a NaN unequal to itself)."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def same_as_oracle(got, want):
    """The same bits, except that a NaN only has to be a NaN on both sides (the device and glibc spell NaN differently)."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    n = np.isnan(got)
    return bool(np.array_equal(n, np.isnan(want)) and np.array_equal(got[~n].view(np.uint32), want[~n].view(np.uint32)))


def n_diff(a, b):
    """Pixels whose bits differ."""
    return int((bits(a) != bits(b)).any(axis=-1).sum()) if a.shape == b.shape else -1


def render_desc(pkg, sc, cam=None, **kw):
    """test_gpu_parity.render_desc on bit patterns (frames here hold NaN channels): three frames from one context -- index order, then
    the launch order fed back by the frame before -- which must not differ."""
    r = pkg.Renderer(sc, device=0, **kw)
    try:
        r.update(cam)
        first = r.download().copy()
        r.update(cam)
        second = r.download().copy()
        r.update(cam)
        img = r.download()
    finally:
        r.cleanup_update()
    assert same(first, second) and same(first, img), "frame changed with the launch order"
    return img


# ---- for use outside pytest ----------------------------------------------------------------------------------------------------
def main():
    os.environ["MI355RT_LEAN"] = "always"
    import __graft_entry__ as graft
    pkg = graft.load_package()
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    bad = 0
    for seed in range(first, first + n):
        s, cam = scene(seed)
        want = s.render(cam=cam, nthreads=4)
        try:
            fr = {name: render_desc(pkg, desc(pkg, s), cam, flags=fl) for name, fl in
                  (("default", 0), ("nocull", pkg.RT_FLAG_NOCULL), ("simple", pkg.RT_FLAG_SIMPLE), ("nolean", pkg.RT_FLAG_NOLEAN))}
            ok = all(same(fr["default"], v) for v in fr.values()) and same_as_oracle(fr["default"][..., :3], want)
            detail = "  ".join(f"{k} {same(fr['default'], v)}" for k, v in fr.items()) + f"  vs-oracle {same_as_oracle(fr['default'][..., :3], want)}"
        except AssertionError as e:
            ok, detail = False, str(e)
        if not ok:
            bad += 1
            print(f"seed {seed}: MISMATCH  {detail}  ({s.width}x{s.height}, {len(s.objects)} objects, {len(s.lights)} lights, class {scene_class(s)}, "
                  f"flags {flags(s)[2:]})", flush=True)
        if (seed - first) % 50 == 49:
            print(f"... {seed - first + 1} scenes, {bad} mismatches", flush=True)
    print(f"raw_desc_scenes: {n} scenes, {bad} mismatches")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
