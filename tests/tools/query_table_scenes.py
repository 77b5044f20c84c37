"""Scenes, aimed rays and oracle-side conditions of the query kernels' table tests (tests/test_query_tables_host.py and
tests/test_query_tables_gpu.py) -- test infrastructure.  The seven query entry points (rt_render_gbuffer, rt_pick, rt_object_extents,
rt_trace_rays, rt_occluded_rays, rt_shade_rays, rt_trace_paths) copy the class tables into LDS and walk them 64 entries at a time
(csrc/rt_rayquery.hpp: rq_tables, for pixels and for rays), so the scenes are the fields of tests/tools/stream_scenes.py with
a count next to a multiple of 64 or next to the 160 KiB limit, and the rays are AIMED: one per chosen table entry, so that a test reaches
that entry on purpose, which the primary rays of a small frame cannot.

The two test files use the cases, seeds, target lists, rays and rows of this module and nothing else: they move together."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gbuffer_ref  # noqa: E402
import rays_ref  # noqa: E402
import stream_scenes as S  # noqa: E402
from stream_scenes import CHUNK, K_EPS, K_MAX_T, O  # noqa: E402

SMALL = [("sphere", 64), ("sphere", 65), ("sphere", 129), ("sphere", 193), ("quadric", 64), ("quadric", 65), ("quadric", 129), ("quadric", 193),
         ("planes", 65)]
LARGE = ["one below the frame limit", "streamed by size", "large mixed", "at the query limit"]
SIZES = ((64, 48), (37, 21))          # the frames of the small cases: the second has partial tiles and partial 8 x 8 blocks
DEPTHS = (0, 1, 4)                    # max_reflections of the small cases
ROWS = (0, 7, 13, 20, 21, 33, 40, 47)   # the rows of the 64 x 48 frame a large case's planes are composed for (20 and 21 make a rectangle)
RECTS_SMALL = {(64, 48): (5, 9, 50, 40), (37, 21): (3, 2, 30, 17)}
RECTS_LARGE = ((0, 20, 63, 21), (5, 40, 60, 40))   # (inside ROWS)
QUERY_LIMIT_SPHERES = S.LDS_LIMIT // 64            # 2 560: 64 table bytes per sphere (rt_scene_dev.h: UsEntry)
AIM_SEED, TMAX_SEED, PICK_SEED, PLANES_SEED = 31, 32, 33, 28
N_RANDOM_TARGETS = 200


def small_scene(pkg, case, w=64, h=48, depth=1):
    """One class, a count next to a multiple of 64, every third object (every fourth plane) a mirror."""
    kind, n = case
    if kind == "planes":
        # (PLANES_SEED: the last plane owns pixels of both frames; the mirrors are those of depth 1 at every depth)
        return S.planes(pkg, n, PLANES_SEED, w=w, h=h, depth=1).set_max_reflections(depth)
    return S.field(pkg, n, S.FIELD_SEED, kind, w=w, h=h, mirrors=True, depth=depth)


def large_scene(pkg, name):
    """The sizes a streamed context allows (64 x 48): the largest scene the wavefront frame kernel takes, the first one beyond it plus the
    large last sphere, the mixed scene whose three tables come to 160 096 bytes, and the sphere field whose table is exactly 160 KiB."""
    n = S.first_count_beyond_lds(pkg)
    if name == LARGE[0]:
        return S.field(pkg, n - 1, S.LARGE_SEED)
    if name == LARGE[1]:
        return S.field(pkg, n, S.LARGE_SEED, big_last=True)
    if name == LARGE[2]:
        return S.mixed_large(pkg, 2000, S.MIXED_SEED)
    assert name == LARGE[3]
    return S.field(pkg, QUERY_LIMIT_SPHERES, S.LARGE_SEED, mirrors=True, depth=2)


def moved_coefs(sc):
    """Every sphere of a field moved by up to 0.7 with its radius kept (tests/test_stream_gpu.py: test_set_scene_moves_the_large_field)."""
    coefs = sc.arrays()["coefs"].copy()
    c = -0.5 * coefs[:, 16:19]
    r2 = (c * c).sum(axis=1) - coefs[:, 19]
    c2 = c + np.random.default_rng(5).uniform(-0.7, 0.7, c.shape)
    coefs[:, 16:19] = -2.0 * c2
    coefs[:, 19] = (c2 * c2).sum(axis=1) - r2
    return coefs


def with_coefs(pkg, sc, coefs):
    a = sc.arrays()
    return pkg.desc_from_arrays(a["width"], a["height"], a["vertical_fov"], a["bg_color"], a["max_reflections"], coefs, a["reflection"], a["albedo"],
                                a["light_is_spherical"], a["light_p"], a["light_color"])


def oracle_with_coefs(osc, coefs):
    o = O.Scene(osc.width, osc.height, 0.0, osc.max_reflections, osc.bg_color)
    o.vertical_fov = osc.vertical_fov
    for k, ob in enumerate(osc.objects):
        o.add_object(coefs[k], list(ob.color), ob.reflection_ratio)
    o.lights = list(osc.lights)
    return o


# ---- the class tables ---------------------------------------------------------------------------------------------------------------------
def tables(coefs):
    """The objects of each class table in table order (= object order): dict(sphere, quadric, plane, cubic) of index lists, by the rule of
    tests/test_stream_host.py::test_large_mixed_scene_shows_every_chunk_of_both_tables with degree 3 first."""
    out = dict(sphere=[], quadric=[], plane=[], cubic=[])
    for k, q in enumerate(np.asarray(coefs)):
        if q[:10].any():
            out["cubic"].append(k)
        elif not q[10:16].any():
            out["plane"].append(k)
        elif (q[10:13] == 1.0).all() and not q[13:16].any():
            out["sphere"].append(k)
        else:
            out["quadric"].append(k)
    return out


def chunks(table):
    return [table[lo:lo + CHUNK] for lo in range(0, len(table), CHUNK)]


def position(coefs):
    """Per object (class, chunk of its class table)."""
    pos = {}
    for name, table in tables(coefs).items():
        for at, k in enumerate(table):
            pos[k] = (name, at // CHUNK)
    return pos


def boundary_targets(coefs):
    """The first and the last entry of every 64-entry chunk of every table."""
    out = []
    for table in tables(coefs).values():
        for ch in chunks(table):
            out += [ch[0], ch[-1]]
    return sorted(set(out))


def targets_of(coefs, small):
    """Small scenes: every object.  Large scenes: the chunk boundaries plus about 200 random objects, as many from every chunk."""
    if small:
        return list(range(len(coefs)))
    rng = np.random.default_rng(PICK_SEED)
    all_chunks = [ch for table in tables(coefs).values() for ch in chunks(table)]
    per = max(1, round(N_RANDOM_TARGETS / len(all_chunks)))
    extra = [k for ch in all_chunks for k in rng.choice(ch, min(per, len(ch)), replace=False).tolist()]
    return sorted(set(boundary_targets(coefs)) | set(extra))


# ---- aimed rays ---------------------------------------------------------------------------------------------------------------------------
def centre_and_radius(q):
    """Of a sphere, an ellipsoid or a degree-3 surface that is mostly one: where the gradient of the quadratic part vanishes, and its
    largest semi-axis.  None for a plane."""
    A = np.array([[q[10], q[13] / 2, q[14] / 2], [q[13] / 2, q[11], q[15] / 2], [q[14] / 2, q[15] / 2, q[12]]])
    if not A.any():
        return None
    c = np.linalg.solve(2.0 * A, -q[16:19])
    f = float(c @ A @ c + q[16:19] @ c + q[19])   # the quadratic part at its centre: (p - c)^T A (p - c) = -f
    return c, float(np.sqrt(-f / np.linalg.eigvalsh(A).min()))


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def aimed_rays(osc, targets, seed, keep=()):
    """One ray per target object (RAY_DTYPE, in the order of `targets`): it starts 0.3 to 1.5 radii above the surface (radii above
    0.8 count as 0.8), in a random direction from the object's centre, and points at the centre; the direction's length is 0.5 .. 2.  A
    plane's ray starts 0.02 .. 0.2 beside a point of the plane near the view and points at that point.  A degree-3 surface has no centre:
    its ray points at the hit point of a pixel it owns (gbuffer_ref.compose of the scene's own frame), from 0.3 .. 1 away on the side of
    the normal there.  About one ray in twenty is replaced by an odd kind of
    tests/test_rays_gpu.py::arbitrary_rays (zero direction, a NaN or +-inf component, a component beyond 1e100, a NaN origin), so that
    the plain path runs in the same waves as the table path -- never a ray whose target is in `keep`."""
    rng = np.random.default_rng(seed)
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, O.NCOEF)
    rays = np.zeros(len(targets), dtype=rays_ref.RAY_DTYPE)
    keep = set(keep)
    seen = gbuffer_ref.compose(osc) if coefs[:, :10].any() else None
    for i, k in enumerate(targets):
        q = coefs[k]
        cr = centre_and_radius(q)
        mine = np.argwhere(seen["object"] == k) if (seen is not None and q[:10].any()) else []
        if len(mine):
            y, x = mine[int(rng.integers(len(mine)))]
            p, nv = seen["point"][y, x], seen["normal"][y, x, :3].astype(np.float64)
            side = _unit(rng)
            side = side if side @ nv > 0 else -side
            o = p + rng.uniform(0.3, 1.0) * (side + nv) / np.linalg.norm(side + nv)
            d = p - o
        elif cr is None:
            nv = q[16:19] / np.linalg.norm(q[16:19])
            t1 = np.cross(nv, [1.0, 0.0, 0.0])
            t1 /= np.linalg.norm(t1)
            p = -q[19] / np.linalg.norm(q[16:19]) * nv + rng.uniform(-2, 2) * t1 + rng.uniform(-2, 2) * np.cross(nv, t1)
            o = p + rng.choice([-1.0, 1.0]) * rng.uniform(0.02, 0.2) * nv + rng.uniform(-0.01, 0.01, 3)
            d = p - o
        else:
            c, r = cr
            o = c + (r + rng.uniform(0.3, 1.5) * min(r, 0.8)) * _unit(rng)
            d = c - o
        d = d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
        odd = rng.random() < 0.05
        which = int(rng.integers(5))
        at, sign = int(rng.integers(3)), float(rng.choice([-1.0, 1.0]))
        if odd and k not in keep:
            if which == 0:
                d = np.zeros(3)
            elif which == 1:
                d[at] = np.nan
            elif which == 2:
                d[at] = np.inf * sign
            elif which == 3:
                d[at] = 1e120 * sign
            else:
                o = o.copy()
                o[at] = np.nan
        rays["o"][i], rays["d"][i] = o, d
    return rays


def aimed_t_max(osc, rays, targets, seed, keep=()):
    """t_max per aimed ray: about half K_MAX_T, the rest 0.9 .. 1.1 times the ray's own root on its target (just short of it to just beyond
    it), one in forty NaN and one in forty +inf.  A ray whose target is in `keep` ends 1.01 .. 1.1 times beyond its target, so that the
    target itself can be what blocks it."""
    rng = np.random.default_rng(seed)
    L, dp = O.lib(), C.POINTER(C.c_double)
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, O.NCOEF)
    out = np.full(len(rays), K_MAX_T)
    for i, k in enumerate(targets):
        o, d = np.ascontiguousarray(rays["o"][i]), np.ascontiguousarray(rays["d"][i])
        t = L.orc_intersect_ray(coefs[k].ctypes.data_as(dp), o.ctypes.data_as(dp), d.ctypes.data_as(dp))
        u, f, g = rng.random(), rng.uniform(0.9, 1.1), rng.uniform(1.01, 1.1)
        if k in keep:
            out[i] = (t if t > 0.0 else 1.0) * g
        elif u < 0.025:
            out[i] = np.nan
        elif u < 0.05:
            out[i] = np.inf
        elif u < 0.5:
            out[i] = (t if t > 0.0 else 1.0) * f
    return out


def lowest_blocker(osc, rays, t_max=None):
    """Per ray the lowest-index object the reference's shadow loop stops at (rays_ref.occluded's loop), or -1."""
    L, dp = O.lib(), C.POINTER(C.c_double)
    coefs, cptr = rays_ref._coef_ptrs(osc)
    tm = np.full(len(rays), K_MAX_T) if t_max is None else np.asarray(t_max, dtype=np.float64)
    out = np.full(len(rays), -1, dtype=np.int64)
    o, d = np.zeros(3), np.zeros(3)
    op, dptr = o.ctypes.data_as(dp), d.ctypes.data_as(dp)
    for i in range(len(rays)):
        o[:], d[:] = rays["o"][i], rays["d"][i]
        lim = float(tm[i])
        for k, cp in enumerate(cptr):
            t = L.orc_intersect_ray(cp, op, dptr)
            if t > K_EPS and t < lim:
                out[i] = k
                break
    return out


class Case:
    """What both test files need of one scene: the product scene, the oracle's, the targets, the aimed rays and their t_max."""

    def __init__(self, sc, osc, small, odd_kinds=True):
        self.sc, self.osc = sc, osc
        self.coefs = np.ascontiguousarray(self.osc.coefs, dtype=np.float64).reshape(-1, O.NCOEF)
        self.targets = targets_of(self.coefs, small)
        self.keep = boundary_targets(self.coefs)
        self.rays = aimed_rays(self.osc, self.targets, AIM_SEED, self.keep if odd_kinds else self.targets)
        self.t_max = aimed_t_max(self.osc, self.rays, self.targets, TMAX_SEED, set(self.keep))

    def at_depth(self, depth):
        return self.osc.with_size(self.osc.width, self.osc.height, depth)


def small_case(pkg, case, w=64, h=48):
    sc = small_scene(pkg, case, w, h)
    return Case(sc, S.oracle_of(pkg, sc), True)


def large_case(pkg, name):
    sc = large_scene(pkg, name)
    return Case(sc, S.oracle_of(pkg, sc), False)


def moved_case(pkg):
    """LARGE[1] after every sphere moved: the aimed rays are formed for the moved scene."""
    sc = large_scene(pkg, LARGE[1])
    coefs = moved_coefs(sc)
    return sc, coefs, Case(with_coefs(pkg, sc, coefs), oracle_with_coefs(S.oracle_of(pkg, sc), coefs), False)


def cubic_case(pkg):
    """Six degree-3 objects (tests/test_cubic_gpu.py: many_cubic_objects_and_mirrors) at 64 x 48: two of them beyond RT_CUB_AT_MAX = 4.
    No odd kinds among its aimed rays: the bars of the degree-3 query tests are stated for rays the class tables answer."""
    from test_cubic_gpu import many_cubic_objects_and_mirrors
    sc = many_cubic_objects_and_mirrors(pkg).set_size(64, 48)
    return Case(sc, S.oracle_of(pkg, sc), True, odd_kinds=False)
