"""Fields of many small degree-3 objects, and the oracle-side conditions that go with them (tests/test_cubic_chunks_host.py,
tests/test_cubic_chunks_gpu.py) -- test infrastructure.  The streamed kernels walk the degree-3 class table as an index list staged
through LDS 64 entries at a time (csrc/rt_stream.hpp: sq_tables, the HAS_CUBIC block); the staged ones walk it in a plain loop
(csrc/rt_rayquery.hpp: rq_tables; csrc/rt_wavefront.hip: S.cub[j]).  These scenes take both past 64 entries.

A cubic surface is unbounded, so a field of small ones needs care.  Each object here is a bent ellipsoid F(x - c) = 0, translated
EXACTLY (the polynomial is expanded), with

    F(u) = ax ux^2 + ay uy^2 + az uz^2 - 1 - (b1 uz^3 + b2 ux^2 uz + b3 uy^2 uz),    a = 1 / (r U(0.7, 1.3))^2,  b = U(0.006, 0.02) / r^3,

all three cubic terms NEGATIVE.  With these signs F > 0 at the camera (the origin lies outside every surface: uz = -cz < 0 makes the
cubic part positive there), the body around c is compact, and the far sheet, where the cubic part overtakes the quadratic one,
lies at uz of the order a / b = 25 .. 50 r BEHIND the body: the sheets form a backdrop that catches shadows and never hide a body.
With random signs, or a bend of 0.15, the sheets fill the frame and two or three objects own every pixel.

The conditions (Conditions) are evaluated on the oracle's own functions: tests/tools/cubic_guard_lab.cpp lists every degree-3 test
of the oracle's frame (each primary ray, each shadow ray of a primary hit, each first bounce of a mirror hit, against EVERY degree-3
object: no early exit), and the oracle answers each."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import query_table_scenes as Q  # noqa: E402
import raw_desc_scenes as R  # noqa: E402
import stream_scenes as S  # noqa: E402
from stream_scenes import CHUNK, FOV, K_EPS, K_MAX_T, O  # noqa: E402

SEED = 1                     # the seed under which the conditions of tests/test_cubic_chunks_host.py hold for every scene of SCENES
PX = 5.0                     # a body's diameter in pixels at its own depth
RT_CUB_AT_MAX = 4            # include/mi355rt.h: the degree-3 objects whose data at the frame's origin the host forms
# the scenes of tests/test_cubic_chunks_gpu.py by name: the arguments of cubic_field after the seed
SCENES = {
    "64": dict(n=64), "65": dict(n=65), "129": dict(n=129),
    "65 quadric": dict(n=65, with_quadric=True), "65 37x21": dict(n=65, w=37, h=21),
    "65 spheres": dict(n=65, spheres=65), "65 spheres quadric": dict(n=65, spheres=65, with_quadric=True), "129 spheres": dict(n=129, spheres=65),
}

# the 20 coefficients as exponents of (x, y, z), in the order of oracle/rt_oracle.h (ORC_X3 .. ORC_C)
MONOMIALS = ((3, 0, 0), (0, 3, 0), (0, 0, 3), (2, 1, 0), (1, 2, 0), (2, 0, 1), (1, 0, 2), (0, 2, 1), (0, 1, 2), (1, 1, 1),
             (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))
_AT = {m: i for i, m in enumerate(MONOMIALS)}
_BINOM = ((1,), (1, 1), (1, 2, 1), (1, 3, 3, 1))


def translated(q, c):
    """The coefficients of F(x - c) for the coefficients q of F: every monomial expanded by the binomial theorem, term by term."""
    out = np.zeros(20)
    for (ex, ey, ez), v in zip(MONOMIALS, q):
        if v == 0.0:
            continue
        for i in range(ex + 1):
            for j in range(ey + 1):
                for k in range(ez + 1):
                    f = _BINOM[ex][i] * _BINOM[ey][j] * _BINOM[ez][k]
                    out[_AT[(i, j, k)]] += v * f * (-c[0]) ** (ex - i) * (-c[1]) ** (ey - j) * (-c[2]) ** (ez - k)
    return out


def bent_ellipsoid(c, r, semi, bend):
    """F(x - c) of the module's docstring: semi = the three factors on r, bend = the three magnitudes times r^3."""
    q = np.zeros(20)
    q[_AT[(2, 0, 0)]], q[_AT[(0, 2, 0)]], q[_AT[(0, 0, 2)]] = 1.0 / (r * np.asarray(semi)) ** 2
    q[_AT[(0, 0, 3)]], q[_AT[(2, 0, 1)]], q[_AT[(0, 2, 1)]] = -np.asarray(bend) / r ** 3
    q[_AT[(0, 0, 0)]] = -1.0
    return translated(q, c)


def cubic_field(n, seed, w=64, h=48, depth=2, spheres=0, with_quadric=False):
    """The oracle scene of n bent ellipsoids placed as the fields of stream_scenes.field (z in 20 .. 30, spread over the view of the
    50 degree camera at the origin), each PX pixels across at its depth, every third a mirror of ratio 0.5; the two lights of
    stream_scenes.field.  spheres: that many spheres of stream_scenes.field's mirrored field (S.FIELD_SEED) appended, so that the
    unit-sphere table has chunks to cull.  with_quadric: one reflecting ellipsoid with cross terms appended (the <1, 1> instantiations)."""
    rng = np.random.default_rng(seed)
    osc = O.Scene(w, h, FOV, depth, (0.05, 0.1, 0.2))
    tan = np.tan(np.radians(FOV / 2))
    osc.bodies = []           # (centre, r) per degree-3 object, for aimed_rays
    for i in range(n):
        z = rng.uniform(20.0, 30.0)
        half_h, half_w = z * tan, z * tan * w / h
        c = np.array([rng.uniform(-half_w, half_w) * 0.96, rng.uniform(-half_h, half_h) * 0.96, z])
        r = 0.5 * PX * 2.0 * z * tan / h
        col = rng.uniform(0.2, 1.0, 3)
        osc.bodies.append((c, r))
        osc.add_object(bent_ellipsoid(c, r, rng.uniform(0.7, 1.3, 3), rng.uniform(0.006, 0.02, 3)), col, 0.5 if i % 3 == 0 else 0.0)
    if spheres:
        import __graft_entry__ as graft
        pkg = graft.load_package()
        for o in S.oracle_of(pkg, S.field(pkg, spheres, S.FIELD_SEED, w=w, h=h, mirrors=True, depth=depth)).objects:
            osc.add_object(list(o.c), list(o.color), o.reflection_ratio)
    if with_quadric:
        osc.add_object(S.ellipsoid(np.array([3.0, 2.0, 18.0]), np.array([1.5, 0.8, 1.1]), np.array([0.3, -0.2, 0.1])), (0.9, 0.6, 0.3), 0.3)
    L = O.lib()
    for kind, v, col, inten in (("directional", [0.2, -1.0, 0.6], (1.0, 0.95, 0.9), 1.2), ("spherical", [4.0, 12.0, 2.0], (0.8, 0.9, 1.0), 500.0)):
        light = O.OrcLight()
        (L.orc_light_directional if kind == "directional" else L.orc_light_spherical)(inten, O._d3(v), O._f3(col), light)
        osc.lights.append(light)
    return osc


def scene(name, seed=SEED):
    return cubic_field(seed=seed, **SCENES[name])


def without(osc, drop):
    """The scene without the objects `drop`."""
    t = R.copy_scene(osc)
    t.objects = [o for k, o in enumerate(t.objects) if k not in set(drop)]
    return t


def aimed_rays(osc, seed=31):
    """One ray per degree-3 body (rays_ref.RAY_DTYPE, in table order): from 1.5 .. 3 times r off the body's centre in a random direction, at
    that centre; the direction's length is 0.5 .. 2."""
    import rays_ref
    rng = np.random.default_rng(seed)
    table = Q.tables(osc.coefs)["cubic"]
    rays = np.zeros(len(table), dtype=rays_ref.RAY_DTYPE)
    for i, k in enumerate(table):
        c, r = osc.bodies[k]
        v = rng.normal(size=3)
        o = c + r * rng.uniform(1.5, 3.0) * v / np.linalg.norm(v)
        rays["o"][i], rays["d"][i] = o, (c - o) / np.linalg.norm(c - o) * rng.uniform(0.5, 2.0)
    return rays


class Conditions:
    """What the oracle's frame of a cubic_field scene shows, by table position of the degree-3 table (Q.tables(coefs)["cubic"]).

    owner [h, w]: the table position of the degree-3 object nearest along each pixel's primary ray, -1 where none is hit.  Where the
        scene holds other classes too, such a pixel may be owned by one of them instead: `owner` is then a superset of what the
        degree-3 objects own, and owned_for_certain(x, y) asks the reference's full nearest-hit loop (S.Owners).
    shadow_only_beyond(lo): the (x, y, light) of primary hits whose shadow ray is blocked by degree-3 objects at positions >= lo and
        by no degree-3 object below.
    bounce_hits: per mirror hit (x, y) the position of the degree-3 object its first bounce meets first, -1 where none."""

    def __init__(self, osc):
        import cubic_device_lab as D
        self.osc = osc
        self.table = Q.tables(osc.coefs)["cubic"]
        self.pos = {k: at for at, k in enumerate(self.table)}
        rays, where = D.enumerate_rays(osc)
        t, _, _ = D.oracle_rays(osc, rays)
        pos = np.vectorize(self.pos.get, otypes=[np.int64])(rays["obj"])
        n, h, w = len(self.table), osc.height, osc.width
        self.n = n
        kind, x, y = where["kind"], where["x"], where["y"]
        # primary: the nearest-hit rule of the reference on the degree-3 objects
        m = kind == 0
        tp = np.full((h, w, n), np.inf)
        ok = m & (t >= K_EPS) & (t < K_MAX_T)
        tp[y[ok], x[ok], pos[ok]] = t[ok]
        self.t_primary = tp.min(axis=2)
        self.owner = np.where(np.isfinite(self.t_primary), tp.argmin(axis=2), -1)
        # shadow: the reference's rule t > K_EPS and t < max_t, per (pixel, light) and position
        m = kind == 1
        nl = len(osc.lights)
        self.blocks = np.zeros((h, w, nl, n), dtype=bool)
        self.has_hit = np.zeros((h, w), dtype=bool)
        self.has_hit[y[m], x[m]] = True
        b = m & (t > K_EPS) & (t < rays["max_t"])
        self.blocks[y[b], x[b], where["light"][b], pos[b]] = True
        # first bounces
        m = kind == 2
        tb = np.full((h, w, n), np.inf)
        ok = m & (t >= K_EPS) & (t < K_MAX_T)
        tb[y[ok], x[ok], pos[ok]] = t[ok]
        self.bounced = np.zeros((h, w), dtype=bool)
        self.bounced[y[m], x[m]] = True
        self.t_bounce = tb.min(axis=2)
        self.bounce_hits = np.where(np.isfinite(self.t_bounce), tb.argmin(axis=2), -1)
        self.others = [k for k in range(len(osc.objects)) if k not in self.pos]
        self._owners = None

    def owned_for_certain(self, x, y):
        """The table position of the degree-3 object that owns pixel (x, y) by the reference's loop over ALL objects, or -1."""
        if not self.others:
            return int(self.owner[y, x])
        if self._owners is None:
            self._owners = S.Owners(self.osc)
        return self.pos.get(self._owners.owner(x, y), -1)

    def some_pixel_owned_in(self, lo, hi, tries=12):
        """A pixel (x, y) a degree-3 object at a position of lo .. hi - 1 owns, or None."""
        cand = np.argwhere((self.owner >= lo) & (self.owner < hi))
        for y, x in cand[:: max(1, len(cand) // tries)].tolist():
            if lo <= self.owned_for_certain(x, y) < hi:
                return x, y
        return None

    def shadow_only_beyond(self, lo):
        """[(x, y, light)]: blocked by some degree-3 object at a position >= lo, by none below -- and by no object of another class
        (rays_ref.occluded on those alone, for the few candidates tried)."""
        import rays_ref
        m = self.blocks[..., lo:].any(axis=-1) & ~self.blocks[..., :lo].any(axis=-1)
        cand = [tuple(int(v) for v in (x, y, l)) for y, x, l in np.argwhere(m)]
        if not self.others or not cand:
            return cand
        rest = without(self.osc, self.table)
        rest.lights = self.osc.lights
        own = S.Owners(self.osc) if self._owners is None else self._owners
        self._owners = own
        out = []
        for x, y, l in cand[:12]:
            # the shadow ray of this pixel's hit, as the reference forms it
            k = own.owner(x, y)
            ray = rays_ref.make_rays(own.o, own.dirs[y, x])
            n64 = np.zeros((1, 3))
            hit = rays_ref.closest(self.osc, ray, n64)
            assert hit["object"][0] == k
            srays, tmax, _, light = rays_ref.shadow_rays(self.osc, hit, n64)
            if not rays_ref.occluded(rest, srays[light == l], tmax[light == l])[0]:
                out.append((x, y, l))
        return out

    def bounce_met_beyond(self, lo):
        """[(x, y)] of mirror hits whose first bounce has its nearest hit on a degree-3 object at a position >= lo -- among ALL objects:
        where the scene holds other classes, paths_ref.paths confirms the few candidates tried."""
        import paths_ref
        import rays_ref
        cand = [(int(x), int(y)) for y, x in np.argwhere(self.bounced & (self.bounce_hits >= lo))]
        if not self.others or not cand:
            return cand
        cand = cand[:: max(1, len(cand) // 12)]
        dirs = rays_ref.primary_rays(self.osc).reshape(self.osc.height, self.osc.width)
        seg, _, _ = paths_ref.paths(self.osc, np.array([dirs[y, x] for x, y in cand]))
        return [xy for xy, k in zip(cand, seg[1]["object"].tolist()) if self.pos.get(k, -1) >= lo]


def changed_pixels(osc, drop_positions):
    """[h, w] bool: the pixels of the oracle's frame that change when the degree-3 objects at `drop_positions` are removed."""
    table = Q.tables(osc.coefs)["cubic"]
    a = osc.render(nthreads=8)
    b = without(osc, [table[p] for p in drop_positions]).render(nthreads=8)
    return (a.view(np.uint32) != b.view(np.uint32)).any(axis=-1)
