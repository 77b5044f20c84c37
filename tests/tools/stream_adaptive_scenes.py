"""Scenes, cases and oracle-side conditions of the streamed adaptive passes' tests (tests/test_stream_adaptive_host.py,
tests/test_stream_adaptive_gpu.py; RT_FLAG_STREAM_ADAPTIVE, csrc/rt_stream_adaptive.hip) -- test infrastructure.
One list of cases for both files: the GPU test renders them, the host test asserts on the CPU oracle alone that they can fail (a
refined set that is neither empty nor everything, samples that go through the first and the last chunk of a table, partly filled
waves, pixels refined because of a halo row, geometric edges, bouncing samples).  Scenes are named by hashable keys:
  ("field", kind, n, w, h, mirrors, depth, px)   stream_scenes.field with FIELD_SEED
  ("planes", n, w, h, depth)                     stream_scenes.planes
  ("mixed", n, w, h)                             stream_scenes.mixed_large (depth 2)
  ("large", n, w, h)                             stream_scenes.field of n spheres with LARGE_SEED and the large sphere appended last
  ("random", ...)                                the keys of tests/test_ssaa_adaptive_fuzz_gpu.py::build"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import gbuffer_ref  # noqa: E402
import query_table_scenes as Q  # noqa: E402
import ssaa_adaptive_ref as ada  # noqa: E402
import ssaa_geometry_ref as geo  # noqa: E402
import stream_scenes as S  # noqa: E402

F32, U8 = 0, 1
INF = float("inf")
TAU = 1.0 / 32.0
TAUS = (-1.0, 0.0, TAU, INF)
FIELD_SEED = S.FIELD_SEED   # the seeds under which the conditions of tests/test_stream_adaptive_host.py hold
MIXED_SEED = S.MIXED_SEED
PLANES_SEED = 28   # a seed under which the last plane (the single entry of the second chunk) owns samples of refined pixels

# 1. forced, chunk boundaries: the last chunk holds 1, 63, 64 entries or a single one behind one or two full chunks; 37 x 21 has partial
# tiles.  Mirrors at depths 0, 1 and 4.
FORCED = [("field", "sphere", 1, 64, 48, False, 0, 2.6), ("field", "sphere", 63, 64, 48, True, 1, 2.6), ("field", "sphere", 64, 64, 48, True, 4, 2.6),
          ("field", "sphere", 65, 64, 48, True, 0, 2.6), ("field", "sphere", 129, 64, 48, True, 1, 2.6),
          ("field", "sphere", 1, 37, 21, False, 0, 2.6), ("field", "sphere", 63, 37, 21, True, 4, 2.6), ("field", "sphere", 64, 37, 21, True, 0, 2.6),
          ("field", "sphere", 65, 37, 21, True, 1, 2.6), ("field", "sphere", 129, 37, 21, True, 4, 2.6),
          ("field", "quadric", 65, 64, 48, True, 4, 2.6), ("planes", 65, 64, 48, 1), ("mixed", 130, 64, 48)]
# 2. bands: (scene, world, band rows, k, format); 37 rows are no multiple of world x band, 37 columns no multiple of 64
BANDS = [(("field", "sphere", 65, 37, 37, True, 1, 2.6), 3, 5, 2, F32), (("field", "sphere", 65, 37, 37, True, 1, 2.6), 2, 1, 4, U8)]
# 3. geometry: larger spheres, so that a sphere has interior pixels whose normals turn
GEOMETRY = ("field", "sphere", 65, 64, 48, True, 1, 8.0)
GEO_COSES = (-INF, 0.9)
GEO_TAUS = (TAU, INF)
GEO_LAYOUTS = ((1, 0, 8), (3, 1, 8))   # (world, rank, band rows)
# 4. beyond each limit, without RT_FLAG_STREAM
BEYOND_LIST = ("random", 9312, 568, 3, True, False, 24, 16, 9)   # fuzz case 12 (567 spheres and the floor) plus one sphere: 569 objects
GEO_SPHERES = 160 * 1024 // 64 + 2


def beyond_wavefront(pkg):
    return ("large", S.first_count_beyond_lds(pkg) - 1, 64, 48)   # first_count_beyond_lds spheres, the large one included


BEYOND_GBUFFER = ("large", GEO_SPHERES - 1, 37, 21)


def _pkg():
    import __graft_entry__ as graft
    return graft.load_package()


def scene(pkg, key):
    """(scene, camera)"""
    kind = key[0]
    if kind == "field":
        _, cls, n, w, h, mirrors, depth, px = key
        return S.field(pkg, n, FIELD_SEED, cls, w=w, h=h, mirrors=mirrors, depth=depth, px=px), None
    if kind == "planes":
        return S.planes(pkg, key[1], PLANES_SEED, w=key[2], h=key[3], depth=key[4]), None
    if kind == "mixed":
        return S.mixed_large(pkg, key[1], MIXED_SEED, w=key[2], h=key[3]), None
    if kind == "large":
        return S.field(pkg, key[1], S.LARGE_SEED, w=key[2], h=key[3], big_last=True), None
    from test_ssaa_adaptive_fuzz_gpu import build
    sc, _, cam = build(key)
    return sc, cam


@functools.lru_cache(maxsize=None)
def oracle_scene(key):
    pkg = _pkg()
    sc, cam = scene(pkg, key)
    return S.oracle_of(pkg, sc), cam


@functools.lru_cache(maxsize=None)
def frame(key, k=1):
    """The oracle's frame of scene `key` at k times its size."""
    osc, cam = oracle_scene(key)
    return osc.with_size(k * osc.width, k * osc.height).render(cam=cam, nthreads=8)


@functools.lru_cache(maxsize=None)
def planes(key):
    """The oracle's primary-hit planes (object, normal) of scene `key`."""
    osc, cam = oracle_scene(key)
    g = gbuffer_ref.compose(osc, cam)
    return g["object"], g["normal"]


def band_bounds(h, world, rank, band):
    """[(first global row, rows)] of the bands of `rank`."""
    out = []
    for g0 in range(rank * band, h, world * band):
        out.append((g0, min(band, h - g0)))
    return out


def banded_mask(p, tau, world, rank, band, obj=None, nrm=None, min_cos=None, halo=True):
    """The refine mask of a rank's rows, band by band with the rows just outside each band (halo = False: without them, as if the
    image ended at every band edge) -> (global rows, bool [rows, W])."""
    h = p.shape[0]
    rows, parts = [], []
    for g0, n in band_bounds(h, world, rank, band):
        lo, hi = g0 - 1, g0 + n
        ch = (p[lo] if (halo and lo >= 0) else None, p[hi] if (halo and hi < h) else None)
        m = ada.refine_mask(p[g0:g0 + n], tau, ch)
        if obj is not None:
            gh = ((obj[lo], nrm[lo]) if (halo and lo >= 0) else None, (obj[hi], nrm[hi]) if (halo and hi < h) else None)
            m = m | geo.geo_mask(obj[g0:g0 + n], nrm[g0:g0 + n], min_cos, gh)
        rows += list(range(g0, g0 + n))
        parts.append(m)
    if not rows:
        return np.zeros(0, dtype=np.int64), np.zeros((0, p.shape[1]), dtype=bool)
    return np.asarray(rows), np.concatenate(parts, axis=0)


class SampleOwners:
    """Who owns sample (X, Y) of the k-times finer grid of scene `key`: the reference's nearest-hit loop, evaluated only where asked."""

    def __init__(self, key, k):
        osc, cam = oracle_scene(key)
        self.k, self.osc = k, osc
        self.own = S.Owners(osc.with_size(k * osc.width, k * osc.height), cam)
        self.pos = Q.position(np.asarray(osc.coefs).reshape(-1, 20))
        self.last = {name: len(Q.chunks(t)) - 1 for name, t in Q.tables(np.asarray(osc.coefs).reshape(-1, 20)).items() if t}

    def of_pixels(self, mask, stop=None, limit=4000):
        """The owners (object indices >= 0) of the samples of the pixels where `mask` is set, pixel by pixel until stop(set) says enough
        (or `limit` pixels were visited)."""
        seen = set()
        for y, x in list(zip(*np.nonzero(mask)))[:limit]:
            for j in range(self.k):
                for i in range(self.k):
                    o = self.own.owner(self.k * int(x) + i, self.k * int(y) + j)
                    if o >= 0:
                        seen.add(o)
            if stop is not None and stop(seen):
                break
        return seen

    def spans_first_and_last_chunk(self, seen):
        """Some owner lies in chunk 0 of its table and some in the last chunk of a table."""
        first = any(self.pos[o][1] == 0 for o in seen)
        last = any(self.pos[o][1] == self.last[self.pos[o][0]] for o in seen)
        return first and last

    def owns_sample_in(self, obj, mask, tries=64):
        """Object `obj` is the primary hit of a sample of a pixel where `mask` is set.  The samples whose ray meets `obj` at all are found
        with one intersection each; the nearest-hit loop then runs only on those that lie in such a pixel, until one is obj's."""
        import ctypes as C
        own, k = self.own, self.k
        dp = C.POINTER(C.c_double)
        ys, xs = np.nonzero(mask)
        tried = 0
        for y, x in zip(ys.tolist(), xs.tolist()):
            for j in range(k):
                for i in range(k):
                    d = np.ascontiguousarray(own.dirs[k * y + j, k * x + i])
                    t = own.L.orc_intersect_ray(own.cptr[obj], own.o.ctypes.data_as(dp), d.ctypes.data_as(dp))
                    if t >= S.K_EPS and t < S.K_MAX_T:
                        if own.owner(k * x + i, k * y + j) == obj:
                            return True
                        tried += 1
                        if tried >= tries:
                            return False
        return False
