"""Scenes and oracle-side conditions of the streamed frame kernel's tests (tests/test_stream_host.py, tests/test_stream_gpu.py) -- test
infrastructure.  The kernel (csrc/rt_stream.hip) passes the class tables through LDS 64 entries at a time, so the scenes are fields of
many small objects of ONE class with a count next to a multiple of 64, and the conditions say which objects must be visible for a
frame to have gone through a given chunk: who owns a pixel is decided by the reference's nearest-hit loop on the oracle's functions."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

CHUNK = 64            # entries the kernel stages at a time (rt_stream.hpp: SQ_CHUNK)
LDS_LIMIT = 160 * 1024
COUNTS = (1, 63, 64, 65, 128, 129, 193)
K_EPS, K_MAX_T = 1e-7, 1e6
FOV = 50.0
FIELD_SEED, LARGE_SEED, MIXED_SEED = 102, 7, 11   # seeds under which the conditions of tests/test_stream_host.py hold


def field(pkg, n, seed, kind="sphere", w=64, h=48, mirrors=False, depth=0, px=2.6, big_last=False):
    """n small objects of one class spread over the view of a w x h frame (camera at the origin looking along +z), about `px` pixels
    across each, at depths 20 .. 30; a directional and a point light.  kind: "sphere", or "quadric" (ellipsoids, half of them with
    cross terms: the general-quadric table).  mirrors: every third object reflects.  big_last: one large sphere more, appended last,
    between the lights and the field, so that its shadow falls on part of the field."""
    rng = np.random.default_rng(seed)
    sc = pkg.Scene.new(w, h, FOV, depth, (0.05, 0.1, 0.2))
    tan = np.tan(np.radians(FOV / 2))
    for i in range(n):
        z = rng.uniform(20.0, 30.0)
        half_h, half_w = z * tan, z * tan * w / h
        c = np.array([rng.uniform(-half_w, half_w) * 0.96, rng.uniform(-half_h, half_h) * 0.96, z])
        r = 0.5 * px * 2.0 * z * tan / h
        col = rng.uniform(0.2, 1.0, 3)
        refl = float(rng.uniform(0.3, 0.8)) if (mirrors and i % 3 == 0) else 0.0
        if kind == "sphere":
            sc.add_object(pkg.surface_make("sphere", c, [r]), col, refl)
        else:
            sc.add_object(ellipsoid(c, r * rng.uniform(0.7, 1.3, 3), rng.uniform(-0.3, 0.3, 3) if i % 2 else np.zeros(3)), col, refl)
    if big_last:
        sc.add_object(pkg.surface_make("sphere", [2.0, 5.0, 14.0], [2.5]), (0.9, 0.9, 0.9), 0.0)
    sc.add_light("directional", [0.2, -1.0, 0.6], (1.0, 0.95, 0.9), 1.2)
    sc.add_light("spherical", [4.0, 12.0, 2.0], (0.8, 0.9, 1.0), 500.0)
    return sc


def ellipsoid(c, semi, cross):
    """(p - c)^T A (p - c) = 1 as the 20 coefficients: A = diag(1 / semi^2) plus symmetric cross terms (relative to the diagonal)."""
    a = 1.0 / (np.asarray(semi) ** 2)
    A = np.diag(a)
    for (i, j), v in zip(((0, 1), (0, 2), (1, 2)), cross):
        A[i, j] = A[j, i] = 0.5 * v * np.sqrt(a[i] * a[j])
    q = np.zeros(20)
    q[10], q[11], q[12] = A[0, 0], A[1, 1], A[2, 2]
    q[13], q[14], q[15] = 2 * A[0, 1], 2 * A[0, 2], 2 * A[1, 2]
    q[16:19] = -2.0 * A @ c
    q[19] = float(c @ A @ c) - 1.0
    return q


def planes(pkg, n, seed, w=64, h=48, depth=0):
    """n planes (the linear table) below and behind the view, all tilted differently, some mirrors when depth > 0."""
    rng = np.random.default_rng(seed)
    sc = pkg.Scene.new(w, h, FOV, depth, (0.05, 0.1, 0.2))
    for i in range(n):
        nv = rng.normal(size=3)
        nv = nv / np.linalg.norm(nv) + np.array([0.0, 1.5, 0.0])
        sc.add_object(pkg.surface_make("plane", rng.uniform([-5, -8, 0], [5, -3, 30]), nv), rng.uniform(0.2, 1.0, 3), 0.4 if (depth and i % 4 == 0) else 0.0)
    sc.add_light("directional", [0.2, -1.0, 0.6], (1.0, 0.95, 0.9), 1.2)
    sc.add_light("spherical", [4.0, 12.0, 2.0], (0.8, 0.9, 1.0), 500.0)
    return sc


def mixed_large(pkg, n, seed, w=64, h=48, depth=2):
    """About n objects of every class of degree <= 2, interleaved so that every table has several chunks except the planes' (a floor and
    a back wall), every fifth object a mirror."""
    rng = np.random.default_rng(seed)
    sc = pkg.Scene.new(w, h, FOV, depth, (0.05, 0.1, 0.2))
    tan = np.tan(np.radians(FOV / 2))
    for i in range(n):
        z = rng.uniform(20.0, 30.0)
        half_h, half_w = z * tan, z * tan * w / h
        c = np.array([rng.uniform(-half_w, half_w) * 0.96, rng.uniform(-half_h, half_h) * 0.96, z])
        r = 1.3 * 2.0 * z * tan / h
        refl = float(rng.uniform(0.3, 0.8)) if i % 5 == 0 else 0.0
        if i % 2 == 0:
            sc.add_object(pkg.surface_make("sphere", c, [r]), rng.uniform(0.2, 1.0, 3), refl)
        else:
            sc.add_object(ellipsoid(c, r * rng.uniform(0.7, 1.3, 3), rng.uniform(-0.3, 0.3, 3) if i % 4 == 1 else np.zeros(3)), rng.uniform(0.2, 1.0, 3), refl)
        if i == n // 2:
            sc.add_object(pkg.surface_make("plane", [0, -14, 0], [0.0, 1.0, 0.05]), (0.5, 0.5, 0.5), 0.3)
    sc.add_object(pkg.surface_make("plane", [0, 0, 40], [0.0, 0.1, -1.0]), (0.4, 0.5, 0.6), 0.0)
    sc.add_light("directional", [0.2, -1.0, 0.6], (1.0, 0.95, 0.9), 1.2)
    sc.add_light("spherical", [4.0, 12.0, 2.0], (0.8, 0.9, 1.0), 500.0)
    return sc


def oracle_of(pkg, sc):
    """The oracle's scene with the arrays of a product scene (tests/test_gpu_parity.py: oracle_from, without the GPU test module)."""
    a = sc.arrays()
    o = O.Scene(a["width"], a["height"], 0.0, a["max_reflections"], a["bg_color"])
    o.vertical_fov = a["vertical_fov"]
    for i in range(len(a["reflection"])):
        o.add_object(a["coefs"][i], a["albedo"][i], a["reflection"][i])
    for i in range(len(a["light_is_spherical"])):
        lt = O.OrcLight()
        lt.is_spherical = int(a["light_is_spherical"][i])
        for k in range(3):
            lt.p[k] = float(a["light_p"][i][k])
            lt.color[k] = float(a["light_color"][i][k])
        o.lights.append(lt)
    return o


class Owners:
    """Who owns a pixel of the oracle scene `osc`: the reference's nearest-hit loop (src/update-cpu.cpp:50-56) over orc_intersect_ray,
    evaluated only where asked (a whole object plane of a large scene would take minutes in Python)."""

    def __init__(self, osc, cam=None):
        self.osc, self.L = osc, O.lib()
        dp = C.POINTER(C.c_double)
        self.cam = np.ascontiguousarray(O.IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        self.sc = osc.c_scene()
        self.coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, O.NCOEF)
        self.cptr = [self.coefs[k].ctypes.data_as(dp) for k in range(len(self.coefs))]
        self.o = self.cam[12:15].copy()
        d = np.zeros(3)
        self.dirs = np.zeros((osc.height, osc.width, 3))
        for y in range(osc.height):
            for x in range(osc.width):
                self.L.orc_primary_dir(C.byref(self.sc), self.cam.ctypes.data_as(dp), x, y, d.ctypes.data_as(dp))
                self.dirs[y, x] = d
        self.known = {}

    def owner(self, x, y):
        if (x, y) not in self.known:
            dp = C.POINTER(C.c_double)
            d = np.ascontiguousarray(self.dirs[y, x])
            best, best_t = -1, np.inf
            for k, cp in enumerate(self.cptr):
                t = self.L.orc_intersect_ray(cp, self.o.ctypes.data_as(dp), d.ctypes.data_as(dp))
                if t >= K_EPS and t < K_MAX_T and t < best_t:
                    best, best_t = k, t
            self.known[(x, y)] = best
        return self.known[(x, y)]

    def centre(self, k):
        """Where the gradient of quadric k vanishes (a sphere's or an ellipsoid's centre)."""
        q = self.coefs[k]
        A = np.array([[2 * q[10], q[13], q[14]], [q[13], 2 * q[11], q[15]], [q[14], q[15], 2 * q[12]]])
        return np.linalg.solve(A, -q[16:19])

    def pixel_of(self, k):
        """A pixel that sphere / ellipsoid k owns, or None: the pixels whose rays point closest to its centre are tried."""
        c = self.centre(k) - self.o
        cosines = self.dirs @ (c / np.linalg.norm(c))
        for flat in np.argsort(-cosines, axis=None)[:4].tolist():
            y, x = divmod(flat, self.osc.width)
            if self.owner(x, y) == k:
                return x, y
        return None

    def some_owner_in(self, lo, hi):
        """The first object of lo .. hi - 1 (spheres / ellipsoids) that owns a pixel, or None."""
        for k in range(lo, hi):
            if self.pixel_of(k) is not None:
                return k
        return None


def first_count_beyond_lds(pkg, n_lights=2):
    """The first sphere count whose default context does not fit a workgroup's LDS, by the launcher's own rule: the library's
    rt_wavefront_lds_bytes_strict on the words rt_create forms for a field of n culled spheres without mirrors (class tables and
    materials: n x (64 + 16) bytes from FrameArgs::off_us on)."""
    f = pkg.lib().rt_wavefront_lds_bytes_strict
    f.restype = C.c_size_t
    f.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_uint32]
    def beyond(n):
        return f(n * (64 + 16), n_lights, 0, n, 0, 0) > LDS_LIMIT
    lo, hi = 4, 8   # beyond(lo) is False, beyond(hi) becomes True: the rule grows with n
    assert not beyond(lo)
    while not beyond(hi):
        lo, hi = hi, 2 * hi
        assert hi < (1 << 24)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if beyond(mid) else (mid, hi)
    return hi
