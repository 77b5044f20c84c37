"""The ray queries' reference statement (include/mi355rt.h, "Ray queries"), composed from what the oracle exports -- test
infrastructure, like gbuffer_ref.py.

closest:  per ray the reference's nearest-hit loop (src/update-cpu.cpp:50-56) over orc_intersect_ray in object order with
          `t >= K_EPS and t < K_MAX_T and t < best_t`; the hit point o + t * d in numpy float64 (one multiply, one add per component);
          orc_normal_vector there; normals through astype(float32).  A miss: object -1, t +inf, point and normal +0.
occluded: per ray the reference's shadow loop (src/update-cpu.cpp:66-72): blocked iff some object gives `t > K_EPS and t < t_max`.
Plain Python loops over the oracle's C functions: nothing is vectorised that could change the arithmetic."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

K_EPS = 1e-7
K_MAX_T = 1e6
K_SHADOW_BIAS = 1e-2   # include/surface_impl.h:18
HIT_DTYPE = np.dtype([("t", np.float64), ("point", np.float64, 3), ("normal", np.float32, 3), ("object", np.int32)])
RAY_DTYPE = np.dtype([("o", np.float64, 3), ("d", np.float64, 3)])


def make_rays(origins, dirs):
    o, d = np.asarray(origins, dtype=np.float64), np.asarray(dirs, dtype=np.float64)
    out = np.zeros(max(o.size, d.size) // 3, dtype=RAY_DTYPE)
    out["o"] = o.reshape(-1, 3)
    out["d"] = d.reshape(-1, 3)
    return out


def _coef_ptrs(osc):
    dp = C.POINTER(C.c_double)
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, O.NCOEF)
    return coefs, [coefs[k].ctypes.data_as(dp) for k in range(len(coefs))]


def closest(osc, rays, normals64=None):
    """HIT_DTYPE records of the RAY_DTYPE array `rays` against the oracle scene `osc`.  normals64: an optional [n, 3] float64 array
    that receives the unrounded normals (what the reference's own shading uses)."""
    L = O.lib()
    dp = C.POINTER(C.c_double)
    coefs, cptr = _coef_ptrs(osc)
    out = np.zeros(len(rays), dtype=HIT_DTYPE)
    out["t"] = np.inf
    out["object"] = -1
    o, d, p, n = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)
    op, dptr, pptr, nptr = (a.ctypes.data_as(dp) for a in (o, d, p, n))
    intersect, normal = L.orc_intersect_ray, L.orc_normal_vector
    with np.errstate(all="ignore"):
        for i in range(len(rays)):
            o[:] = rays["o"][i]
            d[:] = rays["d"][i]
            best, best_t = -1, np.inf
            for k, cp in enumerate(cptr):
                t = intersect(cp, op, dptr)
                if t >= K_EPS and t < K_MAX_T and t < best_t:
                    best, best_t = k, t
            if best >= 0:
                p[:] = o + np.float64(best_t) * d
                normal(cptr[best], pptr, nptr)
                out["object"][i], out["t"][i] = best, best_t
                out["point"][i] = p
                out["normal"][i] = n.astype(np.float32)
                if normals64 is not None:
                    normals64[i] = n
    return out


def occluded(osc, rays, t_max=None):
    """int32 [n]: 1 where ray i is blocked (`t > K_EPS and t < t_max[i]` for some object), else 0.  t_max None: K_MAX_T for every ray."""
    L = O.lib()
    dp = C.POINTER(C.c_double)
    coefs, cptr = _coef_ptrs(osc)
    tm = np.full(len(rays), K_MAX_T) if t_max is None else np.broadcast_to(np.asarray(t_max, dtype=np.float64), (len(rays),))
    out = np.zeros(len(rays), dtype=np.int32)
    o, d = np.zeros(3), np.zeros(3)
    op, dptr = o.ctypes.data_as(dp), d.ctypes.data_as(dp)
    intersect = L.orc_intersect_ray
    for i in range(len(rays)):
        o[:] = rays["o"][i]
        d[:] = rays["d"][i]
        lim = float(tm[i])
        for cp in cptr:
            t = intersect(cp, op, dptr)
            if t > K_EPS and t < lim:
                out[i] = 1
                break
    return out


def primary_rays(osc, cam=None, rows=None, cols=None):
    """The primary rays of the oracle scene's pixel grid as explicit rays, in row-major pixel order: origin = cam[12:15], direction =
    orc_primary_dir."""
    L = O.lib()
    dp = C.POINTER(C.c_double)
    cam = np.ascontiguousarray(O.IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
    rows = np.arange(osc.height) if rows is None else np.asarray(rows, dtype=np.int64)
    cols = np.arange(osc.width) if cols is None else np.asarray(cols, dtype=np.int64)
    sc = osc.c_scene()
    d = np.zeros(3)
    out = np.zeros(len(rows) * len(cols), dtype=RAY_DTYPE)
    out["o"] = cam[12:15]
    i = 0
    for y in rows.tolist():
        for x in cols.tolist():
            L.orc_primary_dir(C.byref(sc), cam.ctypes.data_as(dp), x, y, d.ctypes.data_as(dp))
            out["d"][i] = d
            i += 1
    return out


def shadow_rays(osc, hits, normals64):
    """The reference's shadow rays for the hits of `hits` (HIT_DTYPE, misses are left out) towards every light, hit-major then light
    order: o = sp + K_SHADOW_BIAS * n (FP64 normal), d and max_t from orc_shadow_ray (the direction through float).
    Returns (rays, t_max, hit index per ray, light index per ray)."""
    L = O.lib()
    dp = C.POINTER(C.c_double)
    idx = np.flatnonzero(hits["object"] >= 0)
    nl = len(osc.lights)
    rays = np.zeros(len(idx) * nl, dtype=RAY_DTYPE)
    tmax = np.zeros(len(idx) * nl)
    sp, df, mt = np.zeros(3), np.zeros(3, dtype=np.float32), C.c_double(0.0)
    j = 0
    for i in idx.tolist():
        sp[:] = hits["point"][i]
        for light in osc.lights:
            L.orc_shadow_ray(C.byref(light), sp.ctypes.data_as(dp), df.ctypes.data_as(C.POINTER(C.c_float)), C.byref(mt))
            rays["o"][j] = sp + np.float64(K_SHADOW_BIAS) * normals64[i]
            rays["d"][j] = df.astype(np.float64)
            tmax[j] = mt.value
            j += 1
    return rays, tmax, np.repeat(idx, nl), np.tile(np.arange(nl), len(idx))


def same_records(a, b):
    """Bit equality of two HIT_DTYPE arrays, field by field on integer views (+inf, NaN payloads and signed zeros count)."""
    return (np.array_equal(a["object"], b["object"]) and np.array_equal(a["t"].view(np.uint64), b["t"].view(np.uint64)) and
            np.array_equal(np.ascontiguousarray(a["point"]).view(np.uint64), np.ascontiguousarray(b["point"]).view(np.uint64)) and
            np.array_equal(np.ascontiguousarray(a["normal"]).view(np.uint32), np.ascontiguousarray(b["normal"]).view(np.uint32)))


def describe_difference(a, b):
    bad = np.flatnonzero((a["object"] != b["object"]) | (a["t"].view(np.uint64) != b["t"].view(np.uint64)) |
                         (np.ascontiguousarray(a["point"]).view(np.uint64) != np.ascontiguousarray(b["point"]).view(np.uint64)).any(axis=-1) |
                         (np.ascontiguousarray(a["normal"]).view(np.uint32) != np.ascontiguousarray(b["normal"]).view(np.uint32)).any(axis=-1))
    return f"{len(bad)} of {len(a)} records differ" + (f"; first at {int(bad[0])}: {a[bad[0]]} != {b[bad[0]]}" if len(bad) else "")
