"""The G-buffer's reference statement (include/mi355rt.h, "G-buffer"), composed from what the oracle exports -- test infrastructure.

Per pixel: origin = cam[12:15]; d = orc_primary_dir; the reference's nearest-hit loop (src/update-cpu.cpp:50-56) over
orc_intersect_ray in object order with `t >= K_EPS and t < K_MAX_T and t < best_t`; the hit point o + t * d formed in numpy float64
(one multiply, one add per component); orc_normal_vector there; normals through astype(float32).  A plain Python loop over the
oracle's C functions (about 11 us per pixel and object): nothing is vectorised that could change the arithmetic."""
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


def compose(osc, cam=None, rows=None, cols=None):
    """Planes of the oracle scene `osc` for global rows `rows` (default: all) and columns `cols` (default: all):
    dict(object int32 [R, C], t float64 [R, C], normal float32 [R, C, 4], point float64 [R, C, 3], dir float64 [R, C, 3])."""
    L = O.lib()
    dp = C.POINTER(C.c_double)
    cam = np.ascontiguousarray(O.IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
    rows = np.arange(osc.height) if rows is None else np.asarray(rows, dtype=np.int64)
    cols = np.arange(osc.width) if cols is None else np.asarray(cols, dtype=np.int64)
    sc = osc.c_scene()
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, O.NCOEF)
    cptr = [coefs[k].ctypes.data_as(dp) for k in range(len(coefs))]
    o = cam[12:15].copy()
    op, camp = o.ctypes.data_as(dp), cam.ctypes.data_as(dp)
    d, p, n = np.zeros(3), np.zeros(3), np.zeros(3)
    dptr, pptr, nptr = d.ctypes.data_as(dp), p.ctypes.data_as(dp), n.ctypes.data_as(dp)
    obj = np.full((len(rows), len(cols)), -1, dtype=np.int32)
    tt = np.full((len(rows), len(cols)), np.inf, dtype=np.float64)
    nrm = np.zeros((len(rows), len(cols), 4), dtype=np.float32)
    pts = np.zeros((len(rows), len(cols), 3), dtype=np.float64)
    dirs = np.zeros((len(rows), len(cols), 3), dtype=np.float64)
    intersect, primary, normal = L.orc_intersect_ray, L.orc_primary_dir, L.orc_normal_vector
    for i, y in enumerate(rows.tolist()):
        for j, x in enumerate(cols.tolist()):
            primary(C.byref(sc), camp, x, y, dptr)
            dirs[i, j] = d
            best, best_t = -1, np.inf
            for k, cp in enumerate(cptr):
                t = intersect(cp, op, dptr)
                if t >= K_EPS and t < K_MAX_T and t < best_t:
                    best, best_t = k, t
            if best >= 0:
                p[:] = o + np.float64(best_t) * d
                normal(cptr[best], pptr, nptr)
                obj[i, j], tt[i, j] = best, best_t
                pts[i, j] = p
                nrm[i, j, :3] = n.astype(np.float32)
    return dict(object=obj, t=tt, normal=nrm, point=pts, dir=dirs)
