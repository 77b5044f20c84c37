"""rt_trace_paths' reference statement (include/mi355rt.h, "Ray queries", paths), composed from what the oracle exports -- test
infrastructure, like rays_ref.py and shade_ref.py, with which it shares nothing but rays_ref's constants and record types.

paths: per ray the geometry of the reference's render_pixel (src/update-cpu.cpp:82-119) with ray_origin := o and dir := d, the
       direction used as given.  Per segment the nearest-hit loop over orc_intersect_ray (`t >= K_EPS and t < K_MAX_T and t < best_t`),
       sp = o + t * d in numpy float64 (one multiply, one add per component), orc_normal_vector there; then the reflection-ratio test in
       double, the ratio product in np.float32, the cap test, orc_reflect_ray of the direction as it is and the new origin
       sp + K_SHADOW_BIAS * sn.
Plain Python loops over the oracle's C functions: nothing is vectorised that could change the arithmetic."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays_ref  # noqa: E402
from rays_ref import HIT_DTYPE, K_EPS, K_MAX_T, K_SHADOW_BIAS, O  # noqa: E402

END_DTYPE = np.dtype([("segments", np.uint32), ("end", np.uint32), ("ratio", np.float32), ("object", np.int32)])
MISS, SURFACE, ESCAPED, CAP = 0, 1, 2, 3
MAX_SEGMENTS = 64


def miss_records(shape):
    rec = np.zeros(shape, dtype=HIT_DTYPE)
    rec["t"] = np.inf
    rec["object"] = -1
    return rec


def paths(osc, rays, max_segments=None, ratios=None, seg_rays=None):
    """(segments [M, n] HIT_DTYPE, last [n] HIT_DTYPE, ends [n] END_DTYPE) of the RAY_DTYPE array `rays` against the oracle scene `osc`;
    M = max_segments, by default max_reflections + 1.  ratios: an optional list that receives, per ray, the list of cur_ratio values
    after each mirror met (np.float32), in order.  seg_rays: an optional [M, n] RAY_DTYPE array that receives the ray of every segment
    traced, the one that left the scene included."""
    L = O.lib()
    dp = C.POINTER(C.c_double)
    coefs, cptr = rays_ref._coef_ptrs(osc)
    ratio = [np.float32(ob.reflection_ratio) for ob in osc.objects]
    max_refl = int(osc.max_reflections)
    m = max_refl + 1 if max_segments is None else int(max_segments)
    n = len(rays)
    seg, last, ends = miss_records((m, n)), miss_records(n), np.zeros(n, dtype=END_DTYPE)
    o, d, sp, sn, nd = (np.zeros(3) for _ in range(5))
    op, dptr, spp, snp, ndp = (a.ctypes.data_as(dp) for a in (o, d, sp, sn, nd))
    intersect = L.orc_intersect_ray
    with np.errstate(all="ignore"):
        for i in range(n):
            o[:] = rays["o"][i]
            d[:] = rays["d"][i]
            cur, k, obj, seen = np.float32(1.0), 0, -1, []
            while True:
                if seg_rays is not None and k < len(seg_rays):
                    seg_rays["o"][k, i], seg_rays["d"][k, i] = o, d
                best, best_t = -1, np.inf
                for j, cp in enumerate(cptr):
                    t = intersect(cp, op, dptr)
                    if t >= K_EPS and t < K_MAX_T and t < best_t:
                        best, best_t = j, t
                if best < 0:
                    end, nseg = (MISS if k == 0 else ESCAPED), k
                    break
                sp[:] = o + np.float64(best_t) * d
                L.orc_normal_vector(cptr[best], spp, snp)
                rec = (best_t, sp.copy(), sn.astype(np.float32), best)
                last[i] = rec
                if k < m:
                    seg[k, i] = rec
                obj, nseg = best, k + 1
                if not float(ratio[best]) > K_EPS:
                    end = SURFACE
                    break
                cur = cur * ratio[best]
                seen.append(cur)
                if k == max_refl:
                    end = CAP
                    break
                L.orc_reflect_ray(dptr, snp, ndp)
                d[:] = nd
                o[:] = sp + np.float64(K_SHADOW_BIAS) * sn
                k += 1
            ends[i] = (nseg, end, cur, obj)
            if ratios is not None:
                ratios.append(seen)
    return seg, last, ends


def same_ends(a, b):
    """Bit equality of two END_DTYPE arrays (the ratio on its integer view)."""
    return all(np.array_equal(a[f], b[f]) for f in ("segments", "end", "object")) and np.array_equal(a["ratio"].view(np.uint32), b["ratio"].view(np.uint32))


def nan_to_zero(rec):
    """A copy of HIT_DTYPE records with NaN components replaced by 0, and where they were: against a composer a NaN has to meet a NaN
    (IEEE 754 leaves its sign and payload open; raw_desc_scenes.same_as_oracle)."""
    r = rec.copy()
    masks = []
    for f in ("t", "point", "normal"):
        nan = np.isnan(r[f])
        masks.append(nan)
        r[f][nan] = 0.0
    return r, masks


def same_as_composer(got, want):
    """HIT_DTYPE records (any shape) against the composer's: NaN where it has NaN, the same bits everywhere else."""
    g, gm = nan_to_zero(got.reshape(-1))
    w, wm = nan_to_zero(want.reshape(-1))
    return got.shape == want.shape and all(np.array_equal(a, b) for a, b in zip(gm, wm)) and rays_ref.same_records(g, w)


def ends_as_composer(got, want):
    g, w = got.copy(), want.copy()
    nan = np.isnan(w["ratio"])
    if not np.array_equal(np.isnan(g["ratio"]), nan):
        return False
    g["ratio"][nan] = 0.0
    w["ratio"][nan] = 0.0
    return same_ends(g, w)


def describe(got, want):
    seg, last, ends = got
    wseg, wlast, wends = want
    bad = np.flatnonzero((ends["segments"] != wends["segments"]) | (ends["end"] != wends["end"]) | (ends["object"] != wends["object"]) |
                         (ends["ratio"].view(np.uint32) != wends["ratio"].view(np.uint32)))
    text = f"{len(bad)} of {len(ends)} ends differ" + (f"; first at {int(bad[0])}: {ends[bad[0]]} != {wends[bad[0]]}" if len(bad) else "")
    if last is not None:
        text += "; last: " + rays_ref.describe_difference(last, wlast)
    if seg.size:
        text += "; segments: " + rays_ref.describe_difference(seg.reshape(-1), wseg.reshape(-1))
    return text
