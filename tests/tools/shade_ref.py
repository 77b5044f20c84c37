"""rt_shade_rays' reference statement (include/mi355rt.h, "Ray queries", colour), composed from what the oracle exports -- test
infrastructure, like rays_ref.py.

shade: per ray the reference's render_pixel (rt_oracle.c:563-663 = src/update-cpu.cpp:45-119) with ray_origin := o and dir := d, the
       direction used as given.  Per segment the nearest-hit loop over orc_intersect_ray (`t >= K_EPS and t < K_MAX_T and t < best_t`),
       sp = o + t * d in numpy float64 (one multiply, one add per component), orc_normal_vector there, then per light orc_shadow_ray,
       the shadow loop from sp + K_SHADOW_BIAS * sn (`t > K_EPS and t < max_t`) and orc_surface_color of the unblocked lights.  The
       float32 steps (accumulate, clamp, cur_ratio, blend) are np.float32 scalars, one rounding per operation, in the reference's order.
Plain Python loops over the oracle's C functions: nothing is vectorised that could change the arithmetic."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays_ref  # noqa: E402
from rays_ref import HIT_DTYPE, K_EPS, K_MAX_T, K_SHADOW_BIAS, O  # noqa: E402

F1 = np.float32(1.0)


def shade(osc, rays, hits=False, segments=None):
    """[n, 4] float32 colours (r, g, b, 1) of the RAY_DTYPE array `rays` against the oracle scene `osc`; with hits=True also the
    HIT_DTYPE records of the first segments.  segments: an optional int array [n] that receives the number of segments traced."""
    L = O.lib()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    coefs, cptr = rays_ref._coef_ptrs(osc)
    albedo = [np.asarray(list(ob.color), dtype=np.float32) for ob in osc.objects]
    ratio = [np.float32(ob.reflection_ratio) for ob in osc.objects]
    bg = [np.float32(v) for v in np.asarray(osc.bg_color, dtype=np.float32)]
    lights = list(osc.lights)
    max_refl = int(osc.max_reflections)
    out = np.zeros((len(rays), 4), dtype=np.float32)
    out[:, 3] = 1.0
    rec = np.zeros(len(rays), dtype=HIT_DTYPE)
    rec["t"] = np.inf
    rec["object"] = -1
    o, d, sp, sn, so, sd, nd = (np.zeros(3) for _ in range(7))
    sdf, col = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    op, dptr, spp, snp, sop, sdp, ndp = (a.ctypes.data_as(dp) for a in (o, d, sp, sn, so, sd, nd))
    sdfp, colp = sdf.ctypes.data_as(fp), col.ctypes.data_as(fp)
    mt = C.c_double(0.0)
    intersect = L.orc_intersect_ray

    def trace():
        """get_color_and_object for the ray (o, d): (object or -1, best_t, [3] np.float32 colour); sp and sn are left in place."""
        best, best_t = -1, np.inf
        for k, cp in enumerate(cptr):
            t = intersect(cp, op, dptr)
            if t >= K_EPS and t < K_MAX_T and t < best_t:
                best, best_t = k, t
        if best < 0:
            return -1, best_t, None
        sp[:] = o + np.float64(best_t) * d
        L.orc_normal_vector(cptr[best], spp, snp)
        acc = [np.float32(0.0)] * 3
        alb = albedo[best].ctypes.data_as(fp)
        for light in lights:
            L.orc_shadow_ray(C.byref(light), spp, sdfp, C.byref(mt))
            sd[:] = sdf.astype(np.float64)
            so[:] = sp + np.float64(K_SHADOW_BIAS) * sn
            lim = mt.value
            blocked = False
            for cp in cptr:
                t = intersect(cp, sop, sdp)
                if t > K_EPS and t < lim:
                    blocked = True
                    break
            if not blocked:
                L.orc_surface_color(C.byref(light), spp, snp, alb, colp)
                acc = [acc[i] + col[i] for i in range(3)]
        return best, best_t, [a if a < F1 else F1 for a in acc]

    def blend(res, r, c):
        return [(F1 - r) * res[i] + r * c[i] for i in range(3)]

    with np.errstate(all="ignore"):
        for i in range(len(rays)):
            o[:] = rays["o"][i]
            d[:] = rays["d"][i]
            idx, t, oc = trace()
            nseg = 1
            if idx < 0:
                res = bg
            else:
                rec["object"][i], rec["t"][i] = idx, t
                rec["point"][i] = sp
                rec["normal"][i] = sn.astype(np.float32)
                res = oc
                cur_ratio, n_refl = F1, 0
                while float(ratio[idx]) > K_EPS:
                    cur_ratio = cur_ratio * ratio[idx]
                    if n_refl == max_refl:
                        res = blend(res, cur_ratio, bg)
                        break
                    n_refl += 1
                    L.orc_reflect_ray(dptr, snp, ndp)
                    d[:] = nd
                    o[:] = sp + np.float64(K_SHADOW_BIAS) * sn
                    idx, t, oc = trace()
                    nseg += 1
                    if idx < 0:
                        res = blend(res, cur_ratio, bg)
                        break
                    res = blend(res, cur_ratio, oc)
            out[i, :3] = res
            if segments is not None:
                segments[i] = nseg
    return (out, rec) if hits else out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def describe_difference(a, b):
    bad = np.flatnonzero((np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) != np.ascontiguousarray(b, dtype=np.float32).view(np.uint32)).any(axis=-1))
    return f"{len(bad)} of {len(a)} colours differ" + (f"; first at {int(bad[0])}: {a[bad[0]]} != {b[bad[0]]}" if len(bad) else "")
