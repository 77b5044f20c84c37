"""Exact arithmetic and rounding bounds for surfaces of degree <= 2 -- test infrastructure, like rays_ref.py.  What holds an
RT_FLAG_FAST kernel (tests/test_fast_truth_gpu.py) and is itself held on the CPU first (tests/test_fast_ref_host.py).

TRUTH.  For a surface of degree <= 2 everything a ray test computes is a rational function of doubles plus one square root.  t2, t1, t0
of the reference's ray polynomial are formed with fractions.Fraction from the exact values of the 20 coefficients, o and d, so is the
discriminant t1^2 - 4 t2 t0; the root follows the reference's selection rule (oracle/rt_oracle.c: solve_poly -- the smaller root if it
is >= EPS, else the other; the linear branch; -1) with mpmath at 50 digits.  Nothing here depends on the oracle or on a kernel.

BOUND.  Contraction removes roundings and never adds one, so a first-order running-error bound covers the strict and the contracted
evaluation alike, in any summation order and with any subset of the products fused.  With u = 2^-53, per ray/object pair:
    coefficients   e_k = (n_k + 3) u sum|products|     n_k: the products (of at most three factors) of t_k whose coefficient is not
                                                       an exact zero -- the class tables leave out only those, so the sums are theirs too
    discriminant   e_D = 2|t1| e1 + 4|t2| e0 + 4|t0| e2 + 3u (t1^2 + |4 t2 t0|)
    square root    e_s = e_D / (2 sqrt(D)) + u sqrt(D)
    root           B   = (e1 + e_s + u(|t1| + sqrt(D))) / |2 t2| + |t| (e2 / |t2| + 2u)
    linear branch  B   = e0 / |t1| + |t| (e1 / |t1| + 2u)
all of it in float64 from numpy's own evaluation of the same sums.  Where the direction is itself a rounded quantity (pixel-based entry
points: two kernels may form it a few units in the last place apart) the first-order term of a direction known to 4u per component is
added: with P(t) = F(o + t d), dP/dd_i = t dF/dx_i(o + t d) and dP/dt = 2 t2 t + t1 (+-sqrt(D) at a root), so
    B_dir = |t| sum_i |grad_i F(p)| 4u |d_i| / |2 t2 t + t1|.
(It enters every comparison of a root; what 4u of direction does to |t2| and to the discriminant's sign is a few u of their terms, which
the factor M below covers 2^18 times over.)

DECIDED.  A ray is decided when every decision made on its behalf clears its bound by M = 2^20: per object |t2| against EPS (|t1| in
the linear branch), the sign of D against e_D, the first root against EPS, the accepted t against EPS and MAX_T / t_max, and against
the winner's t as |t_a - t_b| > M (B_a + B_b).  M is a condition, not a measurement: a larger M only moves rays from "checked" to
"excluded", and the callers cap the excluded share.  An occlusion ray is decided when some object blocks it with all of its own
decisions clear, or every object clears all of them.  A path (decided_paths) is decided when every nearest-hit search and every shadow
test along the reference's render_pixel is; its later segments start from values a kernel may round differently by a few u, which M
covers by many orders of magnitude.  An object of degree 3 makes every ray undecided.

NORMALS.  The gradient in Fraction at a given point, normalised in mpmath; its bound is the gradient's own first-order bound over |grad|
(the projection (I - n n^T) has norm 1), 6u for the normalisation's own roundings, and half a float32 ulp of 1 for the stored float."""
import os
import sys
from fractions import Fraction

import mpmath
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays_ref  # noqa: E402

U = 2.0 ** -53
M = 2.0 ** 20
EPS, MAX_T, SHADOW_BIAS = rays_ref.K_EPS, rays_ref.K_MAX_T, rays_ref.K_SHADOW_BIAS
F_EPS = Fraction(EPS)
DPS = 50
HALF_ULP32 = 2.0 ** -24


# ---- truth ----------------------------------------------------------------------------------------------------------------------------------
def _fr(v):
    return [Fraction(float(x)) for x in v]


def exact_poly(q, o, d):
    """(t2, t1, t0) of F(o + t d) as Fractions, F the degree <= 2 part of the 20 coefficients q (the degree-3 part must be zero)."""
    assert not np.asarray(q)[:10].any(), "degree 3 is out of scope"
    x2, y2, z2, xy, xz, yz, kx, ky, kz, c = _fr(np.asarray(q)[10:20])
    (ox, oy, oz), (dx, dy, dz) = _fr(o), _fr(d)

    def s(*terms):   # sum of coefficient * factor, the factor formed only where the coefficient is not an exact zero
        return sum((k * f() for k, f in terms if k), Fraction(0))
    t2 = s((x2, lambda: dx * dx), (y2, lambda: dy * dy), (z2, lambda: dz * dz), (xy, lambda: dx * dy), (xz, lambda: dx * dz), (yz, lambda: dy * dz))
    t1 = s((x2, lambda: 2 * ox * dx), (y2, lambda: 2 * oy * dy), (z2, lambda: 2 * oz * dz), (xy, lambda: ox * dy + dx * oy), (xz, lambda: ox * dz + dx * oz),
           (yz, lambda: oy * dz + dy * oz), (kx, lambda: dx), (ky, lambda: dy), (kz, lambda: dz))
    t0 = s((x2, lambda: ox * ox), (y2, lambda: oy * oy), (z2, lambda: oz * oz), (xy, lambda: ox * oy), (xz, lambda: ox * oz), (yz, lambda: oy * oz),
           (kx, lambda: ox), (ky, lambda: oy), (kz, lambda: oz)) + c
    return t2, t1, t0


def _mpf(f):
    return mpmath.mpf(f.numerator) / mpmath.mpf(f.denominator)


def solve_exact(t2, t1, t0, other_root=False):
    """The reference's root selection on exact coefficients: an mpmath number (-1 where the solver returns -1).  other_root: the
    quadratic branch's other choice (for the mutation tests)."""
    with mpmath.workdps(DPS):
        if abs(t2) > F_EPS:
            disc = t1 * t1 - 4 * t2 * t0
            if disc < 0:
                return mpmath.mpf(-1)
            s = mpmath.sqrt(_mpf(disc))
            lo, hi = (-_mpf(t1) - s) / (2 * _mpf(t2)), (-_mpf(t1) + s) / (2 * _mpf(t2))
            first = lo >= mpmath.mpf(EPS)
            return (lo if first else hi) if not other_root else (hi if first else lo)
        if abs(t1) > F_EPS:
            return _mpf(-t0 / t1)
        return mpmath.mpf(-1)


_T_CACHE, _N_CACHE, _D_CACHE = {}, {}, {}


def exact_t(q, o, d):
    """The root the reference's solver returns for the ray (o, d) on the surface q in exact arithmetic (mpmath, 50 digits)."""
    q, o, d = (np.ascontiguousarray(a, dtype=np.float64) for a in (q, o, d))
    key = (q.tobytes(), o.tobytes(), d.tobytes())
    if key not in _T_CACHE:
        _T_CACHE[key] = solve_exact(*exact_poly(q, o, d))
    return _T_CACHE[key]


def exact_normal(q, p):
    """(n, bound): the normalised gradient of the surface q at the point p (three mpmath numbers) and what a float32 component computed
    in float64 from the same p may differ from it by."""
    q, p = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(p, dtype=np.float64)
    key = (q.tobytes(), p.tobytes())
    if key in _N_CACHE:
        return _N_CACHE[key]
    assert not q[:10].any(), "degree 3 is out of scope"
    x2, y2, z2, xy, xz, yz, kx, ky, kz, _ = _fr(q[10:20])
    px, py, pz = _fr(p)
    terms = [[2 * x2 * px, xy * py, xz * pz, kx], [2 * y2 * py, xy * px, yz * pz, ky], [2 * z2 * pz, xz * px, yz * py, kz]]
    g = [sum(t) for t in terms]
    e_g = sum((sum(1 for v in t if v != 0) + 3) * U * float(sum(abs(v) for v in t)) for t in terms)
    with mpmath.workdps(DPS):
        norm = mpmath.sqrt(_mpf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]))
        n = [_mpf(v) / norm for v in g] if norm != 0 else [mpmath.mpf("nan")] * 3
        bound = (e_g / float(norm) if norm != 0 else np.inf) + 6 * U + HALF_ULP32
    _N_CACHE[key] = (n, bound)
    return _N_CACHE[key]


def exact_point(o, d, t):
    """o + t d as Fractions."""
    tf = Fraction(float(t))
    return [a + tf * b for a, b in zip(_fr(o), _fr(d))]


# ---- the bound, vectorised over rays x objects -----------------------------------------------------------------------------------------------
def _coefs(osc):
    return np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, 20)


def pairs(coefs, o, d, pixel_dirs=False, mutate=None):
    """Every ray (o, d: [n, 3]) against every object (coefs: [m, 20]) in float64: a dict of [n, m] arrays -- t (what the reference's
    solver returns), B (its bound), ok (|t2| or |t1| against EPS, the discriminant's sign and the root choice all clear their bounds
    by M; False for an object of degree 3), other (the quadratic branch's other root, NaN elsewhere) and the coefficients.
    mutate: "drop" leaves the product kz * dz out of t1, "f32" rounds t0 through float32 (the mutation tests' wrong kernels)."""
    o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    q = coefs[:, 10:20]
    (ox, oy, oz), (dx, dy, dz) = o.T, d.T
    one = np.ones_like(ox)
    mono2 = np.stack([dx * dx, dy * dy, dz * dz, dx * dy, dx * dz, dy * dz], axis=1)
    w2 = q[:, 0:6]
    mono1 = np.stack([2 * ox * dx, 2 * oy * dy, 2 * oz * dz, ox * dy, dx * oy, ox * dz, dx * oz, oy * dz, dy * oz, dx, dy, dz], axis=1)
    w1 = q[:, [0, 1, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8]]
    mono0 = np.stack([ox * ox, oy * oy, oz * oz, ox * oy, ox * oz, oy * oz, ox, oy, oz, one], axis=1)
    w0 = q[:, 0:10]
    if mutate == "drop":
        w1 = w1.copy()
        w1[:, 11] = 0.0
    with np.errstate(all="ignore"):
        t2, t1, t0 = mono2 @ w2.T, mono1 @ w1.T, mono0 @ w0.T
        if mutate == "f32":
            t0 = t0.astype(np.float32).astype(np.float64)
        e2 = (np.count_nonzero(w2, axis=1) + 3) * U * (np.abs(mono2) @ np.abs(w2).T)
        e1 = (np.count_nonzero(q[:, [0, 1, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8]], axis=1) + 3) * U * (np.abs(mono1) @ np.abs(w1).T)
        e0 = (np.count_nonzero(w0, axis=1) + 3) * U * (np.abs(mono0) @ np.abs(w0).T)
        a2, a1 = np.abs(t2), np.abs(t1)
        quad = a2 > EPS
        ok = np.abs(a2 - EPS) > M * e2
        # quadratic branch
        four = 4.0 * t2 * t0
        disc = t1 * t1 - four
        e_d = 2 * a1 * e1 + 4 * a2 * e0 + 4 * np.abs(t0) * e2 + 3 * U * (t1 * t1 + np.abs(four))
        root = quad & (disc >= 0)
        s = np.sqrt(np.where(root, disc, 0.0))
        e_s = e_d / (2 * s) + U * s
        num = e1 + e_s + U * (a1 + s)
        lo, hi = (-t1 - s) / (2 * t2), (-t1 + s) / (2 * t2)
        b_lo = num / (2 * a2) + np.abs(lo) * (e2 / a2 + 2 * U)
        b_hi = num / (2 * a2) + np.abs(hi) * (e2 / a2 + 2 * U)
        first = lo >= EPS
        ok &= ~quad | ((np.abs(disc) > M * e_d) & (~root | (np.abs(lo - EPS) > M * b_lo)))
        # linear branch
        lin = ~quad & (a1 > EPS)
        ok &= quad | (np.abs(a1 - EPS) > M * e1)
        t_lin = -t0 / t1
        b_lin = e0 / a1 + np.abs(t_lin) * (e1 / a1 + 2 * U)
        t = np.where(root, np.where(first, lo, hi), np.where(lin, t_lin, -1.0))
        B = np.where(root, np.where(first, b_lo, b_hi), np.where(lin, b_lin, 0.0))
        other = np.where(root, np.where(first, hi, lo), np.nan)
        if pixel_dirs:
            p = o[:, None, :] + t[:, :, None] * d[:, None, :]
            A = coefs[:, [10, 13, 14, 13, 11, 15, 14, 15, 12]].reshape(-1, 3, 3) * np.array([[2.0, 1, 1], [1, 2.0, 1], [1, 1, 2.0]])
            g = np.einsum("mij,nmj->nmi", A, p) + coefs[None, :, 16:19]
            slope = np.abs(2 * t2 * t + t1)
            B = B + np.where(root | lin, np.abs(t) * (np.abs(g) * (4 * U * np.abs(d))[:, None, :]).sum(axis=-1) / slope, 0.0)
        ok &= ~coefs[:, :10].any(axis=1)[None, :]
        ok &= np.isfinite(t) & np.isfinite(B)
    return dict(t=t, B=B, ok=ok, other=other, t2=t2, t1=t1, t0=t0)


def _rays(rays):
    return np.ascontiguousarray(rays["o"], dtype=np.float64), np.ascontiguousarray(rays["d"], dtype=np.float64)


def closest_arrays(coefs, o, d, pixel_dirs=False, mutate=None):
    """(winner [n] or -1, t [n] (+inf for a miss), B [n], decided [n], second [n]: the next accepted object or -1, pairs)."""
    pr = pairs(coefs, o, d, pixel_dirs, mutate)
    t, B = pr["t"], pr["B"]
    n = len(t)
    if t.shape[1] == 0:
        return np.full(n, -1), np.full(n, np.inf), np.zeros(n), np.ones(n, dtype=bool), np.full(n, -1), pr
    with np.errstate(all="ignore"):
        acc = (t >= EPS) & (t < MAX_T)
        clear = pr["ok"] & (np.abs(t - EPS) > M * B) & (np.abs(t - MAX_T) > M * B)
        key = np.where(acc, t, np.inf)
        win = np.argmin(key, axis=1)
        rows = np.arange(n)
        hit = acc[rows, win]
        tw, bw = key[rows, win], np.where(hit, B[rows, win], 0.0)
        rest = key.copy()
        rest[rows, win] = np.inf
        second = np.where(np.isfinite(rest.min(axis=1)), np.argmin(rest, axis=1), -1)
        gap = ~acc | (np.abs(t - tw[:, None]) > M * (B + bw[:, None]))
        gap[rows, win] = True
        decided = clear.all(axis=1) & gap.all(axis=1)
    return np.where(hit, win, -1), tw, bw, decided, second, pr


def decided_closest(osc, rays, pixel_dirs=False):
    """Per ray of the RAY_DTYPE array `rays` against the oracle scene `osc`: (winner or -1, t in float64 (+inf for a miss), B, decided).
    The exact t of a pair is exact_t's; the callers form it for the winner and the reported object only."""
    coefs, (o, d) = _coefs(osc), _rays(rays)
    key = (coefs.tobytes(), o.tobytes(), d.tobytes(), bool(pixel_dirs))
    if key not in _D_CACHE:
        if len(_D_CACHE) >= 8:
            _D_CACHE.clear()
        _D_CACHE[key] = closest_arrays(coefs, o, d, pixel_dirs=pixel_dirs)[:4]
    return _D_CACHE[key]


def occluded_arrays(coefs, o, d, t_max, mutate=None):
    pr = pairs(coefs, o, d, mutate=mutate)
    t, B = pr["t"], pr["B"]
    lim = np.broadcast_to(np.asarray(t_max, dtype=np.float64), (len(t),))[:, None]
    with np.errstate(all="ignore"):
        blocks = (t > EPS) & (t < lim)
        clear = pr["ok"] & (np.abs(t - EPS) > M * B) & (np.abs(t - lim) > M * B)
    return blocks.any(axis=1), (blocks & clear).any(axis=1) | clear.all(axis=1)


def decided_occluded(osc, rays, t_max=None):
    """(blocked [n] bool, decided [n] bool); t_max None: MAX_T for every ray."""
    return occluded_arrays(_coefs(osc), *_rays(rays), MAX_T if t_max is None else t_max)


def _normals(q, p):
    """The normalised gradient of the surfaces q [n, 20] at the points p [n, 3] in float64 (which path a pixel takes next hangs on it)."""
    g = np.stack([2 * q[:, 10] * p[:, 0] + q[:, 13] * p[:, 1] + q[:, 14] * p[:, 2] + q[:, 16],
                  2 * q[:, 11] * p[:, 1] + q[:, 13] * p[:, 0] + q[:, 15] * p[:, 2] + q[:, 17],
                  2 * q[:, 12] * p[:, 2] + q[:, 14] * p[:, 0] + q[:, 15] * p[:, 1] + q[:, 18]], axis=1)
    with np.errstate(all="ignore"):
        return g / np.sqrt((g * g).sum(axis=1))[:, None]


def decided_paths(osc, rays, pixel_dirs=False):
    """[n] bool: is every decision on the ray's whole path decided?  The walk is tests/tools/shade_ref.py::shade's (the reference's
    render_pixel): the nearest-hit search of the primary segment, per light the shadow test from sp + SHADOW_BIAS sn with the direction
    through float32, then bounces while the hit object reflects, up to max_reflections.  pixel_dirs: the primary direction is a
    rounded quantity (B_dir above)."""
    coefs = _coefs(osc)
    refl = np.array([np.float32(ob.reflection_ratio) for ob in osc.objects], dtype=np.float64)
    lights = [(bool(lt.is_spherical), np.array([lt.p[0], lt.p[1], lt.p[2]], dtype=np.float64)) for lt in osc.lights]
    o, d = _rays(rays)
    decided = np.ones(len(o), dtype=bool)
    active = np.arange(len(o))
    n_refl = 0
    while len(active):
        win, t, _, dec, _, _ = closest_arrays(coefs, o, d, pixel_dirs=pixel_dirs and n_refl == 0)
        decided[active] &= dec
        keep = win >= 0
        active, o, d, win, t = active[keep], o[keep], d[keep], win[keep], t[keep]
        if not len(active):
            break
        sp = o + t[:, None] * d
        sn = _normals(coefs[win], sp)
        so = sp + SHADOW_BIAS * sn
        for spherical, lp in lights:
            sd = ((lp[None, :] - sp) if spherical else np.broadcast_to(lp, sp.shape)).astype(np.float32).astype(np.float64)
            decided[active] &= occluded_arrays(coefs, so, sd, 1.0 if spherical else 1e6)[1]
        if n_refl == int(osc.max_reflections):
            break
        n_refl += 1
        keep = refl[win] > EPS
        d = (d - (2.0 * (d * sn).sum(axis=1))[:, None] * sn)[keep]
        active, o = active[keep], so[keep]
    return decided


# ---- the checks ------------------------------------------------------------------------------------------------------------------------------
class Report:
    """What a check found: n rays, excluded (not decided), the worst rho = |t - t_exact| / B, the failures as text."""

    def __init__(self, what, n, excluded):
        self.what, self.n, self.excluded, self.worst_rho, self.worst_normal, self.failures = what, n, int(excluded), 0.0, 0.0, []

    def fail(self, text):
        self.failures.append(text)

    def __str__(self):
        head = (f"{self.what}: worst rho {self.worst_rho:.3g}, worst normal error / bound {self.worst_normal:.3g}, {self.excluded} of {self.n} rays excluded, "
                f"{len(self.failures)} failures")
        return head + "".join("\n  " + f for f in self.failures[:8])

    def passed(self, cap):
        """Every decided ray inside its bounds and the excluded share within `cap`."""
        return not self.failures and self.excluded <= cap * self.n


def check_closest(osc, rays, got, what="", pixel_dirs=False, stop_at_first=False):
    """A Report on closest-hit results `got` (a mapping with "object", "t" and optionally "point" [n, 3] and "normal" [n, >= 3]) for the
    rays against truth: on every decided ray `object` is the winner, |t - t_exact| <= B (a miss: +inf), point[i] within
    2u(|o_i| + |t d_i|) of o_i + t d_i with the reported t, every normal component within exact_normal's bound of the exact normal at the
    reported point (without "point": at o + t d in float64).  Undecided rays are counted, not judged.  stop_at_first: return at the
    first failure (the mutation tests only ask whether there is one)."""
    coefs = _coefs(osc)
    win, _, B, decided = decided_closest(osc, rays, pixel_dirs)
    rep = Report(what, len(rays), (~decided).sum())
    obj, t = np.asarray(got["object"]).reshape(-1), np.asarray(got["t"], dtype=np.float64).reshape(-1)
    names = got.dtype.names if isinstance(got, np.ndarray) else got
    point = np.asarray(got["point"], dtype=np.float64).reshape(-1, 3) if "point" in names else None
    normal = np.asarray(got["normal"]).reshape(len(rays), -1)[:, :3] if "normal" in names else None
    with mpmath.workdps(DPS):
        for i in np.flatnonzero(decided).tolist():
            if stop_at_first and rep.failures:
                break
            k, o, d = int(win[i]), rays["o"][i], rays["d"][i]
            if int(obj[i]) != k:
                rep.fail(f"ray {i} (o {o.tolist()}, d {d.tolist()}): object {int(obj[i])}, exact winner {k}")
                continue
            if k < 0:
                if not np.isposinf(t[i]):
                    rep.fail(f"ray {i}: a miss with t {t[i]!r}")
                continue
            te = exact_t(coefs[k], o, d)
            rho = float(abs(mpmath.mpf(float(t[i])) - te) / mpmath.mpf(float(B[i]))) if np.isfinite(t[i]) else np.inf
            rep.worst_rho = max(rep.worst_rho, rho)
            if not rho <= 1.0:
                rep.fail(f"ray {i} (o {o.tolist()}, d {d.tolist()}), object {k}: t {float(t[i])!r}, exact {mpmath.nstr(te, 25)}, B {B[i]:.3e}, rho {rho:.3g}")
                continue
            if point is not None:
                for a, pe in enumerate(exact_point(o, d, t[i])):
                    tol = 2 * U * (abs(o[a]) + abs(t[i] * d[a]))
                    if not abs(Fraction(float(point[i, a])) - pe) <= Fraction(tol):
                        rep.fail(f"ray {i}, object {k}: point[{a}] {float(point[i, a])!r}, o + t d = {float(pe)!r}, bound {tol:.3e}")
            if normal is not None:
                p = point[i] if point is not None else o + t[i] * d
                ne, bn = exact_normal(coefs[k], p)
                err = max(float(abs(mpmath.mpf(float(normal[i, a])) - ne[a])) for a in range(3))
                rep.worst_normal = max(rep.worst_normal, err / bn)
                if not err <= bn:
                    rep.fail(f"ray {i}, object {k}: normal {normal[i].tolist()}, exact {[float(v) for v in ne]}, error {err:.3e}, bound {bn:.3e}")
    return rep


def check_occluded(osc, rays, t_max, got, what=""):
    """A Report on the blocked flags `got`: on every decided ray the flag is the exact one."""
    blocked, decided = decided_occluded(osc, rays, t_max)
    rep = Report(what, len(rays), (~decided).sum())
    got = np.asarray(got).reshape(-1)
    for i in np.flatnonzero(decided & ((got != 0) != blocked)).tolist():
        rep.fail(f"ray {i} (o {rays['o'][i].tolist()}, d {rays['d'][i].tolist()}, t_max {None if t_max is None else float(np.broadcast_to(t_max, (len(rays),))[i])}): "
                 f"blocked {int(got[i])}, exact {int(blocked[i])}")
    return rep


# ---- the test sets -----------------------------------------------------------------------------------------------------------------------------
W, H = 96, 72
N_RAYS = 2048
QUERY_CAP, FRAME_CAP = 0.01, 0.002   # the share of a set a check may leave out: of a query set's rays, of a frame's pixels
RAY_SEED, TMAX_SEED = 41, 42
SCENES = ("spheres", "mixed", "chunked")


def scene(pkg, name):
    """(a) "spheres": 24 unit spheres without mirrors (the lean path and the default schedule); (b) "mixed": 11 spheres, 11 general
    quadrics (every other one with cross terms), a floor and a back wall, six mirrors, a directional and a point light; (c) "chunked":
    65 spheres and 65 general quadrics plus the two planes -- one entry past the streamed kernels' 64-entry chunk.  All at 96 x 72."""
    import stream_scenes as S
    if name == "spheres":
        return S.field(pkg, 24, 301, "sphere", w=W, h=H, px=9.0)
    if name == "mixed":
        return S.mixed_large(pkg, 22, 302, w=W, h=H, depth=2)
    assert name == "chunked"
    return S.mixed_large(pkg, 130, 303, w=W, h=H, depth=2)


def query_rays(osc, seed, n=N_RAYS):
    """n rays: half the primary rays of a 32 x 32 grid of the 96 x 72 frame's pixels, half aimed -- from a random origin through a random
    point of a random object, from inside an object (near its centre) in a random direction, from a random origin AWAY from an object, and
    between two random points of the field; direction lengths 0.5 .. 2."""
    import query_table_scenes as Q
    rng = np.random.default_rng(seed)
    rows, cols = np.linspace(0, H - 1, 32).astype(np.int64), np.linspace(0, W - 1, 32).astype(np.int64)
    first = rays_ref.primary_rays(osc, rows=rows, cols=cols)
    coefs = _coefs(osc)
    centred = [Q.centre_and_radius(q) for q in coefs]
    centred = [cr for cr in centred if cr is not None]
    out = np.zeros(n, dtype=rays_ref.RAY_DTYPE)
    out[:len(first)] = first
    for i in range(len(first), n):
        c, r = centred[int(rng.integers(len(centred)))]
        r = min(r, 2.0)
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        kind = i % 4
        if kind == 0:
            o = c + (r + rng.uniform(0.3, 8.0)) * u
            v = rng.normal(size=3)
            dvec = c + 0.7 * r * rng.uniform(0, 1) * v / np.linalg.norm(v) - o
        elif kind == 1:
            o = c + 0.3 * r * rng.uniform(0, 1) * u
            dvec = rng.normal(size=3)
        elif kind == 2:
            o = c + (r + rng.uniform(0.3, 8.0)) * u
            dvec = o - c + rng.normal(size=3) * 0.3
        else:
            o = rng.uniform([-12, -9, 0], [12, 9, 32])
            dvec = rng.uniform([-12, -9, 18], [12, 9, 32]) - o
        out["o"][i] = o
        out["d"][i] = dvec / np.linalg.norm(dvec) * rng.uniform(0.5, 2.0)
    return out


def query_t_max(osc, rays, seed):
    """Per ray: half MAX_T, the rest 0.5 .. 1.5 times the nearest hit's t (1 .. 30 where the ray misses)."""
    rng = np.random.default_rng(seed)
    t = decided_closest(osc, rays)[1]
    near = np.where(np.isfinite(t), t * rng.uniform(0.5, 1.5, len(rays)), rng.uniform(1.0, 30.0, len(rays)))
    return np.where(rng.random(len(rays)) < 0.5, MAX_T, near)
