"""Exact arithmetic and rounding bounds for surfaces of degree <= 3 -- test infrastructure, like rays_ref.py.  What holds an
RT_FLAG_FAST kernel, and for degree 3 the strict one too (tests/test_fast_truth_gpu.py), and is itself held on the CPU first
(tests/test_fast_ref_host.py).

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
covers by many orders of magnitude.

DEGREE 3.  Truth: t3 .. t0 in Fraction from every expanded monomial (exact_poly); |t3| > EPS and the sign of q^3 + r^2, q and r as
solve_poly defines them, decided in Fraction; the real roots in mpmath at 60 digits, each isolated by a sign change of the exact
polynomial across 1e-40 of its value (cubic_roots_exact: no threshold on imaginary parts anywhere); the reference's selection -- the one
real root unfiltered, or of three the largest, replaced by a smaller one that is >= EPS.  |t3| <= EPS: the degree <= 2 rule above.
Bound B3, first order, every arithmetic step charged u of its result and every libm call (cbrt, acos, cos) one ulp = 2u of its result,
which is the bar tests/test_oracle_libm.py and tests/test_cubic_device.py hold the device's to:
    coefficients   e_k = (n_k + 4) u sum|products|     over the expanded products of t_k (at most four factors and an integer: the dense
                                                       and the Taylor evaluation, in any order, with any products fused)
    a_k = t_k / t3 e_ak = e_k / |t3| + |a_k| (e3 / |t3| + u)
    q = (3 a1 - a2^2) / 9                     e_q = (3 e_a1 + 2|a2| e_a2 + u(3|a1| + a2^2 + |3 a1 - a2^2|)) / 9 + u|q|
    r = (9 a2 a1 - 27 a0 - 2 a2^3) / 54       e_r = (9(|a2| e_a1 + |a1| e_a2) + 27 e_a0 + 6 a2^2 e_a2
                                                     + u(2|9 a2 a1| + |27 a0| + 3|2 a2^3| + |9 a2 a1 - 27 a0| + |54 r|)) / 54 + u|r|
    D = q^3 + r^2                             e_D = 3 q^2 e_q + 2|r| e_r + u(2|q^3| + r^2 + |D|)
    D > 0:  s = sqrt(D), e_s = e_D / (2s) + u s;  P = r + s, Q = r - s, e_P = e_r + e_s + u|P| (e_Q alike);
            B3 = e_P / (3 cbrt(P)^2) + e_Q / (3 cbrt(Q)^2) + 2u(|cbrt P| + |cbrt Q|) + e_a2 / 3 + u|a2 / 3| + u|cbrt P + cbrt Q| + u|t|
            (where q^3 << r^2 the term in Q is the reference's own cancellation: its formula amplifies rounding by up to 10^6)
    D <= 0: v = -q^3, e_v = 3 q^2 e_q + 2u|q^3|;  sv = sqrt(v), e_sv = e_v / (2 sv) + u sv;  arg = r / sv, e_arg = e_r / sv + |arg|(e_sv / sv + u);
            theta = acos(arg) / 3, e_theta = (e_arg / sqrt(-D / v) + 2u acos(arg)) / 3 + u theta   (1 - arg^2 = -D / v: no cancellation);
            c = 2 sqrt(-q), e_c = e_q / sqrt(-q) + u c;  phi_k = theta + k 2pi/3, e_phi = e_theta + u|phi_k| + k u 2pi/3;
            x_k = c cos(phi_k) - a2 / 3,  B3_k = |cos| e_c + c(|sin| e_phi + 2u|cos|) + u|c cos| + e_a2 / 3 + u|a2 / 3| + u|x_k|
Decided: | |t3| - EPS | > M e3, |D| > M e_D (which also keeps acos away from the ends of its range, so that first order is valid), each of
the two filtered trigonometric roots against EPS and, where one is >= EPS, against the root it is compared with; then the accepted t as
above.  B_dir has P'(t) = 3 t3 t^2 + 2 t2 t + t1 and the full gradient.  PROMISE FOR GUARDED ANSWERS: cubic_guarded (csrc/rt_math.hpp)
answers only where its result is within CUB_TOL = 1e-8 relative of the reference's, so a kernel's degree-3 t is held to
B3 + CUB_TOL |t_exact| (check_closest(guarded=...)); B3 alone holds the oracle and a dense-path result.  The guard protects a root's
comparisons with EPS and max_t, not those between objects: two objects' roots must differ by more than M (B_a + B_b) +
CUB_TOL (|t_a| + |t_b|) when either is of degree 3.

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
DPS3 = 60            # the roots of a degree-3 ray polynomial
CUB_TOL = 1e-8       # csrc/rt_math.hpp: what a guarded degree-3 answer may differ from the reference's by, relative
TWO_THIRD_PI = 3.14159265358979323846 * 2.0 / 3.0
HALF_ULP32 = 2.0 ** -24


# ---- truth ----------------------------------------------------------------------------------------------------------------------------------
def _fr(v):
    return [Fraction(float(x)) for x in v]


# the 20 coefficients as exponents of (x, y, z), in the order of oracle/rt_oracle.h (ORC_X3 .. ORC_C)
MONO = ((3, 0, 0), (0, 3, 0), (0, 0, 3), (2, 1, 0), (1, 2, 0), (2, 0, 1), (1, 0, 2), (0, 2, 1), (0, 1, 2), (1, 1, 1),
        (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))
_BINOM = ((1,), (1, 1), (1, 2, 1), (1, 3, 3, 1))


def exact_poly(q, o, d):
    """(t3, t2, t1, t0) of F(o + t d) as Fractions, F the polynomial of the 20 coefficients q: every monomial with a coefficient that is
    not an exact zero is expanded as the product of its factors (o_a + t d_a)."""
    of, df = _fr(o), _fr(d)
    t = [Fraction(0)] * 4
    for k, e in zip(_fr(np.asarray(q)), MONO):
        if not k:
            continue
        poly = [Fraction(1)]
        for a in range(3):
            for _ in range(e[a]):
                nxt = [Fraction(0)] * (len(poly) + 1)
                for i, c in enumerate(poly):
                    nxt[i] += c * of[a]
                    nxt[i + 1] += c * df[a]
                poly = nxt
        for i, c in enumerate(poly):
            t[i] += k * c
    return t[3], t[2], t[1], t[0]


def _mpf(f):
    return mpmath.mpf(f.numerator) / mpmath.mpf(f.denominator)


def _frac(x):
    """The exact value of an mpmath number."""
    sign, man, exp, _ = x._mpf_
    v = Fraction(int(man)) * (Fraction(2) ** int(exp))
    return -v if sign else v


def cubic_roots_exact(t3, t2, t1, t0):
    """(one_root, roots): the real roots of t3 x^3 + t2 x^2 + t1 x + t0 (Fractions, t3 != 0), ascending, as mpmath numbers at DPS3
    digits.  one_root is the exact sign test of the reference's solver: q^3 + r^2 > 0 with q and r as solve_poly defines them, which
    is also what says how many real roots there are (one, else three counted with multiplicity).  The roots start from closed forms in
    mpmath, are polished by Newton steps on the exact coefficients, and each is then ISOLATED: the exact polynomial changes sign
    between x - w and x + w, w = 1e-40 max(1, |x|), and the intervals are disjoint.  Raises ArithmeticError where that fails (a
    multiple root, or roots closer than 1e-40: nothing a decided ray comes near)."""
    a2, a1, a0 = t2 / t3, t1 / t3, t0 / t3
    q = (3 * a1 - a2 * a2) / 9
    r = (9 * a2 * a1 - 27 * a0 - 2 * a2 * a2 * a2) / 54
    disc = q * q * q + r * r

    def p(x):
        return ((x + a2) * x + a1) * x + a0
    with mpmath.workdps(DPS3):
        m2, m1, m0, shift = _mpf(a2), _mpf(a1), _mpf(a0), _mpf(a2) / 3

        def real_cbrt(v):
            return mpmath.cbrt(v) if v >= 0 else -mpmath.cbrt(-v)
        if disc > 0:
            s = mpmath.sqrt(_mpf(disc))
            xs = [real_cbrt(_mpf(r) + s) + real_cbrt(_mpf(r) - s) - shift]
        elif q == 0:
            xs = [-shift] * 3
        else:
            arg = _mpf(r) / mpmath.sqrt(_mpf(-q * q * q))
            theta = mpmath.acos(max(min(arg, mpmath.mpf(1)), mpmath.mpf(-1))) / 3
            xs = [2 * mpmath.sqrt(_mpf(-q)) * mpmath.cos(theta + 2 * k * mpmath.pi / 3) - shift for k in range(3)]
        for _ in range(3):
            nxt = []
            for x in xs:
                slope = (3 * x + 2 * m2) * x + m1
                nxt.append(x - (((x + m2) * x + m1) * x + m0) / slope if slope != 0 else x)
            xs = nxt
        xs = sorted(xs)
        brackets = []
        for x in xs:
            xf = _frac(x)
            w = max(abs(xf), Fraction(1)) / 10 ** 40
            lo, hi = p(xf - w), p(xf + w)
            if not ((lo < 0 < hi) or (hi < 0 < lo)):
                raise ArithmeticError("a root of the ray polynomial is not isolated")
            brackets.append((xf - w, xf + w))
        for (_, h), (l, _) in zip(brackets, brackets[1:]):
            if not h < l:
                raise ArithmeticError("two roots of the ray polynomial are not separated")
    return disc > 0, xs


def solve_exact(t3, t2, t1, t0, other_root=False):
    """The reference's root selection on exact coefficients: an mpmath number (-1 where the solver returns -1).  |t3| > EPS: the one
    real root, unfiltered, or of three the largest, replaced by a smaller one that is >= EPS.  other_root: the quadratic branch's other
    choice (for the mutation tests)."""
    if abs(t3) > F_EPS:
        one, xs = cubic_roots_exact(t3, t2, t1, t0)
        if one:
            return xs[0]
        x = xs[2]
        for x1 in xs[:2]:
            if x1 >= mpmath.mpf(EPS) and x1 < x:
                x = x1
        return x
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
    """The root the reference's solver returns for the ray (o, d) on the surface q in exact arithmetic (mpmath, 50 digits; 60 for a
    degree-3 polynomial)."""
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
    x3, y3, z3, x2y, xy2, x2z, xz2, y2z, yz2, xyz, x2, y2, z2, xy, xz, yz, kx, ky, kz, _ = _fr(q)
    px, py, pz = _fr(p)
    terms = [[3 * x3 * px * px, 2 * x2y * px * py, 2 * x2z * px * pz, xy2 * py * py, xz2 * pz * pz, xyz * py * pz, 2 * x2 * px, xy * py, xz * pz, kx],
             [3 * y3 * py * py, 2 * xy2 * px * py, 2 * y2z * py * pz, x2y * px * px, yz2 * pz * pz, xyz * px * pz, 2 * y2 * py, xy * px, yz * pz, ky],
             [3 * z3 * pz * pz, 2 * xz2 * px * pz, 2 * yz2 * py * pz, x2z * px * px, y2z * py * py, xyz * px * py, 2 * z2 * pz, xz * px, yz * py, kz]]
    more = 4 if q[:10].any() else 3   # (a degree-3 product has one factor and one rounding more)
    g = [sum(t) for t in terms]
    e_g = sum((sum(1 for v in t if v != 0) + more) * U * float(sum(abs(v) for v in t)) for t in terms)
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
    solver returns), B (its bound), ok (|t3|, |t2| or |t1| against EPS, the discriminant's sign and the root choice all clear their
    bounds by M), other (the quadratic branch's other root; degree 3: the middle root where the smallest is the one returned; NaN
    elsewhere), branch (0 Cardano, 1 trigonometric, 2 quadratic root, 3 linear, -1 none) and the coefficients; cubic [m]: the objects
    with degree-3 terms.  mutate: "drop" leaves the product kz * dz out of t1, "f32" rounds t0 through float32 (degree <= 2), "hyz" and
    "t3term" are _cubic_pairs' (the mutation tests' wrong kernels)."""
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
        t, B, ok, other, root, lin = _quadlin(t2, t1, t0, e2, e1, e0)
        t3 = np.zeros_like(t)
        branch = np.where(root, 2, np.where(lin, 3, -1))
        if pixel_dirs:
            p = o[:, None, :] + t[:, :, None] * d[:, None, :]
            A = coefs[:, [10, 13, 14, 13, 11, 15, 14, 15, 12]].reshape(-1, 3, 3) * np.array([[2.0, 1, 1], [1, 2.0, 1], [1, 1, 2.0]])
            g = np.einsum("mij,nmj->nmi", A, p) + coefs[None, :, 16:19]
            slope = np.abs(2 * t2 * t + t1)
            B = B + np.where(root | lin, np.abs(t) * (np.abs(g) * (4 * U * np.abs(d))[:, None, :]).sum(axis=-1) / slope, 0.0)
        cubic = coefs[:, :10].any(axis=1)
        out = dict(t=t, B=B, ok=ok, other=other, t3=t3, t2=t2, t1=t1, t0=t0, branch=branch)
        if cubic.any():
            for name, v in _cubic_pairs(coefs[cubic], o, d, pixel_dirs, mutate).items():
                out[name][:, cubic] = v
        out["ok"] &= np.isfinite(out["t"]) & np.isfinite(out["B"])
        out["cubic"] = cubic
    return out


def _quadlin(t2, t1, t0, e2, e1, e0):
    """The reference's degree <= 2 rule on coefficients known to e2, e1, e0: (t, B, ok, other, root, lin) -- root / lin: which branch
    gave t (neither: -1)."""
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
    return t, B, ok, other, root, lin


def _expansion():
    """Per power of t the products of the expanded F(o + t d): (coefficient, integer factor, exponents of o, exponents of d)."""
    out = {0: [], 1: [], 2: [], 3: []}
    for at, (ex, ey, ez) in enumerate(MONO):
        for i in range(ex + 1):
            for j in range(ey + 1):
                for k in range(ez + 1):
                    out[i + j + k].append((at, _BINOM[ex][i] * _BINOM[ey][j] * _BINOM[ez][k], (ex - i, ey - j, ez - k), (i, j, k)))
    return out


_EXPANSION = _expansion()


def _gradient(q, p):
    """grad F at the points p [..., 3] for the coefficients q [..., 20] (broadcast against each other), degree 3 included."""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    c = [q[..., k] for k in range(20)]
    return np.stack([3 * c[0] * x * x + 2 * c[3] * x * y + 2 * c[5] * x * z + c[4] * y * y + c[6] * z * z + c[9] * y * z + 2 * c[10] * x + c[13] * y + c[14] * z + c[16],
                     3 * c[1] * y * y + 2 * c[4] * x * y + 2 * c[7] * y * z + c[3] * x * x + c[8] * z * z + c[9] * x * z + 2 * c[11] * y + c[13] * x + c[15] * z + c[17],
                     3 * c[2] * z * z + 2 * c[6] * x * z + 2 * c[8] * y * z + c[5] * x * x + c[7] * y * y + c[9] * x * y + 2 * c[12] * z + c[14] * x + c[15] * y + c[18]], axis=-1)


def _cubic_pairs(coefs, o, d, pixel_dirs, mutate):
    """pairs() for objects with degree-3 terms (the module's docstring, "DEGREE 3").  mutate: "hyz" leaves the product hyz dy dz out
    of the Taylor form's t2, "t3term" one degree-3 coefficient's term out of t3 (the mutation tests' wrong kernels)."""
    tk, ek = {}, {}
    for p, terms in _EXPANSION.items():
        mono = np.stack([np.prod(o ** np.array(eo), axis=1) * np.prod(d ** np.array(ed), axis=1) for _, _, eo, ed in terms], axis=1)
        w = coefs[:, [at for at, _, _, _ in terms]] * np.array([f for _, f, _, _ in terms], dtype=np.float64)
        if mutate == "t3term" and p == 3:
            w = w.copy()
            w[np.arange(len(w)), np.argmax(w != 0, axis=1)] = 0.0
        tk[p] = mono @ w.T
        ek[p] = (np.count_nonzero(w, axis=1) + 4) * U * (np.abs(mono) @ np.abs(w).T)
    if mutate == "hyz":   # hyz(o) = 2 y2z oy + 2 yz2 oz + xyz ox + yz
        hyz = 2 * np.outer(o[:, 1], coefs[:, 7]) + 2 * np.outer(o[:, 2], coefs[:, 8]) + np.outer(o[:, 0], coefs[:, 9]) + coefs[None, :, 15]
        tk[2] = tk[2] - hyz * (d[:, 1] * d[:, 2])[:, None]
    t3, t2, t1, t0 = tk[3], tk[2], tk[1], tk[0]
    e3, e2, e1, e0 = ek[3], ek[2], ek[1], ek[0]
    at3 = np.abs(t3)
    is3 = at3 > EPS
    ok3 = np.abs(at3 - EPS) > M * e3
    # ---- solve_poly's degree-3 branch, step by step: every operation is charged u of its result, every libm call 2u (one ulp) ----
    rel3 = e3 / at3
    a2, a1, a0 = t2 / t3, t1 / t3, t0 / t3
    ea2, ea1, ea0 = e2 / at3 + np.abs(a2) * (rel3 + U), e1 / at3 + np.abs(a1) * (rel3 + U), e0 / at3 + np.abs(a0) * (rel3 + U)
    sq = a2 * a2
    q = (3.0 * a1 - sq) / 9.0
    eq = (3 * ea1 + 2 * np.abs(a2) * ea2 + U * (3 * np.abs(a1) + sq + np.abs(3.0 * a1 - sq))) / 9 + U * np.abs(q)
    A, Bt, Cc = 9.0 * a2 * a1, 27.0 * a0, 2.0 * a2 * a2 * a2
    num = A - Bt - Cc
    r = num / 54.0
    er = (9 * (np.abs(a2) * ea1 + np.abs(a1) * ea2) + 27 * ea0 + 6 * sq * ea2 + U * (2 * np.abs(A) + np.abs(Bt) + 3 * np.abs(Cc) + np.abs(A - Bt) + np.abs(num))) / 54 + U * np.abs(r)
    q3, r2 = q * q * q, r * r
    delta = q3 + r2
    ed = 3 * q * q * eq + 2 * np.abs(r) * er + U * (2 * np.abs(q3) + r2 + np.abs(delta))
    ok3 &= ~is3 | (np.abs(delta) > M * ed)
    card = is3 & (delta > 0)
    trig = is3 & ~card
    third = a2 / 3.0
    e_third = ea2 / 3 + U * np.abs(third)
    # Cardano: cbrt(r + s) + cbrt(r - s) - a2 / 3
    s = np.sqrt(np.where(card, delta, 1.0))
    es = ed / (2 * s) + U * s
    P, Q = r + s, r - s
    cP, cQ = np.cbrt(P), np.cbrt(Q)
    ecP = (er + es + U * np.abs(P)) / (3 * cP * cP) + 2 * U * np.abs(cP)
    ecQ = (er + es + U * np.abs(Q)) / (3 * cQ * cQ) + 2 * U * np.abs(cQ)
    x_c = cP + cQ - third
    b_c = ecP + ecQ + e_third + U * np.abs(cP + cQ) + U * np.abs(x_c)
    # trigonometric: 2 sqrt(-q) cos(acos(r / sqrt(-q^3)) / 3 + 2 k pi / 3) - a2 / 3
    v = np.where(trig, -q3, 1.0)
    sv = np.sqrt(v)
    esv = (3 * q * q * eq + 2 * U * np.abs(q3)) / (2 * sv) + U * sv
    arg = r / sv
    earg = er / sv + np.abs(arg) * (esv / sv + U)
    th3 = np.arccos(np.clip(arg, -1.0, 1.0))
    eth3 = earg / np.sqrt(np.where(trig, -delta / v, 1.0)) + 2 * U * th3      # 1 - arg^2 = -delta / (-q^3), without the cancellation
    th = th3 / 3.0
    eth = eth3 / 3 + U * th
    mq = np.where(trig, -q, 1.0)
    c = 2.0 * np.sqrt(mq)
    ec = eq / np.sqrt(mq) + U * c
    xs, es3 = [], []
    for k in range(3):
        phi = th + k * TWO_THIRD_PI
        ephi = eth + U * np.abs(phi) + k * U * TWO_THIRD_PI                    # (the constant is itself a rounded 2 pi / 3)
        cs = np.cos(phi)
        x = c * cs - third
        xs.append(x)
        es3.append(np.abs(cs) * ec + c * (np.abs(np.sin(phi)) * ephi + 2 * U * np.abs(cs)) + U * np.abs(c * cs) + e_third + U * np.abs(x))
    x_t, b_t = xs[0], es3[0]
    ok_t = np.ones_like(is3)
    for k in (1, 2):
        ok_t &= np.abs(xs[k] - EPS) > M * es3[k]
        ok_t &= (xs[k] < EPS) | (np.abs(xs[k] - x_t) > M * (es3[k] + b_t))       # the comparison x1 < x, where it is made
        take = (xs[k] >= EPS) & (xs[k] < x_t)
        x_t, b_t = np.where(take, xs[k], x_t), np.where(take, es3[k], b_t)
    ok3 &= ~trig | ok_t
    srt = np.sort(np.stack(xs, axis=0), axis=0)
    other3 = np.where(trig & (srt[0] >= EPS), srt[1], np.nan)                  # the middle root where the smallest is the one returned
    # ---- |t3| <= EPS: the degree <= 2 rule on t2, t1, t0 ----
    t_q, b_q, ok_q, other_q, root, lin = _quadlin(t2, t1, t0, e2, e1, e0)
    t = np.where(card, x_c, np.where(trig, x_t, t_q))
    B = np.where(card, b_c, np.where(trig, b_t, b_q))
    ok = ok3 & (is3 | ok_q)
    if pixel_dirs:
        pt = o[:, None, :] + t[:, :, None] * d[:, None, :]
        slope = np.abs(np.where(is3, 3 * t3 * t * t, 0.0) + 2 * t2 * t + t1)
        B = B + np.where(is3 | root | lin, np.abs(t) * (np.abs(_gradient(coefs[None, :, :], pt)) * (4 * U * np.abs(d))[:, None, :]).sum(axis=-1) / slope, 0.0)
    return dict(t=t, B=B, ok=ok, other=np.where(is3, other3, other_q), t3=t3, t2=t2, t1=t1, t0=t0, branch=np.where(card, 0, np.where(trig, 1, np.where(root, 2, np.where(lin, 3, -1)))))


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
        # (cubic_guarded does not protect comparisons between objects: a guarded root may be CUB_TOL of its value off the reference's)
        loose = np.where(pr["cubic"][None, :] | (hit & pr["cubic"][win])[:, None], CUB_TOL * (np.abs(t) + np.abs(tw[:, None])), 0.0)
        gap = ~acc | (np.abs(t - tw[:, None]) > M * (B + bw[:, None]) + loose)
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
    g = _gradient(q, p)
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


def check_closest(osc, rays, got, what="", pixel_dirs=False, stop_at_first=False, guarded=False):
    """A Report on closest-hit results `got` (a mapping with "object", "t" and optionally "point" [n, 3] and "normal" [n, >= 3]) for the
    rays against truth: on every decided ray `object` is the winner, |t - t_exact| <= B (a miss: +inf; + CUB_TOL |t_exact| for a winner of
    degree 3 where `guarded` -- a flag or one per ray -- says that cubic_guarded may have answered), point[i] within
    2u(|o_i| + |t d_i|) of o_i + t d_i with the reported t, every normal component within exact_normal's bound of the exact normal at the
    reported point (without "point": at o + t d in float64).  Undecided rays are counted, not judged.  stop_at_first: return at the
    first failure (the mutation tests only ask whether there is one)."""
    coefs = _coefs(osc)
    win, _, B, decided = decided_closest(osc, rays, pixel_dirs)
    rep = Report(what, len(rays), (~decided).sum())
    cubic = coefs[:, :10].any(axis=1)
    guarded = np.broadcast_to(np.asarray(guarded, dtype=bool), (len(rays),))
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
            bar = mpmath.mpf(float(B[i])) + (CUB_TOL * abs(te) if cubic[k] and guarded[i] else 0)
            rho = float(abs(mpmath.mpf(float(t[i])) - te) / bar) if np.isfinite(t[i]) else np.inf
            rep.worst_rho = max(rep.worst_rho, rho)
            if not rho <= 1.0:
                rep.fail(f"ray {i} (o {o.tolist()}, d {d.tolist()}), object {k}: t {float(t[i])!r}, exact {mpmath.nstr(te, 25)}, bar {float(bar):.3e}, rho {rho:.3g}")
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


def check_pairs(coefs, rays, t_pairs, what="", guarded=False, stop_at_first=False):
    """A Report on per-pair roots t_pairs [n, m] (what a solver returns for ray i against object k alone): on every decided pair with
    an object of degree 3, |t - t_exact| <= B (+ CUB_TOL |t_exact| where guarded [n, m] says so).  n counts pairs."""
    coefs = np.ascontiguousarray(coefs, dtype=np.float64).reshape(-1, 20)
    pr = pairs(coefs, rays["o"], rays["d"])
    judged = pr["ok"] & pr["cubic"][None, :]
    guarded = np.broadcast_to(np.asarray(guarded, dtype=bool), judged.shape)
    rep = Report(what, int(pr["cubic"].sum()) * len(rays), (~judged[:, pr["cubic"]]).sum())
    for i, k in np.argwhere(judged).tolist():
        if stop_at_first and rep.failures:
            break
        te = exact_t(coefs[k], rays["o"][i], rays["d"][i])
        bar = mpmath.mpf(float(pr["B"][i, k])) + (CUB_TOL * abs(te) if guarded[i, k] else 0)
        rho = float(abs(mpmath.mpf(float(t_pairs[i, k])) - te) / bar)
        rep.worst_rho = max(rep.worst_rho, rho)
        if not rho <= 1.0:
            rep.fail(f"ray {i} (o {rays['o'][i].tolist()}, d {rays['d'][i].tolist()}), object {k}, branch {int(pr['branch'][i, k])}: t {float(t_pairs[i, k])!r}, "
                     f"exact {mpmath.nstr(te, 25)}, bar {float(bar):.3e}, rho {rho:.3g}")
    return rep


# ---- the test sets -----------------------------------------------------------------------------------------------------------------------------
# degree 3: query sets of 1 024 rays, frames of 32 x 24 at depth 2 (bent65: 64 x 48, closest hits and planes only)
CUBIC_N_RAYS = 1024
CUBIC_SCENES = ("bent8", "bent8 mixed", "bent65", "clebsch")
CUBIC_FRAME_SCENES = ("bent8", "bent8 mixed")
CLEBSCH_POSE = (0.3, 0.2, -4.0)    # outside the surface, looking down +z
# The frames' fields: with seed 1 the reference alone leaves 4 of the 768 paths undecided (0.52 %: shadow rays whose far negative
# Cardano roots carry a B3 above |t| / M), which is over the cap; 25 is the first seed of 1 .. 80 that leaves none (28 the next).
CUBIC_FRAME_SEED = 25


def cubic_scene(name, frame=False):
    """The oracle scene of a degree-3 set.  bent8: tests/tools/cubic_field_scenes.py's field of 8 bent ellipsoids at 32 x 24 (more
    than the RT_CUB_AT_MAX = 4 records the host forms, mirrors, both light kinds); bent8 mixed: the same plus 8 spheres and an
    ellipsoid with cross terms; bent65: 65 of them at 64 x 48 (one entry past the streamed 64-entry chunk); clebsch: scenes/clebsch.yml
    (its camera is not used: the rays come from cubic_query_rays).  frame: the field of CUBIC_FRAME_SEED, for whole paths."""
    import cubic_field_scenes as CF
    seed = CUBIC_FRAME_SEED if frame else 1
    if name == "bent8":
        return CF.cubic_field(n=8, seed=seed, w=32, h=24)
    if name == "bent8 mixed":
        return CF.cubic_field(n=8, seed=seed, w=32, h=24, spheres=8, with_quadric=True)
    if name == "bent65":
        return CF.cubic_field(n=65, seed=1, w=64, h=48)
    assert name == "clebsch"
    return CF.O.load_scene(os.path.join(rays_ref.ROOT, "scenes", "clebsch.yml")).with_size(32, 24)


def cone_rays(pos, half_angle_deg, rows, cols):
    """rows x cols rays from pos, looking down +z, spread evenly (in tangent) over +-half_angle_deg; unit directions."""
    k = np.tan(np.radians(half_angle_deg))
    y, x = np.meshgrid(np.linspace(k, -k, rows), np.linspace(-k, k, cols), indexing="ij")
    dirs = np.stack([x, y, np.ones_like(x)], axis=-1).reshape(-1, 3)
    return rays_ref.make_rays(np.broadcast_to(np.asarray(pos, dtype=np.float64), dirs.shape), dirs / np.linalg.norm(dirs, axis=1)[:, None])


def cubic_query_rays(osc, name, seed=41, n=CUBIC_N_RAYS):
    """n rays of a degree-3 set: a grid of primary rays (a quarter to a half of them), the rest aimed as query_rays aims them -- from
    outside a body, from inside, away from it, across the field; direction lengths 0.5 .. 2."""
    rng = np.random.default_rng(seed)
    if name == "clebsch":
        first, bodies, box = cone_rays(CLEBSCH_POSE, 25.0, 24, 16), [(np.zeros(3), 1.5)], (np.full(3, -4.0), np.full(3, 4.0))
    else:
        first = rays_ref.primary_rays(osc, rows=np.linspace(0, osc.height - 1, 16).astype(np.int64), cols=np.linspace(0, osc.width - 1, 32).astype(np.int64))
        bodies, box = osc.bodies, (np.array([-12.0, -9, 0]), np.array([12.0, 9, 32]))
    out = np.zeros(n, dtype=rays_ref.RAY_DTYPE)
    out[:len(first)] = first
    for i in range(len(first), n):
        c, r = bodies[int(rng.integers(len(bodies)))]
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
            o = rng.uniform(*box)
            dvec = rng.uniform(*box) - o
        out["o"][i] = o
        out["d"][i] = dvec / np.linalg.norm(dvec) * rng.uniform(0.5, 2.0)
    return out


# degree <= 2: query sets of 2 048 rays, frames of 96 x 72
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
