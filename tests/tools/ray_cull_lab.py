#!/usr/bin/env python3
"""Host lab behind RT_FLAG_STREAM_CULL_RAYS (tests/tools/ray_cull_lab.cpp).  No GPU.
The predicate and the construction are bounce_cull_lab's (rtm::ray_reaches about a packed chunk bound, a member grazed by ONE ray at relative
clearances +-1e-1 ... +-1e-15); this lab adds the rays a bounce never forms but a caller can hand in:
  * `far`            the origin 1e3 .. 1e6 member radii away from a chunk at most 1e2 radii wide, aimed at a member's rim
  * `inside_member`  the origin inside a member of the chunk
  * `behind_near`    the whole chunk behind the origin, its nearest member less than a radius behind it
  * `occlusion`      the rim family under rt_occluded_rays' rule: t_max at 0.9 .. 1.1 of the grazed member's root (a few +inf and NaN)
Unsound = the bound is skipped although orc_intersect_ray gives some member a root with t >= EPS && t < MAX_T (occlusion: t > EPS &&
t < t_max).  `ray_stats_expectation`: what the work words of the GPU statistics test must be, from the rays alone.
usage: python tests/tools/ray_cull_lab.py [n]      n verdicts per family (default 100000: the full count)"""
import ctypes as C
import functools
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOOLS = os.path.join(ROOT, "tests", "tools")
sys.path.insert(0, ROOT)
sys.path.insert(0, TOOLS)
import bounce_cull_lab as B  # noqa: E402
import cull_lab as L  # noqa: E402
import stream_cull_lab as SC  # noqa: E402

FAMILIES = ("far", "inside_member", "behind_near", "occlusion")
N_COMP = SC.N_COMP
ORDERS = ("row", "block", "shuffled")

_LIB = {}


def build(variant="strict"):
    """bounce_cull_lab's two builds of this lab's file: strict (everything here uses it) and contracted (lab_bounce_eval alone)."""
    if variant not in _LIB:
        L.build()   # (the oracle's library)
        out = os.path.join(TOOLS, "bin", "libray_cull_lab.so" if variant == "strict" else "libray_cull_lab_fast.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2"] + B.VARIANT[variant] + ["-Wno-subobject-linkage", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tools", "flopcount_shim"),
                        "-I" + os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-I" + TOOLS,
                        os.path.join(TOOLS, "ray_cull_lab.cpp"), "-o", out, "-L" + os.path.join(ROOT, "oracle"), "-lrt_oracle",
                        "-Wl,-rpath," + os.path.join(ROOT, "oracle")], check=True)
        lib = C.CDLL(out)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        lib.lab_bounce.argtypes = [C.c_uint64, dp, C.c_int, dp, dp, ip, ip, ip, ip, dp]
        lib.lab_bounce_eval.argtypes = [C.c_uint64, dp, ip]
        lib.lab_ray_occluded.argtypes = [C.c_uint64, dp, C.c_int, dp, dp, dp, ip, ip]
        _LIB[variant] = lib
    return _LIB[variant]


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


# ---- the generator -------------------------------------------------------------------------------------------------------------------
def ray_params(n, seed, family):
    """[n, B.BR_W] parameters of lab_bounce.  bounce_cull_lab.ray_params' scales, origins and directions; what differs per family is where
    the grazed member lies along the ray."""
    base = "behind" if family == "behind_near" else "rim"
    par = B.ray_params(n, 7000 + seed + 13 * FAMILIES.index(family), base)
    rng = np.random.default_rng(560000 + seed + 17 * FAMILIES.index(family))
    r = par[:, 6]
    dn = np.linalg.norm(par[:, 3:6], axis=1)
    if family == "far":            # the tangent point 1e3 .. 1e6 member radii ahead
        par[:, 8] = r * 10.0 ** rng.uniform(3, 6, n) / dn
    elif family == "behind_near":  # the member's nearest point 1e-6 .. 1 radii behind the plane through the origin, its centre up to 0.9 r off the line
        par[:, 8] = -r * (1.0 + 10.0 ** rng.uniform(-6, 0, n)) / dn
        par[:, 7] = 0.0
    return par


def companions(family, par, centre, seed):
    """[n, N_COMP, 4] companions (centre, radius) of the grazed member."""
    n = len(par)
    rng = np.random.default_rng(570000 + seed)
    r, o = par[:, 6], par[:, 0:3]
    if family == "far":            # a chunk at most 1e2 radii wide: half of them exactly away from the ray's line, so that the bound touches the member where the ray passes
        out = centre - (o + par[:, 8:9] * par[:, 3:6])
        rnd = SC._unit(rng.normal(size=(n, 3)))
        d = np.where(((out * out).sum(axis=1, keepdims=True) > 0) & (rng.random((n, 1)) < 0.5), SC._unit(np.where((out * out).sum(axis=1, keepdims=True) > 0, out, rnd)), rnd)
        far = centre + (r * 10.0 ** rng.uniform(0, 2, n))[:, None] * d
        comp = np.zeros((n, N_COMP, 4))
        comp[:, 0, :3], comp[:, 0, 3] = far, r * 10.0 ** rng.uniform(-1, 0, n)
        for k in range(1, N_COMP):
            comp[:, k, :3] = centre + rng.uniform(0, 1, (n, 1)) * (far - centre) + (r * rng.uniform(0, 1, n))[:, None] * SC._unit(rng.normal(size=(n, 3)))
            comp[:, k, 3] = r * 10.0 ** rng.uniform(-1, 0, n)
        return comp
    if family == "behind_near":
        return B.companions("behind", par, centre, 7000 + seed)
    comp = B.companions("rim", par, centre, 7000 + seed)
    if family == "inside_member":  # the origin 0 .. 0.999 radii from the centre of one member
        comp[:, 1, :3] = o + (comp[:, 1, 3] * rng.uniform(0, 0.999, n))[:, None] * SC._unit(rng.normal(size=(n, 3)))
    return comp


def t_max_factors(n, seed):
    rng = np.random.default_rng(580000 + seed)
    f = rng.uniform(0.9, 1.1, n)
    pick = rng.random(n)
    f[pick < 0.02] = np.inf
    f[(pick >= 0.02) & (pick < 0.04)] = np.nan
    f[(pick >= 0.04) & (pick < 0.08)] = 1.0 + rng.choice([-1.0, 1.0], int(((pick >= 0.04) & (pick < 0.08)).sum())) * 2.0 ** -52
    return f


def cases(family, n, seed):
    """One batch: (records [n, REC_SH], verdicts, truth, parameters, t_max or None, members [n, N_COMP + 1, 5], the half-line's truth)."""
    lib = build()
    par = np.ascontiguousarray(ray_params(n, seed, family))
    comp = np.ascontiguousarray(companions(family, par, B.graze_centre(par), seed))
    rec = np.zeros((n, B.REC_SH))
    v, t, g, alone = (np.zeros(n, np.int32) for _ in range(4))
    members = np.zeros((n, N_COMP + 1, 5))
    lib.lab_bounce(n, L._dp(par), N_COMP, L._dp(comp), L._dp(rec), _ip(v), _ip(t), _ip(g), _ip(alone), L._dp(members))
    t_max, half = None, t
    if family == "occlusion":      # the same bounds and rays under the occlusion rule
        f = np.ascontiguousarray(t_max_factors(n, seed))
        t_max, vo, to = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
        lib.lab_ray_occluded(n, L._dp(par), N_COMP, L._dp(comp), L._dp(f), L._dp(t_max), _ip(vo), _ip(to))
        assert np.array_equal(vo, v)                 # (the verdict never sees t_max)
        assert not ((to != 0) & (half == 0) & (t_max <= 1e6)).any()   # (what t < t_max <= MAX_T accepts, the nearest-hit rule accepts; beyond
        # MAX_T -- t_max = +inf -- an occlusion query accepts roots that rule does not, and the verdict, being about the half-line, has to cover them)
        t = to
    return rec, v, t, par, t_max, members, half


def run_family(family, n, chunk=20000):
    """n verdicts of one family: dict(family, cases, culled, accepted, unsound, origin_inside_skipped, repeat_differs, fast_cases, fast_unsound,
    fast_differs, limited: occlusion cases whose finite t_max lies below a root the half-line accepts)."""
    row = dict(family=family, cases=0, culled=0, accepted=0, unsound=0, origin_inside_skipped=0, repeat_differs=0, fast_cases=0, fast_unsound=0, fast_differs=0, limited=0)
    done = seed = 0
    while done < n:
        k = min(chunk, n - done)
        rec, v, t, par, t_max, members, half = cases(family, k, seed)
        if seed == 0:       # two runs agree
            rec2, v2, t2 = cases(family, k, seed)[:3]
            row["repeat_differs"] += int(rec.tobytes() != rec2.tobytes()) + int((v != v2).sum() + (t != t2).sum())
        assert (rec[:, 25] == 1.0).all()       # (every generated ray can be culled for)
        row["cases"] += k
        row["culled"] += int((v == 0).sum())
        row["accepted"] += int((t != 0).sum())
        row["unsound"] += int(((v == 0) & (t != 0)).sum())
        bc, br = -0.5 * rec[:, 0:3], rec[:, 4]
        row["origin_inside_skipped"] += int(((v == 0) & np.isfinite(br) & (np.linalg.norm(rec[:, 6:9] - bc, axis=1) < br)).sum())
        if family == "occlusion":
            row["limited"] += int(((half != 0) & (t == 0) & np.isfinite(t_max)).sum())
        if family == "inside_member":      # (members[0] is the grazed one, the companions follow; a member's radius is the one its coefficients
            # give back, which at |centre| / r ~ 1e8 is not the radius that went in: a few origins in a thousand end up outside)
            assert (np.linalg.norm(members[:, 2, :3] - par[:, 0:3], axis=1) < members[:, 2, 3]).mean() > 0.99
        if B.host_has_fma():      # the predicate as the FAST build contracts it, about the same bounds and truths
            vf = np.zeros(k, np.int32)
            build("fast").lab_bounce_eval(k, L._dp(np.ascontiguousarray(rec)), _ip(vf))
            row["fast_unsound"] += int(((vf == 0) & (t != 0)).sum())
            row["fast_differs"] += int((vf != v).sum())
            row["fast_cases"] += k
        done += k
        seed += 1
    return row


# ---- the statistics test ------------------------------------------------------------------------------------------------------------------
def ordered(rays, w, h, order):
    """The frame's rays in row order, in 8 x 8 block order (block after block, rows inside a block), or shuffled (a fixed seed)."""
    idx = np.arange(w * h)
    if order == "block":
        y, x = idx // w, idx % w
        idx = np.lexsort((x % 8, y % 8, x // 8, y // 8))
    elif order == "shuffled":
        idx = np.random.default_rng(29).permutation(w * h)
    else:
        assert order == "row"
    return np.ascontiguousarray(rays[idx])


def ray_stats_expectation(pkg, sc, order="row"):
    """The primary rays of sc's frame as caller-supplied rays, a wave being 64 consecutive rays: D = waves x chunks; L = the (wave, chunk)
    pairs for which no lane's half-line comes within 1.01 r + 0.1 of the bound's centre (bounce_cull_lab.stats_expectation's rule;
    float64 here, the margin dwarfs its rounding).  Returns dict(D, L, n_chunks, waves, rays: the ordered rays)."""
    import rays_ref
    import stream_scenes as S
    a = sc.arrays()
    w, h = a["width"], a["height"]
    assert (w * h) % 64 == 0
    osc = S.oracle_of(pkg, sc)
    rays = ordered(np.ascontiguousarray(rays_ref.primary_rays(osc)).reshape(-1), w, h, order)
    _, bounds, _ = SC.image(a)
    b = bounds.view(SC.US_DTYPE)
    centre, reach = -0.5 * b["k"], 1.01 * b["r"] + 0.1
    assert np.isfinite(b["r"]).all()
    D = Lo = 0
    for wave in range(len(rays) // 64):
        o, d = rays["o"][64 * wave:64 * wave + 64], rays["d"][64 * wave:64 * wave + 64]
        for c in range(len(b)):
            D += 1
            v = centre[c] - o
            t = np.maximum((v * d).sum(axis=1) / (d * d).sum(axis=1), 0.0)
            dist = np.linalg.norm(o + t[:, None] * d - centre[c], axis=1)
            Lo += int((dist > reach[c]).all())
    return dict(D=D, L=Lo, n_chunks=len(b), waves=len(rays) // 64, rays=rays)


@functools.lru_cache(maxsize=None)
def expectation(order="row"):
    """ray_stats_expectation of bounce_cull_lab.bounce_scene, once per process and order (the host test and the GPU test share it)."""
    import __graft_entry__ as graft
    pkg = graft.load_package()
    return ray_stats_expectation(pkg, B.bounce_scene(pkg), order)


def format_row(r):
    return (f"ray_reaches {r['family']:14s} cases {r['cases']:7d}  culled {r['culled']:7d}  oracle accepts a member {r['accepted']:7d}  unsound {r['unsound']}  "
            f"origin inside, skipped {r['origin_inside_skipped']}  t_max cut a root {r['limited']}  repeat differs {r['repeat_differs']}  contracted build: "
            f"{r['fast_cases']} cases, {r['fast_differs']} verdicts differ, unsound {r['fast_unsound']}")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    t0 = time.time()
    rows = []
    for family in FAMILIES:
        rows.append(run_family(family, n))
        print(format_row(rows[-1]), flush=True)
    for order in ORDERS:
        e = expectation(order)
        print(f"statistics scene, {order:8s} order: D = {e['D']}, L = {e['L']}")
    bad = sum(r["unsound"] + r["origin_inside_skipped"] + r["repeat_differs"] + r["fast_unsound"] for r in rows)
    print(f"ray_cull_lab: {sum(r['cases'] for r in rows)} verdicts, {sum(r['unsound'] for r in rows)} unsound, {time.time() - t0:.0f} s")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
