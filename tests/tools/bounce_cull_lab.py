#!/usr/bin/env python3
"""Host lab behind RT_FLAG_STREAM_CULL_BOUNCE (tests/tools/bounce_cull_lab.cpp).  No GPU.
  * `cases` / `run`: rtm::ray_reaches (csrc/rt_ray_bound.hpp) asked about the bound of a chunk that holds a sphere grazed by ONE ray -- relative
    clearances +-1e-1 ... +-1e-15, radii 1e-4 ... 10 scales, translations to 1e7, |d| from 1e-3 to 1e3 -- and companions up to 1e5 radii away
    (stream_cull_lab's families `rim` and `any`), plus the families a bounce ray brings: the origin 1e-2 above a member (`on_member`), the
    origin inside the bound (`inside`), the grazed member wholly behind the origin or just not (`behind`).  The truth is the oracle's verdict
    for every member; unsound = the bound is skipped although the oracle accepts a member.  Tightness: stream_cull_lab's band.
  * `never_culled`: rays nothing may be culled for.
  * `bounce_scene`, `stats_expectation`: the scene of the GPU statistics test and what the oracle's rays say its work words must be.
usage: python tests/tools/bounce_cull_lab.py [n]      n verdicts per family (default 100000: the full count)"""
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
import cull_lab as L  # noqa: E402
import stream_cull_lab as SC  # noqa: E402

BR_W = 12
REC_SH = L.REC["sh"]
FAMILIES = ("rim", "any", "on_member", "inside", "behind")
N_COMP = SC.N_COMP
BIAS = 1e-2

_LIB = {}
VARIANT = {"strict": ["-ffp-contract=off"], "fast": ["-mfma", "-ffp-contract=fast", "-DRT_FAST=1"]}


def host_has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read().replace("\n", " ")
    except OSError:
        return False


def build(variant="strict"):
    """The lab as the strict kernel build compiles the predicate (everything here uses this one) -- or, variant "fast", a second build
    with contraction on, of which only lab_bounce_eval is called (eval_records)."""
    if variant not in _LIB:
        L.build()   # (the oracle's library)
        out = os.path.join(TOOLS, "bin", "libbounce_cull_lab.so" if variant == "strict" else "libbounce_cull_lab_fast.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2"] + VARIANT[variant] + ["-Wno-subobject-linkage", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tools", "flopcount_shim"),
                        "-I" + os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-I" + TOOLS,
                        os.path.join(TOOLS, "bounce_cull_lab.cpp"), "-o", out, "-L" + os.path.join(ROOT, "oracle"), "-lrt_oracle",
                        "-Wl,-rpath," + os.path.join(ROOT, "oracle")], check=True)
        lib = C.CDLL(out)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        lib.lab_bounce.argtypes = [C.c_uint64, dp, C.c_int, dp, dp, ip, ip, ip, ip, dp]
        lib.lab_bounce_verdicts.argtypes = [C.c_uint64, dp, dp, ip]
        lib.lab_bounce_eval.argtypes = [C.c_uint64, dp, ip]
        _LIB[variant] = lib
    return _LIB[variant]


def eval_records(rec, variant):
    """ray_reaches about every record's bound and ray, by the given build of the predicate."""
    rec = np.ascontiguousarray(rec)
    v = np.zeros(len(rec), np.int32)
    build(variant).lab_bounce_eval(len(rec), L._dp(rec), v.ctypes.data_as(C.POINTER(C.c_int32)))
    return v


# ---- the generator -------------------------------------------------------------------------------------------------------------------
def ray_params(n, seed, family, wide=False):
    """[n, BR_W] parameters of lab_bounce: scene scales 1e-2 .. 1e6, origins up to 1e7 away, radii 1e-4 .. 10 scales, directions of any
    orientation (a third nearly along an axis) and length 1e-3 .. 1e3, the tangent point 1e-2 .. 1e2 scales along the ray (15 % behind the
    origin).  `behind`: the grazed sphere's far side a relative clearance behind (or across) the plane through the origin.  wide: the ray
    misses the grazed sphere by 1e-3 .. 10 of the predicate's distance scale instead (the tightness sample: half of these lie beyond the band)."""
    rng = np.random.default_rng(540000 + seed + 11 * FAMILIES.index(family))
    par = np.zeros((n, BR_W))
    scale = 10.0 ** rng.uniform(-2, 6, n)
    par[:, 0:3] = rng.normal(size=(n, 3)) * np.where(rng.random(n) < 0.2, 0.0, 10.0 ** rng.uniform(0, 7, n))[:, None]
    d = rng.normal(size=(n, 3))
    axis = rng.random(n) < 1 / 3
    e = np.zeros((n, 3))
    e[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    d = np.where(axis[:, None], e + rng.normal(size=(n, 3)) * (10.0 ** (-rng.integers(1, 12, n).astype(float)))[:, None], d)
    dn = 10.0 ** rng.uniform(-3, 3, n)
    par[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True) * dn[:, None]
    r = scale * 10.0 ** rng.uniform(-4, 1, n)
    delta = L._clearance(rng, n)
    dist = scale * 10.0 ** rng.uniform(-2, 2, n) * np.where(rng.random(n) < 0.85, 1.0, -1.0)
    f = np.ones(n)
    if wide:
        delta = 10.0 ** rng.uniform(-3, 1, n) * (np.abs(dist) + r + 1.0) / r
    if family == "behind":
        f = rng.uniform(0.0, 0.9, n)
        dist = -r * (1.0 + delta)
    par[:, 6], par[:, 7], par[:, 8], par[:, 9], par[:, 10] = r, (0.0 if family == "behind" else delta), dist / dn, rng.uniform(0, 2 * np.pi, n), f
    par[:, 11] = delta   # (`behind`: the clearance acts along the ray, not around it)
    return par


def graze_centre(par):
    """The grazed sphere's centre as lab_bounce forms it (to rounding: it only places the companions)."""
    o, d, r, delta, s, phi, f = par[:, 0:3], par[:, 3:6], par[:, 6], par[:, 7], par[:, 8], par[:, 9], par[:, 10]
    dn = np.linalg.norm(d, axis=1)
    a = np.where((np.abs(d[:, 0]) < 0.5 * dn)[:, None], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    u = np.cross(d, a)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(d, u) / dn[:, None]
    return o + s[:, None] * d + (f * r * (1.0 + delta))[:, None] * (np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * v)


def companions(family, par, centre, seed):
    """stream_cull_lab.companions for the ray as a directional "light" from a ball of radius 0, then the family's own member."""
    n = len(par)
    rec = np.zeros((n, REC_SH))
    rec[:, 6:9], rec[:, 16:19] = par[:, 0:3], par[:, 3:6]
    fake = np.zeros((n, 8))
    fake[:, 4] = par[:, 6]
    comp = SC.companions("sh_dir", "rim" if family in ("rim", "behind") else "any", rec, fake, centre, seed)
    rng = np.random.default_rng(550000 + seed)
    o = par[:, 0:3]
    if family == "on_member":      # the ray leaves a member: its origin is 1e-2 above that member's surface, along the normal there
        nrm = SC._unit(rng.normal(size=(n, 3)))
        comp[:, 1, :3] = o - (comp[:, 1, 3] + BIAS)[:, None] * nrm
    elif family == "inside":       # the far companion opposite the grazed sphere: the bound's centre lies next to the origin
        comp[:, 0, :3] = 2.0 * o - centre + (par[:, 6] * rng.uniform(0, 1, n))[:, None] * SC._unit(rng.normal(size=(n, 3)))
    elif family == "behind":       # the whole chunk behind the origin: the far companion 1 .. 1e3 radii further back, the others between
        r = par[:, 6]
        back = -SC._unit(par[:, 3:6])
        comp[:, 0, :3] = centre + (r * 10.0 ** rng.uniform(0, 3, n))[:, None] * back + (r * rng.uniform(0, 1, n))[:, None] * SC._unit(rng.normal(size=(n, 3)))
        for k in range(1, N_COMP):
            comp[:, k, :3] = centre + rng.uniform(0, 1, (n, 1)) * (comp[:, 0, :3] - centre) + (r * rng.uniform(0, 0.5, n))[:, None] * SC._unit(rng.normal(size=(n, 3)))
    return comp


def cases(family, n, seed, wide=False):
    """One batch: (records [n, REC_SH], verdicts, oracle accepts some member, ... the grazed one, ray_reaches about the grazed sphere alone,
    members [n, N_COMP + 1, 5], parameters)."""
    lib = build()
    par = np.ascontiguousarray(ray_params(n, seed, family, wide))
    comp = np.ascontiguousarray(companions(family, par, graze_centre(par), seed))
    rec = np.zeros((n, REC_SH))
    v, t, g, alone = (np.zeros(n, np.int32) for _ in range(4))
    members = np.zeros((n, N_COMP + 1, 5))
    ip = C.POINTER(C.c_int32)
    lib.lab_bounce(n, L._dp(par), N_COMP, L._dp(comp), L._dp(rec), v.ctypes.data_as(ip), t.ctypes.data_as(ip), g.ctypes.data_as(ip), alone.ctypes.data_as(ip),
                   L._dp(members))
    return rec, v, t, g, alone, members, par


def run_family(family, n, chunk=20000, sample=400):
    """n verdicts of one family: dict(family, cases, culled, accepted, g_accepted, unsound, member_kept_bound_skipped, not_enclosed, inv_r_short,
    beyond, kept, repeat_differs)."""
    row = dict(family=family, cases=0, culled=0, accepted=0, g_accepted=0, unsound=0, member_kept_bound_skipped=0, not_enclosed=0, inv_r_short=0, beyond=0, kept=0,
               repeat_differs=0, origin_inside_skipped=0, fast_unsound=0, fast_differs=0, fast_cases=0)
    done = seed = 0
    while done < n:
        k = min(chunk, n - done)
        rec, v, t, g, alone, members, _ = cases(family, k, seed)
        if seed == 0:       # two runs agree
            rec2, v2, t2, _, alone2, _, _ = cases(family, k, seed)
            row["repeat_differs"] += int(rec.tobytes() != rec2.tobytes()) + int((v != v2).sum() + (t != t2).sum() + (alone != alone2).sum())
        assert (rec[:, 25] == 1.0).all()       # (every generated ray can be culled for)
        row["cases"] += k
        row["culled"] += int((v == 0).sum())
        row["accepted"] += int((t != 0).sum())
        row["g_accepted"] += int((g != 0).sum())
        row["unsound"] += int(((v == 0) & (t != 0)).sum())
        assert np.array_equal(eval_records(rec, "strict"), v)
        if host_has_fma():      # the predicate as the FAST build contracts it, about the same bounds and truths
            vf = eval_records(rec, "fast")
            row["fast_unsound"] += int(((vf == 0) & (t != 0)).sum())
            row["fast_differs"] += int((vf != v).sum())
            row["fast_cases"] += k
        row["member_kept_bound_skipped"] += int(((v == 0) & (alone != 0)).sum())      # (the bound's verdict covers the member's own)
        bc, br, bq = -0.5 * rec[:, 0:3], rec[:, 4], rec[:, 5]
        fin = np.isfinite(br)
        reach = (np.linalg.norm(members[:, :, :3] - bc[:, None, :], axis=2) + members[:, :, 3]).max(axis=1)
        row["not_enclosed"] += int((fin & (br < reach)).sum())
        row["inv_r_short"] += int((fin & (bq < members[:, :, 4].max(axis=1))).sum())
        row["origin_inside_skipped"] += int(((v == 0) & fin & (np.linalg.norm(rec[:, 6:9] - bc, axis=1) < br)).sum())     # (an origin inside the bound reaches it)
        _, _, b, kb = SC.kept_beyond_band("sh_dir", rec, v, sample=max(1, sample * k // n), seed=seed)
        row["beyond"] += b
        row["kept"] += kb
        if seed == 0 and family in ("rim", "any"):       # the tightness sample proper: rays that miss by about the band's width
            wrec, wv = cases(family, min(k, 2000), seed, wide=True)[:2]
            _, _, b, kb = SC.kept_beyond_band("sh_dir", wrec, wv, sample=sample, seed=seed)
            row["beyond"] += b
            row["kept"] += kb
            if host_has_fma():
                row["kept"] += SC.kept_beyond_band("sh_dir", wrec, eval_records(wrec, "fast"), sample=sample, seed=seed)[3]
        done += k
        seed += 1
    return row


def never_culled(variant="strict"):
    """(verdicts for rays nothing may be culled for, verdict for an ordinary ray pointing away): one bound, far from every origin."""
    lib = build(variant)
    bound = np.array([-2.0 * 50.0, 0.0, 0.0, 1.0, 1.0])     # centre (50, 0, 0), r = 1
    away = [0.0, 0.0, 0.0, -1.0, 0.0, 0.0]
    odd = [[0, 0, 0, -3e-4, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, -1e-4, -1e-4, 2e-4], [0, 0, 0, -np.nan, 0, 0], [0, 0, 0, -1, np.inf, 0], [0, 0, 0, -1, 0, -np.inf],
           [np.nan, 0, 0, -1, 0, 0], [0, np.inf, 0, -1, 0, 0], [0, 0, 2e100, -1, 0, 0], [-2e100, 0, 0, -1, 0, 0], [0, 0, 0, -2e100, 0, 0], [0, 0, 0, -1, 3e100, 0],
           [0, 0, 0, -1e200, 1e200, 0], [0, 0, 0, -1, 0, 1.5e100]]
    rays = np.ascontiguousarray(np.array(odd + [away], np.float64))
    v = np.zeros(len(rays), np.int32)
    lib.lab_bounce_verdicts(len(rays), L._dp(bound), L._dp(rays), v.ctypes.data_as(C.POINTER(C.c_int32)))
    return v[:-1], int(v[-1])


# ---- the scene of the statistics test ---------------------------------------------------------------------------------------------------
def bounce_scene(pkg, centres=None, w=64, h=48):
    """stream_cull_lab's clusters (320 spheres, 5 chunks) under cluster_scene's lights; every sphere reflects 0.6, max_reflections = 2."""
    import stream_scenes as S
    sc = pkg.Scene.new(w, h, S.FOV, 2, (0.05, 0.1, 0.2))
    coefs, cols = SC.cluster_coefs(centres)
    for q, col in zip(coefs, cols):
        sc.add_object(q, col, 0.6)
    sc.add_light("directional", [0.2, -1.0, 0.6], (1.0, 0.95, 0.9), 1.2)
    sc.add_light("spherical", [4.0, 12.0, 2.0], (0.8, 0.9, 1.0), 500.0)
    return sc


def stats_expectation(pkg, sc):
    """From the oracle's per-segment rays of a frame of whole 8 x 8 blocks (paths_ref.paths on the primary rays): D = sum over blocks and
    segments >= 1 with a bouncing lane, times n_chunks; L = the (block, segment, chunk) triples for which no lane's half-line comes within
    1.01 r + 0.1 of the bound's centre (float64 here: the margin dwarfs its rounding).  Returns dict(D, L, n_chunks, queries, rays)."""
    import paths_ref
    import rays_ref
    import stream_scenes as S
    a = sc.arrays()
    w, h = a["width"], a["height"]
    assert w % 8 == 0 and h % 8 == 0
    osc = S.oracle_of(pkg, sc)
    rays = np.ascontiguousarray(rays_ref.primary_rays(osc)).reshape(-1)
    assert len(rays) == w * h
    m = int(osc.max_reflections) + 1
    seg = np.zeros((m, len(rays)), dtype=rays_ref.RAY_DTYPE)
    seg["d"] = np.nan
    paths_ref.paths(osc, rays, seg_rays=seg)
    traced = ~np.isnan(seg["d"][:, :, 0])
    _, bounds, words = SC.image(a)
    b = bounds.view(SC.US_DTYPE)
    centre, reach = -0.5 * b["k"], 1.01 * b["r"] + 0.1
    block = ((np.arange(h)[:, None] // 8) * (w // 8) + (np.arange(w)[None, :] // 8)).reshape(-1)
    D = Lo = queries = n_rays = 0
    for k in range(1, m):
        for blk in range((w // 8) * (h // 8)):
            lanes = np.flatnonzero((block == blk) & traced[k])
            if not len(lanes):
                continue
            queries += 1
            n_rays += len(lanes)
            D += len(b)
            o, d = seg["o"][k, lanes], seg["d"][k, lanes]
            for c in range(len(b)):
                if not np.isfinite(b["r"][c]):
                    continue
                v = centre[c] - o
                t = np.maximum((v * d).sum(axis=1) / (d * d).sum(axis=1), 0.0)
                dist = np.linalg.norm(o + t[:, None] * d - centre[c], axis=1)
                Lo += int((dist > reach[c]).all())
    return dict(D=D, L=Lo, n_chunks=len(b), queries=queries, rays=n_rays)


@functools.lru_cache(maxsize=None)
def expectation():
    """stats_expectation of bounce_scene, once per process (the host test and the GPU test share it)."""
    import __graft_entry__ as graft
    pkg = graft.load_package()
    return stats_expectation(pkg, bounce_scene(pkg))


def format_row(r):
    return (f"ray_reaches {r['family']:10s} cases {r['cases']:7d}  culled {r['culled']:7d}  oracle accepts a member {r['accepted']:7d} (the grazed one "
            f"{r['g_accepted']:7d})  unsound {r['unsound']}  member kept, bound skipped {r['member_kept_bound_skipped']}  beyond the 1e-3 band (sample) {r['beyond']}, "
            f"kept {r['kept']}  repeat differs {r['repeat_differs']}  contracted build: {r['fast_cases']} cases, "
            f"{r['fast_differs']} verdicts differ, unsound {r['fast_unsound']}")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    t0 = time.time()
    rows = []
    for family in FAMILIES:
        rows.append(run_family(family, n))
        print(format_row(rows[-1]), flush=True)
    odd, away = never_culled()
    bad = sum(r["unsound"] + r["member_kept_bound_skipped"] + r["inv_r_short"] + r["not_enclosed"] + r["kept"] + r["repeat_differs"] + r["origin_inside_skipped"] + r["fast_unsound"] for r in rows) + int((odd != 1).sum()) + away
    print(f"bounce_cull_lab: {sum(r['cases'] for r in rows)} verdicts, {sum(r['unsound'] for r in rows)} unsound, {len(odd)} odd rays all tested: {bool((odd == 1).all())}, "
          f"{time.time() - t0:.0f} s")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
