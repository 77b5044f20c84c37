#!/usr/bin/env python3
"""Host lab behind RT_FLAG_STREAM_CULL (tests/tools/stream_cull_lab.cpp).  No GPU.
  * `image`: the scene image of a context whose decision is true -- the blob with its ordered unit-sphere table and the chunk bounds --
    by the library's own host functions, and the checks the tests make on it (`check_image`: a permutation of the unflagged table, every
    bound encloses its members in 50-digit arithmetic, unbounded chunks are +inf, every byte written, two runs agree);
  * `run_predicates`: the culling predicates asked about the bound of a chunk that holds a sphere of cull_lab's grazing generator and
    companions up to 1e5 radii away; the truth is the oracle's verdict for every member;
  * `cluster_scene`, `stats_expectation`: the scene of the GPU statistics test and what the oracle says its work words must be.
usage: python tests/tools/stream_cull_lab.py [n]      n grazing cases per predicate and family (default 100000)"""
import ctypes as C
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
from scene_pack_lab import LabDesc  # noqa: E402

O = L.O
CHUNK, US_BYTES = 64, 64
US_DTYPE = np.dtype([("k", "<f8", 3), ("c", "<f8"), ("r", "<f8"), ("inv_r", "<f8"), ("orig", "<u4"), ("own_lo", "<f4"), ("own_hi", "<f4"), ("pad", "<u4")])
assert US_DTYPE.itemsize == US_BYTES
FAMILIES = ("rim", "any", "light")   # companions away from the rays / anywhere / (point lights) so that the light lies inside or next to the bound
BAND = 1e-3

_LIB = None


def build():
    global _LIB
    if _LIB is None:
        L.build()   # (the oracle's library)
        out = os.path.join(TOOLS, "bin", "libstream_cull_lab.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-subobject-linkage", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tools", "flopcount_shim"),
                        "-I" + os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-I" + TOOLS,
                        os.path.join(TOOLS, "stream_cull_lab.cpp"), "-o", out, "-L" + os.path.join(ROOT, "oracle"), "-lrt_oracle",
                        "-Wl,-rpath," + os.path.join(ROOT, "oracle")], check=True)
        lib = C.CDLL(out)
        dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
        lib.lab_stream_cull_image.restype = C.c_uint64
        lib.lab_stream_cull_image.argtypes = [C.POINTER(LabDesc), C.c_uint32, C.c_uint32, C.c_int, vp, vp, C.c_uint64, vp, C.c_uint64, vp]
        lib.lab_bound_primary.argtypes = lib.lab_bound_shadow.argtypes = [C.c_uint64, dp, C.c_int, dp, dp, ip, ip, ip, dp]
        _LIB = lib
    return _LIB


# ---- the scene image ---------------------------------------------------------------------------------------------------------------
def image(a, flags=0, fill=0, ordered=True, slot_orig=None):
    """a: a scene's descriptor arrays (Scene.arrays() of the package, or any mapping with coefs, reflection, albedo, light_is_spherical,
    light_p, light_color).  Returns (blob bytes, bounds bytes, words) with words = dict(n_us, off_us, n_chunks, cull, scene_bytes)."""
    lib = build()
    keep = [np.ascontiguousarray(a["coefs"], np.float64), np.ascontiguousarray(a["reflection"], np.float32), np.ascontiguousarray(a["albedo"], np.float32),
            np.ascontiguousarray(a["light_is_spherical"], np.uint8), np.ascontiguousarray(a["light_p"], np.float64), np.ascontiguousarray(a["light_color"], np.float32)]
    d = LabDesc(keep[1].size, keep[3].size, *[x.ctypes.data for x in keep])
    words = np.zeros(5, np.uint32)
    so = None if slot_orig is None else np.ascontiguousarray(slot_orig, np.uint32)
    n = lib.lab_stream_cull_image(C.byref(d), flags, fill, 0, None, None, 0, None, 0, words.ctypes.data)
    blob = np.full(n, fill ^ 0xFF, np.uint8)
    bounds = np.full(((int(words[0]) + CHUNK - 1) // CHUNK) * US_BYTES, fill ^ 0xFF, np.uint8)
    lib.lab_stream_cull_image(C.byref(d), flags, fill, 1 if ordered else 0, None if so is None else so.ctypes.data, blob.ctypes.data, blob.size,
                              bounds.ctypes.data, bounds.size, words.ctypes.data)
    w = dict(zip(("n_us", "off_us", "n_chunks", "cull", "scene_bytes"), (int(x) for x in words)))
    return blob, (bounds if ordered else bounds[:0]), w


def table_of(blob, w):
    return blob[w["off_us"]:w["off_us"] + US_BYTES * w["n_us"]].view(US_DTYPE)


def arrays_of_oracle(osc):
    return dict(coefs=osc.coefs, reflection=osc.reflection, albedo=osc.albedo, light_is_spherical=osc.light_is_spherical, light_p=osc.light_p,
                light_color=osc.light_color)


def check_image(a, flags=0):
    """Every claim about the flagged image of one scene; returns dict(n_us, n_chunks, n_inf, worst_slack) -- worst_slack: the smallest
    r - max_i(|c_i - C| + r_i) over the finite bounds, relative to r (it must be positive)."""
    import mpmath as mp
    mp.mp.dps = 50
    plain, none, w0 = image(a, flags, ordered=False)
    blob, bounds, w = image(a, flags)
    assert none.size == 0 and w == dict(w0, n_chunks=(w["n_us"] + CHUNK - 1) // CHUNK) and blob.size == plain.size == w["scene_bytes"]
    lo, hi = w["off_us"], w["off_us"] + US_BYTES * w["n_us"]
    # the flagged blob differs from the unflagged one only inside the table, and is a permutation of it
    assert np.array_equal(blob[:lo], plain[:lo]) and np.array_equal(blob[hi:], plain[hi:])
    t, t0 = table_of(blob, w), table_of(plain, w)
    by_orig = np.argsort(t["orig"], kind="stable")
    assert np.array_equal(t[by_orig].view(np.uint8), t0.view(np.uint8))       # (the unflagged table is in object order)
    # the order: bounded spheres first, unbounded behind them in index order
    bounded = np.isfinite(t["r"])
    nb = int(bounded.sum())
    assert bounded[:nb].all() and not bounded[nb:].any() and (np.diff(t["orig"][nb:].astype(np.int64)) > 0).all()
    # the bounds
    b = bounds.view(US_DTYPE)
    assert len(b) == w["n_chunks"]
    n_inf, worst = 0, np.inf
    for c in range(len(b)):
        mem = t[CHUNK * c:CHUNK * (c + 1)]
        e = b[c]
        assert e["orig"] == c and e["pad"] == 0 and np.isposinf(e["own_lo"]) and e["own_hi"] == 0.0
        if not np.isfinite(mem["r"]).all():
            n_inf += 1
            assert np.isposinf(e["r"]) and e["inv_r"] == 0.0 and not e["k"].any() and e["c"] == 0.0, c
            continue
        assert np.isfinite(e["r"]) and e["inv_r"] >= mem["inv_r"].max(), c
        C3 = [-mp.mpf(float(x)) / 2 for x in e["k"]]
        need = mp.mpf(0)
        for m in mem:
            d = mp.sqrt(sum((-mp.mpf(float(x)) / 2 - y) ** 2 for x, y in zip(m["k"], C3)))
            need = max(need, d + mp.mpf(float(m["r"])))
        slack = (mp.mpf(float(e["r"])) - need) / mp.mpf(float(e["r"]))
        assert slack > 0, (c, float(slack))
        worst = min(worst, float(slack))
        # a genuine sphere: c = |C|^2 - r^2 to rounding
        want = sum(x * x for x in C3) - mp.mpf(float(e["r"])) ** 2
        assert abs(mp.mpf(float(e["c"])) - want) <= mp.mpf(2) ** -48 * (sum(x * x for x in C3) + mp.mpf(float(e["r"])) ** 2), c
    # poisoned fill: every byte of the table and the bounds is written, whatever the fill; two runs give identical bytes
    for fill in (0x5A, 0xC3):
        blob2, bounds2, _ = image(a, flags, fill=fill)
        assert np.array_equal(blob2[lo:hi], blob[lo:hi]) and np.array_equal(bounds2, bounds), fill
    blob3, bounds3, _ = image(a, flags)
    assert np.array_equal(blob3, blob) and np.array_equal(bounds3, bounds)
    # the context's order is reproducible from its `orig` words (what a context that has seen rt_set_scene is held to)
    blob4, bounds4, _ = image(a, flags, slot_orig=t["orig"])
    assert np.array_equal(blob4, blob) and np.array_equal(bounds4, bounds)
    return dict(n_us=w["n_us"], n_chunks=w["n_chunks"], n_inf=n_inf, worst_slack=worst)


# ---- the predicate lab ---------------------------------------------------------------------------------------------------------------
N_COMP = 3


def _unit(v):
    n = np.linalg.norm(v, axis=1, keepdims=True)
    return np.where(n > 0, v / np.where(n > 0, n, 1.0), 0.0)


def _outward(kind, rec, centre):
    """Unit vectors from the rays' cone axis / line / segment to the grazing sphere's centre (random where that is degenerate)."""
    if kind == "cone":
        v = centre - rec[:, 5:8]
        a = _unit(rec[:, 8:11])
        out = v - (v * a).sum(axis=1, keepdims=True) * a
    else:
        w = centre - rec[:, 6:9]
        sph = rec[:, 24] != 0
        e = np.where(sph[:, None], rec[:, 13:16] - rec[:, 6:9], rec[:, 16:19])
        ee = (e * e).sum(axis=1)
        t = (w * e).sum(axis=1) / np.where(ee > 0, ee, 1.0)
        t = np.where(sph, np.clip(t, 0.0, 1.0), t)
        out = w - t[:, None] * e
    return out


def companions(kind, family, rec, par, centre, seed):
    """[n, N_COMP, 4] companions (centre, radius) of the grazing sphere: the first one 1 .. 1e5 radii away -- it sets the bound's width --,
    the others between the two or near either; radii 1e-1 .. 1 of the grazing sphere's (cull_lab draws that one from 1e-4 .. 10 scales)."""
    rng = np.random.default_rng(730000 + seed)
    n = len(rec)
    r = par[:, 23] if kind == "cone" else par[:, 4]
    width = r * 10.0 ** rng.uniform(0, 5, n)
    rnd = _unit(rng.normal(size=(n, 3)))
    if family == "rim":
        d = _unit(_outward(kind, rec, centre))
        d = np.where((d * d).sum(axis=1, keepdims=True) > 0.5, d, rnd)
        d = _unit(d + np.where(rng.random((n, 1)) < 0.5, 0.0, 0.3 * rng.uniform(0, 1, (n, 1))) * rnd)   # (half of them exactly away from the rays: the bound touches the grazing sphere where the rays pass)
        far = centre + width[:, None] * d
    elif family == "any":
        far = centre + width[:, None] * rnd
    else:   # the light at the bound's centre (the far companion as far behind the light as the grazing sphere is in front of it), or next to
        # the bound's rim from inside / outside: the far companion sideways by w with |M - light| = w / 2 + r (1 + delta), M the middle
        lp = par[:, 1:4]
        to = lp - centre
        dist = np.linalg.norm(to, axis=1)
        side = _unit(np.cross(to, rnd))
        rr = r * (1.0 + rng.choice([-1.0, 1.0], n) * 10.0 ** (-rng.integers(1, 9, n).astype(float)))
        w = (dist * dist - rr * rr) / rr
        at_centre = (rng.random(n) < 0.3) | ~(w > 0)
        far = np.where(at_centre[:, None], centre + 2.0 * to, centre + w[:, None] * side)
    comp = np.zeros((n, N_COMP, 4))
    comp[:, 0, :3] = far
    comp[:, 0, 3] = r * 10.0 ** rng.uniform(-1, 0, n)
    for k in range(1, N_COMP):
        s = rng.uniform(0, 1, (n, 1)) if family != "light" else np.zeros((n, 1))   # (light: next to the grazing sphere, not on the way to the light)
        comp[:, k, :3] = centre + s * (far - centre) + (r * rng.uniform(0, 1, n))[:, None] * _unit(rng.normal(size=(n, 3)))
        comp[:, k, 3] = r * 10.0 ** rng.uniform(-1, 0, n)
    return comp


def bound_cases(kind, family, n, seed):
    """One batch: (bound records, verdicts, oracle accepts some member, oracle accepts the grazing sphere, members [n, N_COMP + 1, 5], clearances)."""
    lib = build()
    if kind == "cone":
        r, par, centre = L.graze_primary(n, seed, 0)
        rec, _ = r.get("cone")
        width, fn, delta = L.REC["cone"], lib.lab_bound_primary, par[:, 24]
    else:
        r, par, centre = L.graze_shadow(n, seed, kind == "sh_sph")
        rec, _ = r.get("sh")
        width, fn, delta = L.REC["sh"], lib.lab_bound_shadow, par[:, 5]
    assert len(rec) == n, (kind, len(rec), n)
    comp = np.ascontiguousarray(companions(kind, family, rec, par, centre, seed))
    out = np.zeros((n, width))
    v, t, g = (np.zeros(n, np.int32) for _ in range(3))
    members = np.zeros((n, N_COMP + 1, 5))
    ip = C.POINTER(C.c_int32)
    fn(n, L._dp(np.ascontiguousarray(par)), N_COMP, L._dp(comp), L._dp(out), v.ctypes.data_as(ip), t.ctypes.data_as(ip), g.ctypes.data_as(ip), L._dp(members))
    assert (v >= 0).all()
    return out, v, t, g, members, delta


def bound_excess(kind, rec):
    """cull_lab.exact_excess for a bound's record, with the distance scale the predicate really uses: a bound carries the largest inv_r of
    its members, not 1 / r.  (excess, section 14's scale, the bound's scale), or None where the predicate never culls."""
    x = L.exact_excess(kind, rec)
    if x is None:
        return None
    excess, scale = x
    if kind == "cone":
        c, r, q, s2 = -0.5 * rec[0:3], rec[3], rec[4], 0.0
        s2 = float(c @ c + rec[5:8] @ rec[5:8])
    else:
        c, r, q = -0.5 * rec[0:3], rec[4], rec[5]
        s2 = float(c @ c + rec[6:9] @ rec[6:9]) + (float(rec[13:16] @ rec[13:16]) if kind == "sh_sph" else 0.0)
    return excess, scale, scale + (s2 + 1.0) * 1e-6 * max(q - 1.0 / r, 0.0)


def kept_beyond_band(kind, rec, verdict, sample=400, seed=0):
    """Of a sample: (beyond section 14's band, kept among them, beyond the band at the bound's own scale, kept among those)."""
    rng = np.random.default_rng(seed)
    n14 = k14 = nb = kb = 0
    for i in rng.choice(len(rec), min(sample, len(rec)), replace=False):
        x = bound_excess(kind, rec[i])
        if x is None:
            continue
        excess, s14, sb = x
        if excess > BAND * s14:
            n14 += 1
            k14 += int(verdict[i] != 0)
        if excess > BAND * sb:
            nb += 1
            kb += int(verdict[i] != 0)
    return n14, k14, nb, kb


PREDICATE_OF = {"cone": "sphere_in_cone", "sh_dir": "sphere_relevant<false>", "sh_sph": "sphere_relevant<true>"}


def run_predicates(n, chunk=20000, sample=400, verbose=False):
    """n cases per predicate and family.  Returns rows of dict(predicate, family, cases, culled, accepted, g_accepted, unsound, inv_r_short,
    not_enclosed, beyond14, kept14, beyond, kept)."""
    rows = []
    for kind in ("cone", "sh_dir", "sh_sph"):
        for family in FAMILIES:
            if family == "light" and kind != "sh_sph":
                continue
            row = dict(predicate=PREDICATE_OF[kind], family=family, cases=0, culled=0, accepted=0, g_accepted=0, unsound=0, inv_r_short=0, not_enclosed=0,
                       beyond14=0, kept14=0, beyond=0, kept=0, examples=[])
            done, seed = 0, 0
            while done < n:
                k = min(chunk, n - done)
                rec, v, t, g, members, _ = bound_cases(kind, family, k, seed)
                row["cases"] += k
                row["culled"] += int((v == 0).sum())
                row["accepted"] += int((t != 0).sum())
                row["g_accepted"] += int((g != 0).sum())
                bad = (v == 0) & (t != 0)
                row["unsound"] += int(bad.sum())
                row["examples"] += [rec[i].copy() for i in np.flatnonzero(bad)[:2]]
                # the bound itself (float64 here; tests/test_stream_cull_host.py holds the enclosure in 50 digits on the scenes' chunks)
                bc, br, bq = -0.5 * rec[:, 0:3], (rec[:, 3] if kind == "cone" else rec[:, 4]), (rec[:, 4] if kind == "cone" else rec[:, 5])
                fin = np.isfinite(br)
                reach = (np.linalg.norm(members[:, :, :3] - bc[:, None, :], axis=2) + members[:, :, 3]).max(axis=1)
                row["not_enclosed"] += int((fin & (br < reach)).sum())
                row["inv_r_short"] += int((fin & (bq < members[:, :, 4].max(axis=1))).sum())
                b14, k14, b, kb = kept_beyond_band(kind, rec, v, sample=max(1, sample * k // n), seed=seed)
                row["beyond14"] += b14; row["kept14"] += k14; row["beyond"] += b; row["kept"] += kb
                done += k
                seed += 1
            rows.append(row)
            if verbose:
                print(format_row(row), flush=True)
    return rows


def format_row(r):
    return (f"{r['predicate']:24s} {r['family']:6s} cases {r['cases']:7d}  culled {r['culled']:7d}  oracle accepts a member {r['accepted']:7d} "
            f"(the grazing one {r['g_accepted']:7d})  unsound {r['unsound']}  beyond the 1e-3 band (sample): {r['beyond14']} at section 14's scale, "
            f"{r['kept14']} kept; {r['beyond']} at the bound's scale, {r['kept']} kept")


# ---- the scene of the statistics test -------------------------------------------------------------------------------------------------
CLUSTERS = (((-9.0, -5.0, 22.0), 128), ((8.5, 5.0, 28.0), 128), ((-1.0, 6.5, 25.0), 64))
CLUSTER_SEED = 31


def cluster_coefs(centres=None, seed=CLUSTER_SEED):
    """(coefs [n, 20], colours [n, 3]) of small spheres in well-separated clusters (CLUSTERS: centre, count), radius 0.22, each cluster within
    2.2 of its centre.  centres: other cluster centres for the same spheres (rt_set_scene: the clusters exchange places)."""
    rng = np.random.default_rng(seed)
    coefs, cols = [], []
    for k, (c0, n) in enumerate(CLUSTERS):
        c0 = np.array(c0 if centres is None else centres[k])
        for _ in range(n):
            off = rng.normal(size=3)
            off *= 2.2 * rng.uniform(0, 1) ** (1 / 3) / np.linalg.norm(off)
            c = c0 + off
            q = np.zeros(20)
            q[10:13] = 1.0
            q[16:19] = -2.0 * c
            q[19] = float(c @ c) - 0.22 ** 2
            coefs.append(q)
            cols.append(rng.uniform(0.2, 1.0, 3))
    return np.array(coefs), np.array(cols)


def cluster_scene(pkg, centres=None, w=64, h=48):
    """The clusters under both of stream_scenes.field's lights, no mirrors."""
    import stream_scenes as S
    sc = pkg.Scene.new(w, h, S.FOV, 0, (0.05, 0.1, 0.2))
    coefs, cols = cluster_coefs(centres)
    for q, col in zip(coefs, cols):
        sc.add_object(q, col, 0.0)
    sc.add_light("directional", [0.2, -1.0, 0.6], (1.0, 0.95, 0.9), 1.2)
    sc.add_light("spherical", [4.0, 12.0, 2.0], (0.8, 0.9, 1.0), 500.0)
    return sc


def stats_expectation(pkg, sc):
    """From the oracle's hit points of a 64 x 48 frame (whole 8 x 8 blocks, no mirrors, every light culled for): D = blocks with a hit x lights x
    chunks, and L = a lower bound of the (block, light, chunk) triples whose bound lies beyond the 1e-3 band of the Euclidean criterion
    (the ball of the block's hit points swept along the light's direction / to the light's position; cull_lab's FP32-rounded ball, which
    holds the kernel's).  Returns dict(D, L, blocks, n_chunks)."""
    import stream_scenes as S
    a = sc.arrays()
    assert a["width"] % 8 == 0 and a["height"] % 8 == 0 and not (a["reflection"] > 0).any()
    osc = S.oracle_of(pkg, sc)
    fr = L.frame(osc, stride=1 << 30)
    cone, ctruth = fr.get("cone")
    n_us = len(a["reflection"])
    n_blocks = (a["width"] // 8) * (a["height"] // 8)
    assert len(cone) == n_blocks * n_us
    hit_blocks = int(ctruth.reshape(n_blocks, n_us).any(axis=1).sum())
    n_lights = len(a["light_is_spherical"])
    sh, _ = fr.get("sh")
    sh = sh[:hit_blocks * n_lights * n_us].reshape(hit_blocks, n_lights, n_us, -1)[:, :, 0, :]     # one record per (block, light): ball and light
    _, bounds, w = image(a)
    b = bounds.view(US_DTYPE)
    beyond = 0
    for rec in sh.reshape(-1, sh.shape[-1]):
        for e in b:
            if not np.isfinite(e["r"]):
                continue
            r = rec.copy()
            r[0:3], r[3], r[4], r[5] = e["k"], e["c"], e["r"], e["inv_r"]
            x = bound_excess("sh_sph" if rec[24] != 0 else "sh_dir", r)
            beyond += int(x is not None and x[0] > BAND * x[2])
    return dict(D=hit_blocks * n_lights * w["n_chunks"], L=beyond, blocks=hit_blocks, n_chunks=w["n_chunks"])


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    t0 = time.time()
    rows = run_predicates(n, verbose=True)
    bad = sum(r["unsound"] + r["inv_r_short"] + r["not_enclosed"] + r["kept"] for r in rows)
    print(f"stream_cull_lab: {sum(r['cases'] for r in rows)} verdicts, {sum(r['unsound'] for r in rows)} unsound, {time.time() - t0:.0f} s")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
