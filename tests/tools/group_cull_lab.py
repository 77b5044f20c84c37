#!/usr/bin/env python3
"""Host lab behind RT_FLAG_STREAM_CULL_GROUPS (tests/tools/group_cull_lab.cpp).  No GPU.
  * `group_image`, `check_groups`: the group bounds of a scene's chunk bounds by the library's own host function, and the claims the
    tests make about them (the count, every finite group bound encloses every member chunk ball and every member sphere ball in
    50-digit arithmetic, inv_r at least every member's, unbounded groups +inf / 0, every byte written, two runs agree);
  * `run_predicates`: sphere_in_cone, both kinds of sphere_relevant and ray_reaches asked about a GROUP bound over two chunks -- chunk A a
    sphere of cull_lab's grazing generator with companions, so that the grazing sphere lies on chunk A's rim, chunk B companions further
    out the same way, so that chunk A lies on the group's rim --, about both chunk bounds and about every member;
  * `two_clusters`, `primary_expectation`: the scenes of the GPU tests and the exact primary group words of a frame.
usage: python tests/tools/group_cull_lab.py [n]      n cases per predicate and family (default 100000)"""
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
import bounce_cull_lab as BL  # noqa: E402
import cull_lab as L  # noqa: E402
import pixel_cull_lab as PL  # noqa: E402
import stream_cull_lab as SC  # noqa: E402

FANOUT = 64
GL_OUT = 8
FAMILIES = ("rim", "any")
KINDS = ("cone", "sh_dir", "sh_sph", "ray")
PREDICATE_OF = dict(SC.PREDICATE_OF, ray="ray_reaches")
N_COMP = SC.N_COMP

_LIB = None


def build():
    global _LIB
    if _LIB is None:
        L.build()   # (the oracle's library)
        out = os.path.join(TOOLS, "bin", "libgroup_cull_lab.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-subobject-linkage", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tools", "flopcount_shim"),
                        "-I" + os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-I" + TOOLS,
                        os.path.join(TOOLS, "group_cull_lab.cpp"), "-o", out, "-L" + os.path.join(ROOT, "oracle"), "-lrt_oracle",
                        "-Wl,-rpath," + os.path.join(ROOT, "oracle")], check=True)
        lib = C.CDLL(out)
        dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
        lib.lab_group_image.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
        lib.lab_group_image.restype = None
        for f in (lib.lab_group_primary, lib.lab_group_shadow, lib.lab_group_ray):
            f.argtypes = [C.c_uint64, dp, C.c_int, dp, dp, ip]
            f.restype = None
        _LIB = lib
    return _LIB


# ---- the group bounds ------------------------------------------------------------------------------------------------------------------
def n_groups_of(n_chunks):
    return (n_chunks + FANOUT - 1) // FANOUT


def group_image(bounds, fill=0):
    """The group bounds (bytes, 64 per group) of a chunk-bound table (bytes, 64 per chunk), every byte preset to fill ^ 0xFF here and to
    `fill` by the library before its pack function writes it."""
    bounds = np.ascontiguousarray(bounds, np.uint8)
    n_chunks = bounds.size // SC.US_BYTES
    out = np.full(n_groups_of(n_chunks) * SC.US_BYTES, fill ^ 0xFF, np.uint8)
    build().lab_group_image(bounds.ctypes.data, n_chunks, fill, out.ctypes.data)
    return out


def _mp_centre(mp, e):
    return [-mp.mpf(float(x)) / 2 for x in e["k"]]


def check_groups(a, flags=0):
    """Every claim about the group bounds of one scene (its descriptor arrays); returns dict(n_us, n_chunks, n_groups, n_inf, worst_slack)."""
    import mpmath as mp
    mp.mp.dps = 50
    blob, bounds, w = SC.image(a, flags)
    t, b = SC.table_of(blob, w), bounds.view(SC.US_DTYPE)
    raw = group_image(bounds)
    g = raw.view(SC.US_DTYPE)
    assert len(g) == n_groups_of(w["n_chunks"]) == (w["n_us"] + 4095) // 4096
    n_inf, worst = 0, np.inf
    for G in range(len(g)):
        e, chunks = g[G], b[FANOUT * G:FANOUT * (G + 1)]
        spheres = t[4096 * G:4096 * (G + 1)]
        assert e["orig"] == G and e["pad"] == 0 and np.isposinf(e["own_lo"]) and e["own_hi"] == 0.0
        if not np.isfinite(chunks["r"]).all():
            n_inf += 1
            assert not np.isfinite(spheres["r"]).all()      # (a chunk is unbounded only through a member)
            assert np.isposinf(e["r"]) and e["inv_r"] == 0.0 and not e["k"].any() and e["c"] == 0.0, G
            continue
        assert np.isfinite(e["r"]) and e["inv_r"] >= chunks["inv_r"].max() and e["inv_r"] >= spheres["inv_r"].max(), G
        C3, R = _mp_centre(mp, e), mp.mpf(float(e["r"]))
        need = mp.mpf(0)
        for m in list(chunks) + list(spheres):      # every member chunk ball, and every member sphere ball
            d = mp.sqrt(sum((x - y) ** 2 for x, y in zip(_mp_centre(mp, m), C3)))
            need = max(need, d + mp.mpf(float(m["r"])))
        slack = (R - need) / R
        assert slack > 0, (G, float(slack))
        worst = min(worst, float(slack))
    for fill in (0x5A, 0xC3):       # poisoned fill: every byte is written, whatever the fill
        assert np.array_equal(group_image(bounds, fill), raw), fill
    assert np.array_equal(group_image(SC.image(a, flags)[1]), raw)      # two runs agree
    return dict(n_us=w["n_us"], n_chunks=w["n_chunks"], n_groups=len(g), n_inf=n_inf, worst_slack=worst)


# ---- the predicate lab -----------------------------------------------------------------------------------------------------------------
def _two_chunks(kind, family, rec, par, centre, seed):
    """Chunk A's companions (stream_cull_lab's: the far one sets chunk A's width, in `rim` away from the rays, so the grazing sphere lies on
    chunk A's rim) and chunk B's.  pack_chunk_bound centres a bound on the middle of the box of its members' centres, so a group bound
    touches chunk A's bound where the rays pass only if both chunk bounds share that middle:
      rim   chunk B's spheres lie symmetric about the middle of chunk A's box, up to 0.3 of chunk A's half width from it: the group bound is
            chunk A's bound widened by its pad -- chunk A lies on the group's rim all around, the grazing sphere on both rims;
      any   another draw of stream_cull_lab's `any` pushed 1 .. 10 times further from the grazing sphere: groups of any shape."""
    fam = "rim" if family == "rim" else "any"
    if kind == "ray":
        a, b = BL.companions(fam, par, centre, seed), BL.companions(fam, par, centre, seed + 5000)
    else:
        a, b = SC.companions(kind, fam, rec, par, centre, seed), SC.companions(kind, fam, rec, par, centre, seed + 5000)
    rng = np.random.default_rng(910000 + seed)
    n = len(a)
    b = b.copy()
    if family == "rim":
        pts = np.concatenate([centre[:, None, :], a[:, :, :3]], axis=1)
        mid = 0.5 * pts.min(axis=1) + 0.5 * pts.max(axis=1)
        half = 0.5 * np.linalg.norm(a[:, 0, :3] - centre, axis=1)
        v = SC._unit(rng.normal(size=(n, 3))) * (half * rng.uniform(0.0, 0.3, n))[:, None]
        b[:, 0, :3], b[:, 1, :3] = mid + v, mid - v
        for k in range(2, b.shape[1]):
            b[:, k, :3] = mid + rng.uniform(-1, 1, (n, 1)) * v
    else:
        push = 10.0 ** rng.uniform(0, 1, (n, 1, 1))
        b[:, :, :3] = centre[:, None, :] + push * (b[:, :, :3] - centre[:, None, :])
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def group_cases(kind, family, n, seed):
    """One batch: [n, GL_OUT] int32 -- group verdict (-1: a case the generator drops), chunk A's, chunk B's, some member's own verdict is
    "test it", the oracle accepts a member, not enclosed, inv_r short, chunk verdicts "test it" under a skipped group."""
    lib = build()
    if kind == "cone":
        r, par, centre = L.graze_primary(n, seed, 0)
        rec, _ = r.get("cone")
        fn = lib.lab_group_primary
    elif kind == "ray":
        par = np.ascontiguousarray(BL.ray_params(n, seed, family))
        centre, rec, fn = BL.graze_centre(par), None, lib.lab_group_ray
    else:
        r, par, centre = L.graze_shadow(n, seed, kind == "sh_sph")
        rec, _ = r.get("sh")
        fn = lib.lab_group_shadow
    assert rec is None or len(rec) == n, (kind, n)
    a, b = _two_chunks(kind, family, rec, par, centre, seed)
    out = np.zeros((n, GL_OUT), np.int32)
    fn(n, L._dp(np.ascontiguousarray(par)), N_COMP, L._dp(a), L._dp(b), out.ctypes.data_as(C.POINTER(C.c_int32)))
    return out


def run_predicates(n, chunk=10000, verbose=False):
    """n cases per predicate and family.  Rows of dict(predicate, family, cases, skipped, chunk_skipped, accepted, unsound_chunk, unsound_member,
    unsound_oracle, not_enclosed, inv_r_short, repeat_differs)."""
    rows = []
    for kind in KINDS:
        for family in FAMILIES:
            row = dict(predicate=PREDICATE_OF[kind], family=family, cases=0, skipped=0, chunk_skipped=0, accepted=0, unsound_chunk=0, unsound_member=0, unsound_oracle=0,
                       not_enclosed=0, inv_r_short=0, repeat_differs=0)
            done = seed = 0
            while done < n:
                k = min(chunk, n - done)
                o = group_cases(kind, family, k, seed)
                if seed == 0:
                    row["repeat_differs"] += int((group_cases(kind, family, k, seed) != o).sum())
                o = o[o[:, 0] >= 0]
                skip = o[:, 0] == 0
                row["cases"] += len(o)
                row["skipped"] += int(skip.sum())
                row["chunk_skipped"] += int((o[:, 1] == 0).sum() + (o[:, 2] == 0).sum())
                row["accepted"] += int((o[:, 4] != 0).sum())
                row["unsound_chunk"] += int((skip & ((o[:, 1] != 0) | (o[:, 2] != 0))).sum())
                row["unsound_member"] += int((skip & (o[:, 3] != 0)).sum())
                row["unsound_oracle"] += int((skip & (o[:, 4] != 0)).sum())
                row["not_enclosed"] += int(o[:, 5].sum())
                row["inv_r_short"] += int(o[:, 6].sum())
                done += k
                seed += 1
            rows.append(row)
            if verbose:
                print(format_row(row), flush=True)
    return rows


def format_row(r):
    return (f"{r['predicate']:24s} {r['family']:4s} cases {r['cases']:7d}  groups skipped {r['skipped']:7d}  chunk bounds skipped {r['chunk_skipped']:7d}  oracle accepts a "
            f"member {r['accepted']:7d}  group skipped beside: a kept chunk bound {r['unsound_chunk']}, a kept member {r['unsound_member']}, an accepted member "
            f"{r['unsound_oracle']}")


# ---- the scenes of the GPU tests --------------------------------------------------------------------------------------------------------
CENTRES = ((-9.0, -5.0, 22.0), (40.0, 4.0, 25.0))      # the first inside the view, the second far to its right: the Morton key's top bit is x's
CLUSTER_SEED = 53


def cluster_coefs(counts, centres=CENTRES, seed=CLUSTER_SEED, radius=0.22, spread=2.2):
    """stream_cull_lab.cluster_coefs at other sizes: (coefs [n, 20], colours [n, 3]) of small spheres in clusters of counts[k] around
    centres[k], each within `spread` of its centre.  Other centres for the same spheres: the same seed (rt_set_scene: the clusters
    exchange places)."""
    rng = np.random.default_rng(seed)
    coefs, cols = [], []
    for c0, n in zip(centres, counts):
        off = rng.normal(size=(n, 3))
        off *= (spread * rng.uniform(0, 1, n) ** (1 / 3) / np.linalg.norm(off, axis=1))[:, None]
        c = np.array(c0) + off
        q = np.zeros((n, 20))
        q[:, 10:13] = 1.0
        q[:, 16:19] = -2.0 * c
        q[:, 19] = (c * c).sum(axis=1) - radius ** 2
        coefs.append(q)
        cols.append(rng.uniform(0.2, 1.0, (n, 3)))
    return np.concatenate(coefs), np.concatenate(cols)


def two_clusters(pkg, counts=(4096, 4096), centres=CENTRES, w=64, h=48, mirrors=False, depth=0):
    """Two clusters under both of stream_scenes.field's lights (stream_cull_lab.cluster_scene at other sizes): the camera sees the first,
    and neither light's shadow rays from it come near the second.  mirrors: every third sphere reflects 0.5."""
    import stream_scenes as S
    sc = pkg.Scene.new(w, h, S.FOV, depth, (0.05, 0.1, 0.2))
    coefs, cols = cluster_coefs(counts, centres)
    for i, (q, col) in enumerate(zip(coefs, cols)):
        sc.add_object(q, col, 0.5 if (mirrors and i % 3 == 0) else 0.0)
    sc.add_light("directional", [0.2, -1.0, 0.6], (1.0, 0.95, 0.9), 1.2)
    sc.add_light("spherical", [4.0, 12.0, 2.0], (0.8, 0.9, 1.0), 500.0)
    return sc


def big_field(pkg, n, seed, w=16, h=16):
    """(descriptor, arrays) of n small spheres spread over the view of a w x h frame at depths 20 .. 30 (stream_scenes.field's recipe in
    numpy: a scene of a quarter of a million objects is not added one call at a time), under that scene's two lights."""
    import stream_scenes as S
    rng = np.random.default_rng(seed)
    tan = np.tan(np.radians(S.FOV / 2))
    z = rng.uniform(20.0, 30.0, n)
    c = np.stack([rng.uniform(-1, 1, n) * z * tan * w / h * 0.96, rng.uniform(-1, 1, n) * z * tan * 0.96, z], axis=1)
    r = 0.5 * 0.35 * 2.0 * z * tan / h
    q = np.zeros((n, 20))
    q[:, 10:13] = 1.0
    q[:, 16:19] = -2.0 * c
    q[:, 19] = (c * c).sum(axis=1) - r * r
    lights = S.field(pkg, 1, seed, w=w, h=h).arrays()
    a = dict(coefs=q, reflection=np.zeros(n, np.float32), albedo=rng.uniform(0.2, 1.0, (n, 3)).astype(np.float32),
             light_is_spherical=lights["light_is_spherical"], light_p=lights["light_p"], light_color=lights["light_color"])
    d = pkg.desc_from_arrays(w, h, lights["vertical_fov"], lights["bg_color"], 0, a["coefs"], a["reflection"], a["albedo"], a["light_is_spherical"], a["light_p"],
                             a["light_color"])
    return d, a


def primary_expectation(osc, a):
    """The exact primary group words of one frame of whole 8 x 8 blocks under the identity camera: dict(blocks, n_groups, n_chunks, asked =
    blocks x groups, entered, chunks_asked = the chunk counts of the entered groups, staged) from the numpy cone predicate of
    tools/pixel_cull_lab.py asked about the group bounds (and, for `staged`, about the chunk bounds)."""
    org, axis, cos_t = PL.block_cones(osc)
    _, bounds, w = SC.image(a)
    b = bounds.view(SC.US_DTYPE)
    g = group_image(bounds).view(SC.US_DTYPE)
    nb = len(org)

    def ask(e):
        n = len(e)
        rep = lambda x: np.repeat(x, n, axis=0)
        tile = lambda x: np.tile(x, (nb,) + (1,) * (x.ndim - 1))
        return PL.sphere_in_cone(tile(e["k"]), tile(e["r"]), tile(e["inv_r"]), rep(org), rep(axis), rep(cos_t)).reshape(nb, n)

    vg, vc = ask(g), ask(b)
    size = np.array([min(FANOUT, len(b) - FANOUT * G) for G in range(len(g))])
    assert not (vc & ~np.repeat(vg, FANOUT, axis=1)[:, :len(b)]).any()      # (a kept chunk bound under a skipped group would be a finding)
    return dict(blocks=nb, n_groups=len(g), n_chunks=len(b), asked=nb * len(g), entered=int(vg.sum()), chunks_asked=int((vg * size[None, :]).sum()), staged=int(vc.sum()))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    t0 = time.time()
    rows = run_predicates(n, verbose=True)
    bad = sum(r["unsound_chunk"] + r["unsound_member"] + r["unsound_oracle"] + r["not_enclosed"] + r["inv_r_short"] for r in rows)
    print(f"group_cull_lab: {sum(r['cases'] for r in rows)} group verdicts, {sum(r['skipped'] for r in rows)} skips, {bad} findings, {time.time() - t0:.0f} s")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
