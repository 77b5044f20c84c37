#!/usr/bin/env python3
"""Host lab behind rt_reorder_scene (RT_FLAG_STREAM_CULL_REORDER; csrc/rt_reorder_scene.hip).  No GPU.
  * `keys` / `keys_numpy`: the library's key function (rtp::stream_cull_key, compiled for the host by tests/tools/reorder_lab.cpp) and its
    restatement in numpy, operation for operation in float64;
  * `mix`: the motion of the tests -- S1 gives object i the centre of object pi(i) of S0 for a seeded permutation, plus a small jitter,
    and keeps its radius, class, cullability and material, so rt_set_scene accepts it;
  * `stale` / `fresh`: the images a context created on S0 holds after rt_set_scene(S1) (S0's order of slots) and after rt_reorder_scene
    (the image a fresh rt_create of S1 packs), by stream_cull_lab.image;
  * `chunks_reached`: how many (8 x 8 block, chunk) pairs of a frame's primary cones reach a chunk bound (pixel_cull_lab's predicate).
usage: python tests/tools/reorder_lab.py      prints the conditions of the GPU tests' scenes"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOOLS = os.path.join(ROOT, "tests", "tools")
sys.path.insert(0, ROOT)
sys.path.insert(0, TOOLS)
import pixel_cull_lab as PL  # noqa: E402
import stream_cull_lab as SC  # noqa: E402
import stream_scenes as S  # noqa: E402

W, H = 64, 48
QMAX = 2097151.0                  # the largest quantum: 21 bits per axis
SIZES = (64, 65, 129, 257, 320)   # n_us of the byte tests; 320 carries UNBOUNDED_AT
UNBOUNDED_AT = (5, 160, 311)      # ... spheres with r^2 <= 0, scattered through the index range
MIX_SEED = 77
MANY = 10000                      # the one large run

_LIB = None


def build():
    global _LIB
    if _LIB is None:
        out = os.path.join(TOOLS, "bin", "libreorder_lab.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(TOOLS, "reorder_lab.cpp"), "-o", out], check=True)
        lib = C.CDLL(out)
        lib.lab_stream_cull_keys.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lab_stream_cull_keys.restype = None
        _LIB = lib
    return _LIB


# ---- the key ---------------------------------------------------------------------------------------------------------------------------
def entries(centres, radii):
    """UsEntry records with the fields the key reads: k = -2 c, r (inf = no bounding radius)."""
    e = np.zeros(len(radii), SC.US_DTYPE)
    e["k"] = -2.0 * np.asarray(centres, np.float64)
    e["r"] = radii
    return e


def keys(e, lo, hi):
    e = np.ascontiguousarray(e)
    lo, hi = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(hi, np.float64)
    out = np.zeros(len(e), np.uint64)
    build().lab_stream_cull_keys(len(e), e.ctypes.data, lo.ctypes.data, hi.ctypes.data, out.ctypes.data)
    return out


def keys_numpy(e, lo, hi):
    """The rule restated: q = (uint64) ((c - lo) / span * 2097151.0) clamped to 0 .. 2097151, 0 where the span is not positive and finite;
    bit 3 b + 2 of the key is bit b of q_x, 3 b + 1 of q_y, 3 b of q_z; ~0 without a bounding radius."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = -0.5 * e["k"]
    m = np.zeros(len(e), np.uint64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(3):
            span = hi[k] - lo[k]
            ok = bool(span > 0.0 and np.abs(span) <= 1.7976931348623157e308)
            f = (c[:, k] - lo[k]) / span * QMAX if ok else np.zeros(len(e))
            f = np.where(f > 0.0, np.where(f < QMAX, f, QMAX), 0.0)
            q = f.astype(np.uint64)
            for b in range(21):
                m |= ((q >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + (2 - k))
    return np.where(e["r"] < np.inf, m, np.uint64(0xFFFFFFFFFFFFFFFF))


def box_of(e):
    """lo, hi over the bounded entries' centres, as stream_cull_image forms them (sequential < / >)."""
    c = -0.5 * e["k"][e["r"] < np.inf]
    return c.min(axis=0), c.max(axis=0)


def order_numpy(e):
    """slot -> index into e, by (key, orig): the order of stream_cull_image."""
    lo, hi = box_of(e)
    return np.lexsort((e["orig"], keys_numpy(e, lo, hi)))


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------
def sphere_parts(coefs):
    c = -0.5 * coefs[:, 16:19]
    return c, (c * c).sum(axis=1) - coefs[:, 19]


def with_centres(coefs, centres, unbounded=()):
    """The same unit spheres around other centres: r^2 kept, the spheres of `unbounded` get r^2 = -1 (no bounding radius)."""
    _, r2 = sphere_parts(coefs)
    r2 = r2.copy()
    r2[list(unbounded)] = -1.0
    out = coefs.copy()
    out[:, 16:19] = -2.0 * centres
    out[:, 19] = (centres * centres).sum(axis=1) - r2
    return out


def base_scene(pkg, n, unbounded=(), mirrors=False, depth=0, w=W, h=H, seed=S.FIELD_SEED):
    """S0: stream_scenes.field's spheres (raw coefficients, so that some can be given r^2 <= 0) under its two lights."""
    a = S.field(pkg, n, seed, w=w, h=h, mirrors=mirrors, depth=depth).arrays()
    c, _ = sphere_parts(a["coefs"])
    coefs = with_centres(a["coefs"], c, unbounded)
    sc = pkg.Scene.new(w, h, S.FOV, depth, (0.05, 0.1, 0.2))
    for q, col, refl in zip(coefs, a["albedo"], a["reflection"]):
        sc.add_object(q, col, float(refl))
    sc.add_light("directional", [0.2, -1.0, 0.6], (1.0, 0.95, 0.9), 1.2)
    sc.add_light("spherical", [4.0, 12.0, 2.0], (0.8, 0.9, 1.0), 500.0)
    return sc


def mix(coefs, seed=MIX_SEED, unbounded=(), jitter=0.05):
    """S1's coefficients: object i around the centre of object pi(i), pi a seeded permutation, plus a jitter; radii kept."""
    rng = np.random.default_rng(seed)
    c, _ = sphere_parts(coefs)
    pi = rng.permutation(len(c))
    return with_centres(coefs, c[pi] + rng.uniform(-jitter, jitter, c.shape), unbounded)


def ties(coefs, kind):
    """S1 of the tie tests: "two" distinct centres only, all centres in one "plane" (z fixed), all centres "identical"."""
    c, _ = sphere_parts(coefs)
    n = len(c)
    if kind == "two":
        new = np.where((np.arange(n) % 3 == 0)[:, None], np.array([-3.0, 1.0, 24.0]), np.array([4.0, -2.0, 27.0]))
    elif kind == "plane":
        new = c.copy()
        new[:, 2] = 25.0
        new = new[np.random.default_rng(5).permutation(n)]
    else:
        assert kind == "identical"
        new = np.tile(np.array([0.5, -0.25, 24.0]), (n, 1))
    return with_centres(coefs, new)


def scene_with(pkg, sc, coefs):
    """The scene `sc` with other coefficients (what a fresh context on S1 is created from)."""
    a = sc.arrays()
    out = pkg.Scene.new(a["width"], a["height"], S.FOV, a["max_reflections"], (0.05, 0.1, 0.2))
    for q, col, refl in zip(coefs, a["albedo"], a["reflection"]):
        out.add_object(q, col, float(refl))
    out.add_light("directional", [0.2, -1.0, 0.6], (1.0, 0.95, 0.9), 1.2)
    out.add_light("spherical", [4.0, 12.0, 2.0], (0.8, 0.9, 1.0), 500.0)
    return out


# ---- the images ----------------------------------------------------------------------------------------------------------------------------
def fresh(a, coefs):
    """(blob, bounds, words) a fresh rt_create packs for the scene with these coefficients."""
    return SC.image(dict(a, coefs=coefs))


def slot_order(a):
    """The `orig` column of the context's table as rt_create orders it for the arrays a."""
    blob, _, w = SC.image(a)
    return SC.table_of(blob, w)["orig"].copy()


def stale(a, coefs):
    """... and what a context created on `a` holds after rt_set_scene(coefs): the new entries in the old slots."""
    return SC.image(dict(a, coefs=coefs), slot_orig=slot_order(a))


def finite_radius_sum(bounds):
    r = bounds.view(SC.US_DTYPE)["r"]
    return float(r[np.isfinite(r)].sum())


def chunks_reached(pkg, sc, bounds):
    """The (block, chunk) pairs of the frame of `sc` whose cone reaches the chunk's bound: what the culled frame stages for its primary rays."""
    org, axis, cos_t = PL.block_cones(S.oracle_of(pkg, sc))
    b = bounds.view(SC.US_DTYPE)
    nb, nc = len(org), len(b)
    k = np.broadcast_to(b["k"][None], (nb, nc, 3)).reshape(-1, 3)
    r, q = np.broadcast_to(b["r"][None], (nb, nc)).reshape(-1), np.broadcast_to(b["inv_r"][None], (nb, nc)).reshape(-1)
    o, ax = np.broadcast_to(org[:, None], (nb, nc, 3)).reshape(-1, 3), np.broadcast_to(axis[:, None], (nb, nc, 3)).reshape(-1, 3)
    ct = np.broadcast_to(cos_t[:, None], (nb, nc)).reshape(-1)
    return int(PL.sphere_in_cone(k, r, q, o, ax, ct).sum())


def conditions(pkg, sc, coefs):
    """What the GPU tests rely on for (S0 = sc, S1 = coefs): dict(differs, stale_radii, fresh_radii, stale_reached, fresh_reached)."""
    a = sc.arrays()
    sb, sbounds, _ = stale(a, coefs)
    fb, fbounds, _ = fresh(a, coefs)
    s1 = scene_with(pkg, sc, coefs)
    return dict(differs=not np.array_equal(sb, fb), stale_radii=finite_radius_sum(sbounds), fresh_radii=finite_radius_sum(fbounds),
                stale_reached=chunks_reached(pkg, s1, sbounds), fresh_reached=chunks_reached(pkg, s1, fbounds))


def main():
    import __graft_entry__ as g
    pkg = g.load_package()
    for n in SIZES:
        ub = UNBOUNDED_AT if n == 320 else ()
        sc = base_scene(pkg, n, ub)
        print(n, conditions(pkg, sc, mix(sc.arrays()["coefs"], unbounded=ub)))


if __name__ == "__main__":
    main()
