"""Scenes, cases and oracle-side conditions of the culled streamed adaptive passes' tests (tests/test_stream_cull_adaptive_host.py,
tests/test_stream_cull_adaptive_gpu.py; csrc/rt_stream_cull_adaptive.hip) -- test infrastructure.  One list of
cases for both files.  Scenes are named by the keys of tests/tools/stream_adaptive_scenes.py, and
  ("cluster", swapped)   stream_cull_lab.cluster_scene (five chunks), swapped: the clusters exchanged as rt_set_scene's test moves them
  ("unbounded",)         test_stream_cull_host.raw_scene_with_unbounded_spheres (raw descriptors: the table's tail has no radius)
The wave cone on the CPU: tests/tools/wave_cone_lab.cpp compiles csrc/rt_wave_cone.hpp for the host; this file forms the waves as
ray_list_cull_kernel takes them -- 64 / k^2 consecutive entries of the refine list in the classifier's order (tiles, the four 8 x 8
blocks of a tile, a block's pixels row by row), lane bits i (sub-column) then j (sub-row); 64 consecutive slots of the halo rows for
k = 1 -- and asks the oracle which object every ray hits first."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOOLS = os.path.join(ROOT, "tests", "tools")
for p in (ROOT, os.path.join(ROOT, "tests"), TOOLS):
    if p not in sys.path:
        sys.path.insert(0, p)
import raw_desc_scenes as R  # noqa: E402
import ssaa_adaptive_ref as ada  # noqa: E402
import stream_adaptive_scenes as A  # noqa: E402
import stream_cull_lab as SC  # noqa: E402
import stream_scenes as S  # noqa: E402

O = S.O
F32, U8, INF, TAU, TAUS = A.F32, A.U8, A.INF, A.TAU, A.TAUS
SWAPPED = (SC.CLUSTERS[1][0], SC.CLUSTERS[0][0], (3.0, -6.0, 23.0))

# 1. fields: 65 spheres = two chunks, the second holding one entry; 128 = two full ones; 129, 193; mirrors at depths 1 and 4 (bounce
# segments run the culled shadow path from scattered hit points); 37 x 21: lanes outside the image, partial tiles
FIELDS = [("field", "sphere", 65, 64, 48, False, 0, 2.6), ("field", "sphere", 128, 64, 48, True, 1, 2.6), ("field", "sphere", 129, 64, 48, True, 1, 2.6),
          ("field", "sphere", 193, 64, 48, True, 1, 2.6), ("field", "sphere", 193, 64, 48, True, 4, 2.6), ("field", "sphere", 129, 37, 21, True, 1, 2.6)]
CLUSTER = ("cluster", False)
MIXED = ("mixed", 130, 64, 48)     # 65 spheres, 65 ellipsoids (the general-quadric table), two planes, mirrors
UNBOUNDED = ("unbounded",)
SCENES = FIELDS + [CLUSTER, MIXED, UNBOUNDED]
# 2. bands: (scene, world, band rows, k, format): the K = 1 halo kernel's cases
BANDS = [(("field", "sphere", 65, 37, 37, True, 1, 2.6), 3, 5, 2, F32), (("field", "sphere", 65, 37, 37, True, 1, 2.6), 2, 1, 4, U8)]
# 3. geometry
GEOMETRY = ("field", "sphere", 65, 64, 48, True, 1, 8.0)
GEO_COSES = (-INF, 0.9)


def _pkg():
    import __graft_entry__ as graft
    return graft.load_package()


def scene(pkg, key):
    """(scene or descriptor, camera)"""
    if key[0] == "cluster":
        return SC.cluster_scene(pkg, SWAPPED if key[1] else None), None
    if key[0] == "unbounded":
        from test_stream_cull_host import raw_scene_with_unbounded_spheres
        a = raw_scene_with_unbounded_spheres()
        return pkg.desc_from_arrays(64, 48, np.radians(S.FOV), (0.05, 0.1, 0.2), 0, a["coefs"], a["reflection"], a["albedo"], a["light_is_spherical"], a["light_p"],
                                    a["light_color"]), None
    return A.scene(pkg, key)


@functools.lru_cache(maxsize=None)
def oracle_scene(key):
    if key[0] == "cluster":
        pkg = _pkg()
        return S.oracle_of(pkg, scene(pkg, key)[0]), None
    if key[0] == "unbounded":
        from test_stream_cull_host import raw_scene_with_unbounded_spheres
        a = raw_scene_with_unbounded_spheres()
        osc = O.Scene(64, 48, 0.0, 0, (0.05, 0.1, 0.2))
        osc.vertical_fov = float(np.radians(S.FOV))
        for i in range(len(a["reflection"])):
            osc.add_object(a["coefs"][i], a["albedo"][i], a["reflection"][i])
        for i in range(2):
            osc.lights.append(R.stored_light(a["light_is_spherical"][i], a["light_p"][i], a["light_color"][i]))
        return osc, None
    return A.oracle_scene(key)


@functools.lru_cache(maxsize=None)
def frame(key, k=1):
    """The oracle's frame of scene `key` at k times its size."""
    osc, cam = oracle_scene(key)
    return osc.with_size(k * osc.width, k * osc.height).render(cam=cam, nthreads=8)


# ---- the lab ----------------------------------------------------------------------------------------------------------------------------
_LIB = None


def build():
    global _LIB
    if _LIB is None:
        SC.build()   # (the oracle's library, and the scene image)
        out = os.path.join(TOOLS, "bin", "libwave_cone_lab.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tools", "flopcount_shim"),
                        "-I" + os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-I" + TOOLS,
                        os.path.join(TOOLS, "wave_cone_lab.cpp"), "-o", out, "-L" + os.path.join(ROOT, "oracle"), "-lrt_oracle",
                        "-Wl,-rpath," + os.path.join(ROOT, "oracle")], check=True)
        lib = C.CDLL(out)
        vp = C.c_void_p
        lib.lab_sample_rays.argtypes = [vp, vp, C.c_uint64, vp, vp, vp]
        lib.lab_wave_cones.argtypes = [C.c_uint64, vp, vp, vp, vp, vp, vp]
        lib.lab_cone_verdicts.argtypes = [C.c_uint64, vp, vp, vp, C.c_double, vp]
        lib.lab_sample_rays.restype = lib.lab_wave_cones.restype = lib.lab_cone_verdicts.restype = None
        _LIB = lib
    return _LIB


@functools.lru_cache(maxsize=None)
def table(key):
    """(chunk of every object in the context's ordered unit-sphere table, or -1; the chunk bounds as US_DTYPE records)"""
    osc, _ = oracle_scene(key)
    blob, bounds, w = SC.image(SC.arrays_of_oracle(osc))
    assert w["cull"] == 1
    t = SC.table_of(blob, w)
    chunk = np.full(len(osc.objects), -1, np.int64)
    chunk[t["orig"]] = np.arange(len(t)) // SC.CHUNK
    return chunk, bounds.view(SC.US_DTYPE).copy()


def classifier_order(mask):
    """[(local row, x)] of the set pixels of a rank's rows in the classifier's append order: 16 x 16 tiles row by row, a tile's four 8 x 8
    blocks, a block's pixels row by row.  (On the device the blocks' runs land in the order of their atomics; a run is a block's.)"""
    rows, width = mask.shape
    out = []
    for ty in range((rows + 15) // 16):
        for tx in range((width + 15) // 16):
            for wave in range(4):
                y0, x0 = ty * 16 + (wave >> 1) * 8, tx * 16 + (wave & 1) * 8
                blk = mask[y0:y0 + 8, x0:x0 + 8]
                ys, xs = np.nonzero(blk)
                out += [(int(y0 + y), int(x0 + x)) for y, x in zip(ys, xs)]
    return out


def list_waves(key, k, tau, world=1, rank=0, band=8, mask=None):
    """The refine kernel's waves for the oracle's refined list of a rank: (xy int32 [n, 64, 2] on the k-times finer grid, -1 = no ray;
    pixels [n, 64 / k^2, 2] (x, global row), -1 = past the list's end).  mask: the whole frame's refine mask where it is not
    ssaa_adaptive_ref's (RT_FLAG_SSAA_GEOMETRY; world 1)."""
    p = frame(key)
    rows, mask = A.banded_mask(p, tau, world, rank, band) if mask is None else (np.arange(p.shape[0]), mask)
    items = classifier_order(mask)
    ppw = 64 // (k * k)
    n = (len(items) + ppw - 1) // ppw
    xy = np.full((n, 64, 2), -1, np.int32)
    pix = np.full((n, ppw, 2), -1, np.int64)
    for q, (lr, x) in enumerate(items):
        w, slot = divmod(q, ppw)
        y = int(rows[lr])
        pix[w, slot] = (x, y)
        for sub in range(k * k):
            i, j = sub % k, sub // k
            xy[w, slot * k * k + sub] = (k * x + i, k * y + j)
    return xy, pix


def halo_waves(key, world, rank, band):
    """The halo kernel's waves (K = 1): slot h = 2 b + side of band b of this rank, item q = h * width + x; xy [n, 64, 2], -1 = no ray."""
    p = frame(key)
    h, width = p.shape[:2]
    bands = A.band_bounds(h, world, rank, band)
    if world == 1 or not bands:
        return np.zeros((0, 64, 2), np.int32)
    n_items = 2 * len(bands) * width
    n = (n_items + 63) // 64
    xy = np.full((n * 64, 2), -1, np.int32)
    for q in range(n_items):
        slot, x = divmod(q, width)
        g0, nrows = bands[slot >> 1]
        gy = g0 + nrows if (slot & 1) else g0 - 1
        if 0 <= gy < h:
            xy[q] = (x, gy)
    return xy.reshape(n, 64, 2)


def cones_of(key, k, xy):
    """For waves xy [n, 64, 2] on the k-times finer grid: dict(dirs, use, owner, axis, cos_t, pick, bad) by the lab."""
    lib = build()
    osc, cam = oracle_scene(key)
    big = osc.with_size(k * osc.width, k * osc.height)
    sc = big.c_scene()
    cam = np.ascontiguousarray(O.IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
    xy = np.ascontiguousarray(xy, np.int32)
    n = len(xy)
    dirs, owner = np.zeros((n, 64, 3)), np.zeros((n, 64), np.int32)
    lib.lab_sample_rays(C.addressof(sc), cam.ctypes.data, n * 64, xy.ctypes.data, dirs.ctypes.data, owner.ctypes.data)
    use = np.ascontiguousarray(xy[:, :, 0] >= 0, np.uint8)
    axis, cos_t, pick, bad = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.lab_wave_cones(n, dirs.ctypes.data, use.ctypes.data, axis.ctypes.data, cos_t.ctypes.data, pick.ctypes.data, bad.ctypes.data)
    return dict(dirs=dirs, use=use, owner=owner, axis=axis, cos_t=cos_t, pick=pick, bad=bad, origin=cam[12:15].copy())


def verdicts(key, c):
    """sphere_in_cone about every chunk bound for every wave's cone: int32 [n, n_chunks] (waves without a cone: all ones)."""
    lib = build()
    _, bounds = table(key)
    b = np.ascontiguousarray(bounds)
    out = np.ones((len(c["pick"]), len(b)), np.int32)
    for w in np.flatnonzero(c["pick"] >= 0):
        ax = np.ascontiguousarray(c["axis"][w])
        lib.lab_cone_verdicts(len(b), b.ctypes.data, c["origin"].ctypes.data, ax.ctypes.data, float(c["cos_t"][w]), out[w].ctypes.data)
    return out


def check_waves(key, k, xy):
    """What the host test asserts per set of waves: dict(waves, used_lanes, bad_lanes, axis_not_a_lane, unsound, culled, hit_pairs)."""
    c = cones_of(key, k, xy)
    chunk, _ = table(key)
    v = verdicts(key, c)
    unsound = hit_pairs = not_a_lane = 0
    for w in range(len(xy)):
        if c["pick"][w] < 0:
            continue
        not_a_lane += int(not (c["use"][w, c["pick"][w]] and c["axis"][w].tobytes() == c["dirs"][w, c["pick"][w]].tobytes()))
        own = c["owner"][w][c["use"][w] != 0]
        hit = np.unique(chunk[own[own >= 0]])
        hit = hit[hit >= 0]
        hit_pairs += len(hit)
        unsound += int((v[w, hit] == 0).sum())
    return dict(waves=len(xy), used_lanes=int(c["use"].sum()), bad_lanes=int(c["bad"].sum()), axis_not_a_lane=not_a_lane, unsound=unsound,
                culled=int((v == 0).sum()), hit_pairs=hit_pairs, cones=c, verdicts=v)


def straddles_two_blocks(pix):
    """Some wave holds pixels of two different 8 x 8 blocks."""
    for w in pix:
        blocks = {(int(x) // 8, int(y) // 8) for x, y in w if x >= 0}
        if len(blocks) > 1:
            return True
    return False


# ---- the statistics test ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stats_expectation():
    """CLUSTER, k = 4, tau = -1: every pixel is listed in whole-block runs of 64, so a wave is four pixels of one block.  D0 = the primary
    chunk decisions, L = the (wave, chunk) pairs whose bound lies beyond the 1e-3 band of the Euclidean cone criterion
    (stream_cull_lab.bound_excess with the wave's cone), H = the pairs in which the oracle has a primary hit."""
    key, k = CLUSTER, 4
    xy, pix = list_waves(key, k, -1.0)
    r = check_waves(key, k, xy)
    _, bounds = table(key)
    h, w = frame(key).shape[:2]
    assert len(xy) == w * h * 16 // 64 and (pix[:, :, 0] >= 0).all() and not straddles_two_blocks(pix)
    c = r["cones"]
    beyond = 0
    for i in range(len(xy)):
        for e in bounds:
            if not np.isfinite(e["r"]):
                continue
            rec = np.concatenate([e["k"], [e["r"], e["inv_r"]], c["origin"], c["axis"][i], [c["cos_t"][i]]])
            x = SC.bound_excess("cone", rec)
            beyond += int(x is not None and x[0] > SC.BAND * x[2])
    return dict(D0=len(xy) * len(bounds), L=beyond, H=r["hit_pairs"], n_chunks=len(bounds), culled=r["culled"], unsound=r["unsound"], bad_lanes=r["bad_lanes"])
