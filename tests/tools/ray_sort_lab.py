#!/usr/bin/env python3
"""Host lab behind rt_sort_rays (tests/tools/ray_sort_lab.cpp).  No GPU.
  * keys(rays), box(rays): csrc/rt_ray_sort_key.hpp compiled for the host -- the header is the key's definition;
  * keys_numpy(rays): a numpy restatement of it, held to the header bit for bit (tests/test_sort_rays_host.py);
  * radix_sort(keys): the plain C++ restatement of the device's sort (histogram, levelled scan, tile ranking) over the header's constants and
    work-space layout; run_sanitized(): the same file as a stand-alone program under AddressSanitizer and UBSan;
  * sorted_expectation(order): ray_cull_lab.ray_stats_expectation of the statistics scene for the rays of `order` stably sorted by the key;
  * the ray sets of tests/test_sort_rays_gpu.py.
usage: python tests/tools/ray_sort_lab.py      the CPU proxy figures of DESIGN.md section 31 and the sanitized run"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOOLS = os.path.join(ROOT, "tests", "tools")
sys.path.insert(0, ROOT)
sys.path.insert(0, TOOLS)
import ray_cull_lab as RL  # noqa: E402

RAY_DTYPE = np.dtype([("o", np.float64, 3), ("d", np.float64, 3)])
_SRC = os.path.join(TOOLS, "ray_sort_lab.cpp")
_INC = ["-I" + os.path.join(ROOT, "tools", "flopcount_shim"), "-I" + os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")]
_FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-Wno-subobject-linkage"]
_LIB = []


def build():
    if not _LIB:
        out = os.path.join(TOOLS, "bin", "libray_sort_lab.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++"] + _FLAGS + ["-fPIC", "-shared"] + _INC + [_SRC, "-o", out], check=True)
        lib = C.CDLL(out)
        lib.lab_work_bytes.restype = C.c_uint64
        lib.lab_work_bytes.argtypes = [C.c_uint32]
        _LIB.append(lib)
    return _LIB[0]


def run_sanitized():
    """The sort's restatement as a stand-alone program of its own under -fsanitize=address,undefined: (return code, output)."""
    exe = os.path.join(TOOLS, "bin", "ray_sort_lab_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wno-subobject-linkage", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DRAY_SORT_LAB_MAIN"] + _INC + [_SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    return r.returncode, r.stdout + r.stderr


@functools.lru_cache(maxsize=None)
def constants():
    """dict(T: pairs per workgroup and pass, W: tiles one scan workgroup covers in one step, origin_bits, dir_bits, class1, passes)."""
    out = (C.c_uint32 * 8)()
    build().lab_sort_constants(out)
    return dict(T=out[0], W=out[1], origin_bits=out[2], dir_bits=out[3], class1=out[4], passes=out[5], threads=out[6], items=out[7])


def work_bytes(n):
    return int(build().lab_work_bytes(int(n)))


def _flat(rays):
    r = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
    return r, np.ascontiguousarray(r.view(np.float64).reshape(-1, 6))


def keys(rays):
    r, flat = _flat(rays)
    out = np.zeros(len(r), dtype=np.uint32)
    build().lab_keys(C.c_uint64(len(r)), flat.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out


def box(rays):
    r, flat = _flat(rays)
    out = np.zeros(6)
    build().lab_box(C.c_uint64(len(r)), flat.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)))
    return out[:3].copy(), out[3:].copy()


def host_perm(rays):
    return np.argsort(keys(rays), kind="stable").astype(np.uint32)


def radix_sort(k):
    """(perm, sorted keys) of the device's sort as the lab restates it."""
    k = np.ascontiguousarray(k, dtype=np.uint32)
    perm, ks = np.zeros(len(k), np.uint32), np.zeros(len(k), np.uint32)
    p = C.POINTER(C.c_uint32)
    assert build().lab_radix_sort(C.c_uint32(len(k)), k.ctypes.data_as(p), perm.ctypes.data_as(p), ks.ctypes.data_as(p)) == 0
    return perm, ks


# ---- the key, restated -------------------------------------------------------------------------------------------------------------------
def class0(rays):
    """rtm::ray_bound(o, d).cull: every |component| <= 1e100 (a NaN fails), 1e-7 < |d|^2 < inf."""
    r, _ = _flat(rays)
    o, d = r["o"], r["d"]
    with np.errstate(all="ignore"):
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        small = (np.abs(o) <= 1e100).all(axis=1) & (np.abs(d) <= 1e100).all(axis=1)
        return small & (dd > 1e-7) & (dd < np.inf)


def _spread(v, bits, step):
    out = np.zeros(len(v), dtype=np.uint32)
    for b in range(bits):
        out |= ((v >> np.uint32(b)) & np.uint32(1)) << np.uint32(step * b)
    return out


def _cell(x, cells):
    with np.errstate(all="ignore"):
        f = np.floor(x * float(cells))
        return np.where(f >= cells - 1, cells - 1, np.where(f > 0, f, 0)).astype(np.uint32)


def keys_numpy(rays):
    c = constants()
    r, _ = _flat(rays)
    ok = class0(r)
    out = np.full(len(r), c["class1"], dtype=np.uint32)
    if not ok.any():
        return out
    o, d = r["o"][ok] + 0.0, r["d"][ok]
    lo, hi = o.min(axis=0), o.max(axis=0)
    mo = np.zeros(len(o), dtype=np.uint32)
    for a in range(3):
        if hi[a] != lo[a]:
            mo |= _spread(_cell((o[:, a] - lo[a]) / (hi[a] - lo[a]), 1 << c["origin_bits"]), c["origin_bits"], 3) << np.uint32(a)
    s = (np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])
    nx, ny, nz = d[:, 0] / s, d[:, 1] / s, d[:, 2] / s
    fold = nz < 0.0
    u = np.where(fold, (1.0 - np.abs(ny)) * np.where(nx < 0.0, -1.0, 1.0), nx)
    v = np.where(fold, (1.0 - np.abs(nx)) * np.where(ny < 0.0, -1.0, 1.0), ny)
    cells = 1 << c["dir_bits"]
    md = _spread(_cell(u * 0.5 + 0.5, cells), c["dir_bits"], 2) | (_spread(_cell(v * 0.5 + 0.5, cells), c["dir_bits"], 2) << np.uint32(1))
    out[ok] = (mo << np.uint32(2 * c["dir_bits"])) | md
    return out


# ---- the statistics scene ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sorted_expectation(order="shuffled"):
    """ray_cull_lab.ray_stats_expectation of the statistics scene, for the rays of `order` stably sorted by the host key (the function
    itself, with its ordering step followed by the sort)."""
    import __graft_entry__ as graft
    pkg = graft.load_package()
    plain = RL.ordered

    def ordered_then_sorted(rays, w, h, o):
        r = plain(rays, w, h, o)
        return np.ascontiguousarray(r[host_perm(r)])
    RL.ordered = ordered_then_sorted
    try:
        return RL.ray_stats_expectation(pkg, RL.B.bounce_scene(pkg), order)
    finally:
        RL.ordered = plain


# ---- ray sets ----------------------------------------------------------------------------------------------------------------------------
def stats_rays(order="shuffled"):
    return RL.expectation(order)["rays"]


def odd_ray(kind, i):
    """A ray nothing can be culled for (class 1), of one of the odd kinds."""
    o, d = np.array([0.0, 0.0, -2.0]) + i * 1e-3, np.array([0.0, 0.0, 1.0])
    kind %= 7
    if kind == 0:
        d = np.zeros(3)
    elif kind == 1:
        d = np.array([1e-4, 0.0, 2e-4])       # |d|^2 <= 1e-7
    elif kind == 2:
        o[i % 3] = np.nan
    elif kind == 3:
        d = np.array([1e120, 0.0, 1.0])       # beyond 1e100
    elif kind == 4:
        o[i % 3] = np.inf
    elif kind == 5:
        d = np.array([0.0, -np.inf, 1.0])
    else:
        o[i % 3] = -1e101
    return o, d


def tiled_shuffled(n, seed=31):
    """n of the statistics scene's primary rays, tiled and shuffled; copy k of a ray starts k thousandths of its direction further on, so
    that the origins differ."""
    base = stats_rays("row")
    reps = -(-n // len(base))
    r = np.tile(base, reps)
    k = np.repeat(np.arange(reps), len(base)).astype(np.float64)
    r["o"] = r["o"] + (1e-3 * k)[:, None] * r["d"]
    idx = np.random.default_rng(seed).permutation(len(r))[:n]
    return np.ascontiguousarray(r[idx])


EDGE_BOX = (np.array([0.0, 1e-300, -48 * 5e-324]), np.array([3.0, 3e-300, 64 * 5e-324]))      # an axis from 0.0, one 2e-300 wide, one 112 sub-normal steps wide
EDGE_FIXED = ([1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0],
              [0.3, -0.2, 0.0], [0.3, -0.2, -0.0], [-0.0, 0.0, -1.0], [3.2e-4, 0.0, 0.0])


def _ulp_moved(x, move):
    """x one representable value down, where it is, or one up (move = -1, 0, +1 per element)."""
    return np.where(move < 0, np.nextafter(x, -np.inf), np.where(move > 0, np.nextafter(x, np.inf), x))


def edge_rays(n, seed):
    """n class-0 rays at the values where one rounding decides the key's cell (csrc/rt_ray_sort_key.hpp claims host and device agree there).
    Origins: every coordinate on lo + (hi - lo) k / 16 of EDGE_BOX, k in 0 .. 16, one value down, as it is or one up, clipped to the box;
    rays 0 and 1 are the two corners; -0.0 stands among the zeroes of the axis that starts at 0.0.  Directions: the octahedral
    coordinates (a / 256 - 1, b / 256 - 1), a, b in 0 .. 512 -- the cell boundaries of the direction's 512 x 512 grid -- unfolded (to the
    lower hemisphere where |u| + |v| > 1), scaled by 10^U(-3, 90), every component moved as the origins' are; the first sixty rows have the
    directions of EDGE_FIXED instead, six each: the axes (u or v * 0.5 + 0.5 == 1.0, the clamp), n.z == +-0.0 against the fold, |d|^2 just
    above 1e-7."""
    rng = np.random.default_rng(seed)
    lo, hi = EDGE_BOX
    r = np.zeros(n, dtype=RAY_DTYPE)
    k = rng.integers(0, 17, (n, 3))
    k[0], k[1] = 0, 16
    move = rng.integers(-1, 2, (n, 3))
    move[:2] = 0
    with np.errstate(under="ignore"):
        o = np.clip(_ulp_moved(lo + (hi - lo) * k / 16.0, move), lo, hi)
    o[:, 0] = np.where((k[:, 0] == 0) & (move[:, 0] < 0), -0.0, o[:, 0])
    r["o"] = o
    a, b = rng.integers(0, 513, n), rng.integers(0, 513, n)
    u, v = a / 256.0 - 1.0, b / 256.0 - 1.0
    z = 1.0 - np.abs(u) - np.abs(v)
    x = np.where(z < 0.0, (1.0 - np.abs(v)) * np.where(u < 0.0, -1.0, 1.0), u)
    y = np.where(z < 0.0, (1.0 - np.abs(u)) * np.where(v < 0.0, -1.0, 1.0), v)
    d = np.stack([x, y, z], axis=1) * (10.0 ** rng.uniform(-3.0, 90.0, n))[:, None]
    r["d"] = _ulp_moved(d, rng.integers(-1, 2, (n, 3)))
    fixed = np.repeat(np.array(EDGE_FIXED), 6, axis=0)
    r["d"][:len(fixed)] = fixed[:n]
    return r


ADVERSARIAL = ("all equal", "two alternating", "top digit", "lowest digit", "sorted", "reversed", "one origin", "quarter odd", "all odd")


def adversarial(name, n=None):
    """The ray sets of the GPU tests' adversarial keys, n = 2T + 1 rays each.  What the host key must come out as is asserted by
    check_adversarial (the host test runs it, the GPU test runs it first)."""
    c = constants()
    n = 2 * c["T"] + 1 if n is None else n
    rng = np.random.default_rng(4000 + ADVERSARIAL.index(name))
    r = np.zeros(n, dtype=RAY_DTYPE)
    if name == "all equal":
        r["o"], r["d"] = [0.25, -1.0, 3.0], [0.3, 0.2, 1.0]
    elif name == "two alternating":
        r["o"] = [0.0, 0.0, -2.0]
        r["d"] = np.where((np.arange(n) % 2 == 0)[:, None], [0.3, 0.2, 1.0], [-0.5, 0.1, -1.0])
    elif name == "top digit":
        # origins on the cells 0, 4, 8, 12 of every axis (bits 2 and 3 of q: the key's top digit), one direction; the box's upper corner has
        # to be some ray's origin and lies in cell 15: the last ray, the only one whose lower digits differ
        cells = rng.integers(0, 4, (n, 3)) * 4
        r["o"] = (cells + 0.5) / 16.0
        r["o"][0] = 0.0
        r["o"][-1] = 1.0
        r["d"] = [0.3, 0.2, 1.0]
    elif name == "lowest digit":
        # one origin; directions in the 16 x 16 cells (256 + a, 256 + b) of the octahedral map: the low four bits of qu and qv, the key's lowest digit
        a, b = rng.integers(0, 16, n), rng.integers(0, 16, n)
        u, v = (256 + a + 0.5) / 512.0 * 2.0 - 1.0, (256 + b + 0.5) / 512.0 * 2.0 - 1.0
        r["o"] = [1.0, 2.0, 3.0]
        r["d"] = np.stack([u, v, 1.0 - np.abs(u) - np.abs(v)], axis=1) * 3.0
    elif name in ("sorted", "reversed"):
        s = tiled_shuffled(n, 37)
        s = s[host_perm(s)]
        r = np.ascontiguousarray(s if name == "sorted" else s[::-1])
    elif name == "one origin":
        s = stats_rays("shuffled")
        r = np.ascontiguousarray(np.tile(s, -(-n // len(s)))[:n])
    elif name == "quarter odd":
        r = tiled_shuffled(n, 41)
        for i in range(1, n, 4):
            r["o"][i], r["d"][i] = odd_ray(i // 4, i)
    elif name == "all odd":
        for i in range(n):
            r["o"][i], r["d"][i] = odd_ray(i, i)
    else:
        raise KeyError(name)
    return r


def check_adversarial(name, rays):
    """The host key of adversarial(name) is what the name says; returns (keys, the stable argsort)."""
    c = constants()
    k = keys(rays)
    n = len(k)
    perm = np.argsort(k, kind="stable").astype(np.uint32)
    if name == "all equal":
        assert (k == k[0]).all() and k[0] != c["class1"] and np.array_equal(perm, np.arange(n))
    elif name == "two alternating":
        assert len(np.unique(k)) == 2 and (k[0::2] == k[0]).all() and (k[1::2] == k[1]).all() and k[0] > k[1]
    elif name == "top digit":
        assert len(np.unique(k[:-1] & 0x00FFFFFF)) == 1 and len(np.unique(k[:-1] >> 24)) == 64 and (k >> 24 < 64).all()
    elif name == "lowest digit":
        assert len(np.unique(k >> 8)) == 1 and len(np.unique(k & 0xFF)) == 256
    elif name == "sorted":
        assert (np.diff(k.astype(np.int64)) >= 0).all() and len(np.unique(k)) > n // 8
    elif name == "reversed":
        assert (np.diff(k.astype(np.int64)) <= 0).all() and len(np.unique(k)) > n // 8
    elif name == "one origin":
        assert (rays["o"] == rays["o"][0]).all() and (k >> (2 * c["dir_bits"]) == 0).all() and len(np.unique(k)) > 100
    elif name == "quarter odd":
        odd = np.arange(n) % 4 == 1
        assert (k[odd] == c["class1"]).all() and (k[~odd] < c["class1"]).all()
        assert np.array_equal(perm[n - odd.sum():], np.nonzero(odd)[0])       # they stand last, in input order
    elif name == "all odd":
        assert (k == c["class1"]).all() and np.array_equal(perm, np.arange(n)) and np.isinf(box(rays)[0]).all()
    return k, perm


def main():
    rc, out = run_sanitized()
    print(out.strip())
    for order in RL.ORDERS:
        print(f"statistics scene, {order:8s}: L = {RL.expectation(order)['L']:3d} of 240 (CPU proxy); stably sorted by the key: L = {sorted_expectation(order)['L']:3d}")
    sys.exit(rc)


if __name__ == "__main__":
    main()
