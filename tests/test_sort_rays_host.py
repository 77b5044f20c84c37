"""rt_sort_rays and rt_permute (csrc/rt_sort_rays.hip), host side: the prototypes, what the entry points answer before
they look for a device, the work-space size, the key of csrc/rt_ray_sort_key.hpp against its numpy restatement on every ray set of
tests/test_sort_rays_gpu.py (the edge values of ray_sort_lab.edge_rays among them, and that they are what they are said to be), the class rule, the device's sort as tests/tools/ray_sort_lab.cpp restates it against numpy's stable argsort
(and, as a stand-alone program, under AddressSanitizer and UBSan), the build report's lines for the new kernels, and the condition that keeps
the GPU test of the work words from being vacuous."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

CSRC = os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")
KERNELS = ("init_box_kernel", "box_kernel", "keys_kernel", "histogram_kernel", "reduce_chunks_kernel", "scan_chunks_kernel", "scatter_kernel", "gather_rays_kernel",
           "permute_kernel")
PROTOTYPES = (
    r"size_t rt_sort_rays_work_bytes\(uint32_t n\);",
    r"int rt_sort_rays\(rt_ctx \*ctx, const rt_ray \*dev_rays, uint32_t n, rt_ray \*dev_sorted, uint32_t \*dev_perm, uint32_t \*dev_keys,\s*"
    r"void \*dev_work, size_t work_bytes, void \*stream, float \*ms\);",
    r"int rt_permute\(rt_ctx \*ctx, const uint32_t \*dev_perm, uint32_t n, const void \*dev_src, void \*dev_dst, uint32_t elem_bytes,\s*"
    r"uint32_t planes, int scatter, void \*stream, float \*ms\);")
EDGE_SEEDS = (3, 4)      # the seeds of tests/test_sort_rays_gpu.py::test_edge_values


@functools.lru_cache(maxsize=None)
def lab():
    import ray_sort_lab as SL
    SL.build()
    return SL


def sizes():
    c = lab().constants()
    T, W = c["T"], c["W"]
    return [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, min(W * T + 1, 1 << 20)]


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------
def test_prototypes_in_header_and_binding(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    for proto in PROTOTYPES:
        assert re.search(proto, hdr), proto
    assert "#define RT_ABI_VERSION 3" in hdr
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("rt_sort_rays_work_bytes", "rt_sort_rays", "rt_permute", "rt_launch_sort_rays", "rt_launch_permute"):
        assert re.search(rf"\bT {sym}\b", names), sym
        assert sym.startswith("rt_launch") or sym in pkg.ABI_SYMBOLS, sym
    lib = pkg.lib()
    assert lib.rt_sort_rays_work_bytes.restype == C.c_size_t and len(lib.rt_sort_rays.argtypes) == 10 and len(lib.rt_permute.argtypes) == 10
    for name in ("sort_work_bytes", "sort_rays_into", "permute_into", "sort_rays"):
        assert callable(getattr(pkg.Renderer, name)), name
    import inspect
    for name in ("trace", "occluded", "shade", "paths"):
        assert inspect.signature(getattr(pkg.Renderer, name)).parameters["sort"].default is False, name
    launch = open(os.path.join(CSRC, "rt_launch.h")).read()
    assert 'extern "C" hipError_t rt_launch_sort_rays(' in launch and 'extern "C" hipError_t rt_launch_permute(' in launch
    mk = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "Makefile")).read()
    assert "$(BUILD)/csrc/rt_sort_rays.o" in mk.split("\nOBJ ")[1].split("\n")[0]
    once = next(l for l in mk.splitlines() if l.startswith("$(BUILD)/csrc/rt_resolve.o") and "rt_sort_rays.o" in l)      # the rule that says -ffp-contract=off once
    assert "rt_planes.o" in once and "-ffp-contract=off" in mk.split(once)[1].split("\n\n")[0] and "RT_VARIANT" not in mk.split(once)[1].split("\n")[2]


def test_null_arguments_and_no_rays_are_refused_before_a_device_is_looked_for(pkg):
    """With NULL for the context nothing can be looked for; with a handle that is no context the refusal has to come before it is read."""
    lib = pkg.lib()
    one = C.c_void_p(16)
    assert lib.rt_sort_rays(None, one, 1, None, one, None, one, 1 << 20, None, None) == -1 and lib.rt_last_error() == b"rt_sort_rays: null argument"
    assert lib.rt_permute(None, one, 1, one, one, 4, 1, 0, None, None) == -1 and lib.rt_last_error() == b"rt_permute: null argument"
    fake = C.c_void_p(16)      # never dereferenced by what follows
    for args in ((fake, None, 1, None, one, None, one, 1 << 20), (fake, one, 1, None, None, None, one, 1 << 20), (fake, one, 1, None, one, None, None, 1 << 20)):
        assert lib.rt_sort_rays(*args, None, None) == -1 and lib.rt_last_error() == b"rt_sort_rays: null argument", args
    assert lib.rt_sort_rays(fake, one, 0, None, one, None, one, 1 << 20, None, None) == -1 and lib.rt_last_error() == b"rt_sort_rays: n is 0"
    for args in ((fake, None, 1, one, one, 4, 1, 0), (fake, one, 1, None, one, 4, 1, 0), (fake, one, 1, one, None, 4, 1, 0)):
        assert lib.rt_permute(*args, None, None) == -1 and lib.rt_last_error() == b"rt_permute: null argument", args
    assert lib.rt_permute(fake, one, 0, one, one, 4, 1, 0, None, None) == -1 and lib.rt_last_error() == b"rt_permute: n is 0"


def test_the_other_refusals_need_no_device_either(pkg):
    lib = pkg.lib()
    fake = C.c_void_p(16)
    n = 100
    need = lib.rt_sort_rays_work_bytes(n)
    rays, srt, perm, keys, work = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000

    def sort(**kw):
        a = dict(rays=rays, n=n, srt=srt, perm=perm, keys=keys, work=work, bytes=need)
        a.update(kw)
        rc = lib.rt_sort_rays(fake, C.c_void_p(a["rays"]), a["n"], C.c_void_p(a["srt"]) if a["srt"] else None, C.c_void_p(a["perm"]), C.c_void_p(a["keys"]) if a["keys"] else None,
                              C.c_void_p(a["work"]), a["bytes"], None, None)
        return rc, lib.rt_last_error().decode()
    for kw, word in ((dict(rays=rays + 8), "16-byte"), (dict(srt=srt + 8), "16-byte"), (dict(perm=perm + 2), "aligned"), (dict(keys=keys + 1), "aligned"),
                     (dict(bytes=need - 1), "work space"), (dict(bytes=0), "work space"),
                     (dict(srt=rays + 48), "overlap"), (dict(perm=rays + 4 * n), "overlap"), (dict(keys=perm), "overlap"), (dict(work=rays + 16), "overlap"),
                     (dict(work=perm - need + 4), "overlap"), (dict(srt=work + 256), "overlap"), (dict(keys=srt + 16), "overlap")):
        rc, msg = sort(**kw)
        assert rc == -1 and msg.startswith("rt_sort_rays: ") and word in msg, (kw, rc, msg)

    def permute(perm=perm, n=n, src=rays, dst=srt, elem=48, planes=1):
        rc = lib.rt_permute(fake, C.c_void_p(perm), n, C.c_void_p(src), C.c_void_p(dst), elem, planes, 0, None, None)
        return rc, lib.rt_last_error().decode()
    for kw, word in ((dict(elem=0), "elem_bytes"), (dict(elem=6), "elem_bytes"), (dict(elem=260), "elem_bytes"), (dict(elem=1 << 31), "elem_bytes"), (dict(planes=0), "planes"),
                     (dict(dst=rays), "overlaps"), (dict(dst=rays + 48 * n - 4), "overlaps"), (dict(src=srt + 48 * n * 2 - 16, planes=3), "overlaps"), (dict(dst=perm), "overlaps"),
                     (dict(dst=srt + 2, elem=4), "aligned")):
        rc, msg = permute(**kw)
        assert rc == -1 and msg.startswith("rt_permute: ") and word in msg, (kw, rc, msg)


def test_work_bytes(pkg):
    lib, SL = pkg.lib(), lab()
    assert lib.rt_sort_rays_work_bytes(0) == 0 == pkg.Renderer.sort_work_bytes(0)
    ns = sorted(set(sizes() + [2, 1000, (1 << 20) + 1, 1 << 24, (1 << 31) + 5, (1 << 32) - 1] + list(range(2040, 2060)) + list(range(16380, 16390))))
    got = [lib.rt_sort_rays_work_bytes(n) for n in ns]
    assert all(b >= a for a, b in zip(got, got[1:])) and got[0] > 0, got
    for n, b in zip(ns, got):
        assert b == SL.work_bytes(n) and b >= 16 * n, n      # the layout of the header, which the lab's restatement of the sort lives in
    assert got[-1] < 17 * ((1 << 32) - 1)


# ---- the key ------------------------------------------------------------------------------------------------------------------------------
def ray_sets():
    SL = lab()
    for n in sizes():
        yield f"tiled and shuffled, n = {n}", SL.tiled_shuffled(n)
    for name in SL.ADVERSARIAL:
        yield name, SL.adversarial(name)
    for order in ("row", "block", "shuffled"):
        yield f"statistics scene, {order}", SL.stats_rays(order)
    for seed in EDGE_SEEDS:
        yield f"edge values, seed {seed}", SL.edge_rays(2 * SL.constants()["T"] + 1, seed)


def test_header_and_restatement_give_the_same_keys():
    """Every ray set of the GPU tests; where the two differ, the header wins and the restatement is to be fixed."""
    SL = lab()
    count = 0
    for what, rays in ray_sets():
        k = SL.keys(rays)
        assert np.array_equal(k, SL.keys_numpy(rays)), what
        assert ((k == SL.constants()["class1"]) | (k < (1 << 30))).all(), what
        lo, hi = SL.box(rays)
        ok = SL.class0(rays)
        if ok.any():
            assert np.array_equal(lo, (rays["o"][ok] + 0.0).min(axis=0)) and np.array_equal(hi, (rays["o"][ok] + 0.0).max(axis=0)), what
        count += 1
    assert count == 9 + 9 + 3 + len(EDGE_SEEDS)
    c = SL.constants()
    assert 3 * c["origin_bits"] + 2 * c["dir_bits"] == 30 and c["class1"] == 0x80000000


def test_the_edge_values_are_what_they_are_said_to_be():
    """SL.edge_rays: every ray of class 0 (so every key is computed), the box SL.EDGE_BOX with both corners present, -0.0 among the origins,
    the sixty fixed directions, and a set that does not collapse into a few cells: more than n / 2 distinct keys, more than 1 000 of the
    4 096 origin cells.  Every origin coordinate is at most one representable value off a sixteenth of its axis, every direction's
    octahedral coordinates at most a few off a 512th."""
    SL = lab()
    c = SL.constants()
    n = 2 * c["T"] + 1
    for seed in EDGE_SEEDS:
        rays = SL.edge_rays(n, seed)
        assert len(rays) == n and SL.class0(rays).all()
        k = SL.keys(rays)
        assert (k < (1 << 30)).all() and len(np.unique(k)) > n // 2 and len(np.unique(k >> (2 * c["dir_bits"]))) > 1000, (seed, len(np.unique(k)))
        lo, hi = SL.box(rays)
        assert np.array_equal(lo, SL.EDGE_BOX[0]) and np.array_equal(hi, SL.EDGE_BOX[1]) and lo[0] == 0.0 and abs((hi[1] - lo[1]) / 2e-300 - 1.0) < 1e-15
        assert 0.0 < hi[2] - lo[2] < 2.3e-308 and (hi[2] - lo[2]) / 5e-324 % 16 == 0      # a sub-normal width, whole sixteenths of it representable
        assert np.array_equal(rays["o"][0], lo) and np.array_equal(rays["o"][1], hi)
        assert np.signbit(rays["o"][:, 0]).any() and not (rays["o"][:, 0] < 0.0).any()      # -0.0
        assert np.array_equal(rays["d"][:60:6], np.array(SL.EDGE_FIXED)) and np.signbit(rays["d"][42, 2]) and np.signbit(rays["d"][48, 0])
        assert k[0] >> (2 * c["dir_bits"]) == 0 and k[1] >> (2 * c["dir_bits"]) == (1 << (3 * c["origin_bits"])) - 1      # the corners' cells
        with np.errstate(all="ignore"):
            sixteenths = (rays["o"] - lo) / (hi - lo) * 16.0
            steps = (rays["o"][:, 2] - lo[2]) / 5e-324      # on the sub-normal axis a sixteenth is seven representable values
        assert (np.abs(sixteenths - np.round(sixteenths))[:, :2] < 1e-9).all() and (np.abs(steps - 7.0 * np.round(steps / 7.0)) <= 1.0).all()
        assert len(np.unique(SL.keys(rays[60:]) & ((1 << (2 * c["dir_bits"])) - 1))) > 1000      # ... nor do the directions


def test_the_adversarial_sets_are_what_their_names_say():
    SL = lab()
    for name in SL.ADVERSARIAL:
        rays = SL.adversarial(name)
        assert len(rays) == 2 * SL.constants()["T"] + 1
        SL.check_adversarial(name, rays)


def test_class_1_rays_all_get_the_one_key():
    SL = lab()
    base = SL.stats_rays("row")[:64].copy()
    odd = base.copy()
    kinds = []
    for i in range(64):
        o, d = base["o"][i].copy(), base["d"][i].copy()
        kind = i % 12
        if kind == 0:
            o[i % 3] = np.nan
        elif kind == 1:
            d[i % 3] = np.nan
        elif kind == 2:
            o[i % 3] = np.inf
        elif kind == 3:
            o[i % 3] = -np.inf
        elif kind == 4:
            d[i % 3] = np.inf
        elif kind == 5:
            d[i % 3] = -np.inf
        elif kind == 6:
            o[i % 3] = 1.0000001e100
        elif kind == 7:
            d[i % 3] = -1.0000001e100
        elif kind == 8:
            d[:] = 0.0
        elif kind == 9:
            d[:] = [1e-4, 0.0, 3e-4]      # |d|^2 = 1e-7 exactly in the reals, not above it as rounded
        elif kind == 10:
            d[:] = [0.0, -0.0, 1e-4]
        else:
            d[:] = [1e99, 1e99, 1e99]       # every component passes, |d|^2 is finite: class 0 -- the rule is the predicate's, nothing more
        odd["o"][i], odd["d"][i] = o, d
        kinds.append(kind)
    k = SL.keys(odd)
    kinds = np.array(kinds)
    assert (k[kinds != 11] == 0x80000000).all() and (k[kinds == 11] < (1 << 30)).all()
    assert np.array_equal(k, SL.keys_numpy(odd))
    assert not SL.class0(odd)[kinds != 11].any()
    # the boundary of the magnitude rule: exactly 1e100 is class 0
    edge = base[:2].copy()
    edge["o"][0, 0] = 1e100
    assert (SL.keys(edge) < (1 << 30)).all()


def test_class_1_rays_do_not_change_the_other_keys():
    SL = lab()
    rays = SL.tiled_shuffled(777)
    k = SL.keys(rays)
    more = np.concatenate([rays[:300], SL.adversarial("all odd", 50), rays[300:]])
    km = SL.keys(more)
    assert np.array_equal(np.concatenate([km[:300], km[350:]]), k) and (km[300:350] == 0x80000000).all()
    assert all(np.array_equal(a, b) for a, b in zip(SL.box(rays), SL.box(more)))


def test_negative_and_positive_zero_origins_give_one_key():
    SL = lab()
    rays = SL.tiled_shuffled(200)
    rays["o"][::2, 1] = 0.0      # an axis whose box starts at zero, half the rays on it
    rays["o"][1::2, 1] = np.arange(100) * 0.01 + 0.5
    neg = rays.copy()
    neg["o"][::4, 1] = -0.0
    assert np.signbit(neg["o"][::4, 1]).all() and not np.signbit(rays["o"][::4, 1]).any()
    assert np.array_equal(SL.keys(rays), SL.keys(neg)) and np.array_equal(SL.keys_numpy(neg), SL.keys(neg))
    lo, _ = SL.box(neg)
    assert lo[1] == 0.0 and not np.signbit(lo[1])
    allneg = rays.copy()
    allneg["o"][:, 1] = -0.0      # hi == lo == 0 either way
    allpos = allneg.copy()
    allpos["o"][:, 1] = 0.0
    assert np.array_equal(SL.keys(allneg), SL.keys(allpos))


# ---- the statistics scene -------------------------------------------------------------------------------------------------------------------
def test_sorted_statistics_are_not_vacuous():
    """What tests/test_sort_rays_gpu.py::test_work_words asks of the device is more than the shuffled rays give and no less than row order
    gives: L of the shuffled rays stably sorted by the key >= L of row order (a CPU figure: the distance rule of ray_cull_lab, float64)."""
    import ray_cull_lab as RL
    SL = lab()
    e, row, shuffled = SL.sorted_expectation("shuffled"), RL.expectation("row"), RL.expectation("shuffled")
    print({k: v for k, v in e.items() if k != "rays"}, "row", row["L"], "shuffled", shuffled["L"])
    assert e["D"] == row["D"] == 240 and e["n_chunks"] == 5
    assert e["L"] >= row["L"], (e["L"], row["L"])
    assert e["L"] > 4 * shuffled["L"]
    assert np.array_equal(e["rays"], shuffled["rays"][SL.host_perm(shuffled["rays"])])


# ---- the sort -----------------------------------------------------------------------------------------------------------------------------
def test_the_radix_emulation_is_numpys_stable_argsort():
    SL = lab()
    for name in SL.ADVERSARIAL:
        k, perm = SL.check_adversarial(name, SL.adversarial(name))
        got, ks = SL.radix_sort(k)
        assert np.array_equal(got, perm) and np.array_equal(ks, k[perm]), name
    for n in sizes():
        k = SL.keys(SL.tiled_shuffled(n))
        got, ks = SL.radix_sort(k)
        assert np.array_equal(got, np.argsort(k, kind="stable")) and np.array_equal(ks, np.sort(k)), n
    rng = np.random.default_rng(5)
    k = rng.integers(0, 1 << 32, 3 * SL.constants()["T"] + 17, dtype=np.uint64).astype(np.uint32)      # every bit of every digit
    got, ks = SL.radix_sort(k)
    assert np.array_equal(got, np.argsort(k, kind="stable"))


def test_the_radix_emulation_under_the_sanitizers():
    """The same file as a stand-alone program with -fsanitize=address,undefined: its key sets at the sizes around a wave, a tile and a scan
    chunk against std::stable_sort, every access inside the work space of the header's layout."""
    rc, out = lab().run_sanitized()
    print(out)
    assert rc == 0 and " 0 differ" in out and "ERROR" not in out and "runtime error" not in out, out


# ---- the build ----------------------------------------------------------------------------------------------------------------------------
def test_build_report_lists_the_new_kernels_without_spills():
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    mine = [l for l in open(report).read().splitlines() if l.startswith("rt_sort_rays.o")]
    assert len(mine) == len(KERNELS) + 3, mine      # permute_kernel: 16-byte vectors and words, gather and scatter
    for l in mine:
        assert re.search(r"SGPR spills\s+0\s+VGPR spills\s+0\s+scratch 0\b", l), l
        assert int(re.search(r"occupancy (\d+)\b", l).group(1)) >= 4, l
    remarks = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "csrc", "rt_sort_rays.o.remarks")).read()
    names = set(re.findall(r"Function Name: (\S+)", remarks))
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel
    assert not os.path.exists(os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "csrc", "rt_sort_rays_strict.o"))      # built once


def test_the_device_file_leaves_the_order_to_nothing_that_races():
    code = "\n".join(l.split("//")[0] for l in open(os.path.join(CSRC, "rt_sort_rays.hip")).read().splitlines())
    assert re.findall(r"\batomic\w+", code) == ["atomicMin", "atomicMax", "atomicAdd"]      # the box's extremes and the histogram's integer sum
    for word in ("hipMalloc", "hipMemcpy", "hipStreamSynchronize", "hipDeviceSynchronize", "hipEvent", "printf", "assert("):
        assert word not in code, word
    key = open(os.path.join(CSRC, "rt_ray_sort_key.hpp")).read()
    assert "ray_bound(o, d).cull" in key and "RB_PLAIN_ABOVE" not in key and "1e100" not in key.split("#ifndef")[1]      # the class is the predicate's, not restated
