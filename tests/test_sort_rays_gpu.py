"""rt_sort_rays and rt_permute on the GPU (csrc/rt_sort_rays.hip).  The order is held to the host: the key of
csrc/rt_ray_sort_key.hpp compiled for the host (tests/tools/ray_sort_lab.py) and numpy's stable argsort, bit for bit; the results of the ray
queries by way of sort, query and scatter are held to the direct call on the caller's order, bit for bit.  "Four flags" is RT_FLAG_STREAM |
RT_FLAG_STREAM_QUERIES | RT_FLAG_STREAM_CULL | RT_FLAG_STREAM_CULL_RAYS.  T = the sort's tile (pairs per workgroup and pass), W = the tiles one
scan workgroup covers in one step, both from the header's constants.  The host-side conditions are in tests/test_sort_rays_host.py.
Sections 8 and 9 take every loop of the file past the cap of its grid (G workgroups: the tile loop two and three times, permute_kernel three
trips and more, the scan with three levels) against a reference formed on the device, and the key to the values where one rounding decides
the cell (SL.edge_rays; DESIGN.md section 8, "Past one grid trip")."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import bounce_cull_lab as BL  # noqa: E402
import query_table_scenes as Q  # noqa: E402
import ray_cull_lab as RL  # noqa: E402
import ray_sort_lab as SL  # noqa: E402
import rays_ref  # noqa: E402
import stream_query_scenes as B  # noqa: E402
import stream_scenes as S  # noqa: E402
from test_paths_gpu import ends_of  # noqa: E402
from test_rays_gpu import hits_of, to_device, trace_dev  # noqa: E402
from test_stream_queries_gpu import assert_same_outputs, ray_outputs  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64          # words of guard band behind every output
FILL = 0xA5         # ... and what they hold
T, W = SL.constants()["T"], SL.constants()["W"]
SIZES = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, min(W * T + 1, 1 << 20)]      # (the scan has two levels from 9 tiles on: 2^20 rays are 512)
ELEMS = (4, 8, 16, 48, 48, 16)      # ..., sizeof(rt_hit), sizeof(rt_path_end)


@pytest.fixture(autouse=True)
def the_feature(pkg):
    assert callable(pkg.Renderer.sort_rays_into) and pkg.HIT_DTYPE.itemsize == ELEMS[4] and pkg.PATH_END_DTYPE.itemsize == ELEMS[5]


def four(pkg):
    return pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_QUERIES | pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_RAYS


@pytest.fixture(scope="module")
def any_ctx(pkg):
    """A context of no matter which scene: the two calls take nothing of it but the device."""
    r = pkg.Renderer(Q.small_case(pkg, ("sphere", 65)).sc, device=0)
    yield r
    r.cleanup_update()


def guarded(n_bytes):
    """A device buffer of n_bytes and a guard band, all FILL."""
    import torch
    return torch.full((n_bytes + 4 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0")


def guard_untouched(buf, n_bytes):
    return bool((buf[n_bytes:] == FILL).all().item())


class Sorted:
    """rt_sort_rays of host rays on guarded device buffers; the outputs as numpy arrays."""

    def __init__(self, r, rays, want_sorted=True, want_keys=True, stream=None, timed=True):
        import torch
        self.n = n = len(rays)
        self.d_rays = to_device(rays)
        self.b_sorted, self.b_perm, self.b_keys = (guarded(48 * n) if want_sorted else None), guarded(4 * n), (guarded(4 * n) if want_keys else None)
        self.work_bytes = r.sort_work_bytes(n)
        self.b_work = guarded(self.work_bytes)
        torch.cuda.synchronize()
        ms = r.sort_rays_into(self.d_rays.data_ptr(), n, self.b_sorted.data_ptr() if want_sorted else None, self.b_perm.data_ptr(),
                              self.b_keys.data_ptr() if want_keys else None, self.b_work.data_ptr(), self.work_bytes, stream=stream, timed=timed)
        assert (ms is not None and ms >= 0.0) if timed else ms is None
        torch.cuda.synchronize()
        self.perm = self.b_perm[:4 * n].cpu().numpy().view(np.uint32)
        self.keys = self.b_keys[:4 * n].cpu().numpy().view(np.uint32) if want_keys else None
        self.sorted = self.b_sorted[:48 * n].cpu().numpy().view(rays_ref.RAY_DTYPE) if want_sorted else None

    def guards_untouched(self):
        return all(guard_untouched(b, k * self.n) for b, k in ((self.b_sorted, 48), (self.b_perm, 4), (self.b_keys, 4)) if b is not None) and \
            guard_untouched(self.b_work, self.work_bytes)


def check_sort(r, rays, what):
    """Everything test 1 asks of one sort; returns the device's perm."""
    k = SL.keys(rays)
    want = np.argsort(k, kind="stable").astype(np.uint32)
    s = Sorted(r, rays)
    n = len(rays)
    assert np.array_equal(np.sort(s.perm), np.arange(n, dtype=np.uint32)), (what, "perm is a permutation")
    assert (np.diff(s.keys.astype(np.int64)) >= 0).all(), (what, "keys are non-decreasing")
    same = np.diff(s.keys.astype(np.int64)) == 0
    assert (np.diff(s.perm.astype(np.int64))[same] > 0).all(), (what, "equal keys keep ascending perm")
    assert np.array_equal(s.keys, k[s.perm]), (what, "the device's keys are the host's")
    assert np.array_equal(s.perm, want), (what, "perm is the host's stable argsort")
    assert s.sorted.tobytes() == np.ascontiguousarray(rays[s.perm]).tobytes(), (what, "sorted == rays[perm]")
    assert s.guards_untouched(), (what, "guard bands")
    again = Sorted(r, rays)
    assert again.perm.tobytes() == s.perm.tobytes() and again.keys.tobytes() == s.keys.tobytes() and again.sorted.tobytes() == s.sorted.tobytes(), (what, "a second call")
    return s.perm


# ---- 1. sizes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sizes(any_ctx, n):
    check_sort(any_ctx, SL.tiled_shuffled(n), n)


def test_optional_outputs_may_be_null(any_ctx):
    rays = SL.tiled_shuffled(T + 1)
    full = Sorted(any_ctx, rays)
    bare = Sorted(any_ctx, rays, want_sorted=False, want_keys=False, timed=False)
    assert bare.perm.tobytes() == full.perm.tobytes() and bare.guards_untouched()


# ---- 2. adversarial keys ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SL.ADVERSARIAL)
def test_adversarial_keys(any_ctx, name):
    rays = SL.adversarial(name)
    assert len(rays) == 2 * T + 1
    k, want = SL.check_adversarial(name, rays)      # the host key is what the name says
    perm = check_sort(any_ctx, rays, name)
    if name in ("all equal", "all odd", "sorted"):
        assert np.array_equal(perm, np.arange(len(rays)))
    if name == "quarter odd":
        odd = np.nonzero(np.arange(len(rays)) % 4 == 1)[0]
        assert np.array_equal(perm[len(rays) - len(odd):], odd)      # last, in input order


# ---- 3. rt_permute ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 2 * T + 1])
def test_permute_gather_then_scatter_is_the_identity(any_ctx, n):
    import torch
    r = any_ctx
    rng = np.random.default_rng(600 + n)
    perm = rng.permutation(n).astype(np.uint32)
    d_perm = torch.from_numpy(perm.view(np.int32)).to("cuda:0")
    for elem in ELEMS:
        for planes in (1, 3):
            src = rng.integers(0, 256, (planes, n, elem), dtype=np.uint8)
            nbytes = src.size
            d_src = torch.from_numpy(src).to("cuda:0")
            mid, back = guarded(nbytes), guarded(nbytes)
            torch.cuda.synchronize()
            r.permute_into(d_perm.data_ptr(), n, d_src.data_ptr(), mid.data_ptr(), elem, planes=planes)
            r.permute_into(d_perm.data_ptr(), n, mid.data_ptr(), back.data_ptr(), elem, planes=planes, scatter=True, timed=False)
            torch.cuda.synchronize()
            got = mid[:nbytes].cpu().numpy().reshape(planes, n, elem)
            assert np.array_equal(got, src[:, perm]), (elem, planes, "gather is numpy's fancy indexing")
            assert back[:nbytes].cpu().numpy().tobytes() == src.tobytes(), (elem, planes, "gather then scatter")
            assert guard_untouched(mid, nbytes) and guard_untouched(back, nbytes), (elem, planes)
    # 16-byte records on pointers that only allow words
    src = rng.integers(0, 256, (n, 48), dtype=np.uint8)
    d_src, out = guarded(48 * n + 4), guarded(48 * n + 4)
    d_src[4:4 + 48 * n] = torch.from_numpy(src.reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    r.permute_into(d_perm.data_ptr(), n, d_src.data_ptr() + 4, out.data_ptr() + 4, 48)
    torch.cuda.synchronize()
    assert np.array_equal(out[4:4 + 48 * n].cpu().numpy().reshape(n, 48), src[perm]) and guard_untouched(out, 48 * n + 4) and (out[:4] == FILL).all().item()


def test_refusals_write_nothing(pkg, any_ctx):
    import torch
    r = any_ctx
    n = 100
    need = r.sort_work_bytes(n)
    rays, srt, perm, keys, work = guarded(48 * n), guarded(48 * n), guarded(4 * n), guarded(4 * n), guarded(need)
    src, dst = guarded(48 * n * 3), guarded(48 * n * 3)
    bufs = (rays, srt, perm, keys, work, src, dst)
    torch.cuda.synchronize()
    p = {k: v.data_ptr() for k, v in dict(rays=rays, srt=srt, perm=perm, keys=keys, work=work, src=src, dst=dst).items()}
    assert all(v % 16 == 0 for v in p.values())

    def sort(**kw):
        a = dict(rays=p["rays"], n=n, srt=p["srt"], perm=p["perm"], keys=p["keys"], work=p["work"], bytes=need)
        a.update(kw)
        return lambda: r.sort_rays_into(a["rays"], a["n"], a["srt"], a["perm"], a["keys"], a["work"], a["bytes"], timed=False)

    def permute(**kw):
        a = dict(perm=p["perm"], n=n, src=p["src"], dst=p["dst"], elem=48, planes=1)
        a.update(kw)
        return lambda: r.permute_into(a["perm"], a["n"], a["src"], a["dst"], a["elem"], planes=a["planes"], timed=False)
    refused = [sort(rays=None), sort(perm=None), sort(work=None), sort(n=0), sort(rays=p["rays"] + 8), sort(srt=p["srt"] + 8), sort(perm=p["perm"] + 2), sort(keys=p["keys"] + 2),
               sort(bytes=need - 1), sort(srt=p["rays"] + 48), sort(perm=p["rays"]), sort(keys=p["perm"] + 4), sort(work=p["srt"] + 16), sort(keys=p["work"] + 256),
               permute(perm=None), permute(src=None), permute(dst=None), permute(n=0), permute(elem=0), permute(elem=6), permute(elem=260), permute(planes=0),
               permute(dst=p["src"] + 48), permute(src=p["dst"] + 48 * n * 3 - 48, planes=3)]
    for k, call in enumerate(refused):
        with pytest.raises(pkg.RtError) as e:
            call()
        assert e.value.code == -1, (k, e.value.message)
    torch.cuda.synchronize()
    assert all(bool((b == FILL).all().item()) for b in bufs)


# ---- 4. results are unchanged -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stats_case():
    import __graft_entry__ as graft
    pkg = graft.load_package()
    sc = BL.bounce_scene(pkg)
    return Q.Case(sc, S.oracle_of(pkg, sc), True)


def shuffled_case(c, seed):
    idx = np.random.default_rng(seed).permutation(len(c.rays))
    return np.ascontiguousarray(c.rays[idx]), np.ascontiguousarray(c.t_max[idx])


def sorted_outputs(r, rays, t_max):
    """ray_outputs by way of rt_sort_rays: every entry point on the sorted rays (t_max gathered), every output scattered back."""
    import torch
    n, m = len(rays), r._max_segments(None)
    s = Sorted(r, rays, want_keys=False)
    assert np.array_equal(s.perm, SL.host_perm(rays))
    perm, srt = s.b_perm.data_ptr(), s.b_sorted.data_ptr()

    def fresh(shape, dtype, fill):
        return torch.full(shape, fill, dtype=dtype, device="cuda:0")

    def back(t, elem, planes=1):
        out = torch.empty_like(t)
        torch.cuda.synchronize()
        r.permute_into(perm, n, t.data_ptr(), out.data_ptr(), elem, planes=planes, scatter=True)
        torch.cuda.synchronize()
        return out
    d_tmax, g_tmax = torch.from_numpy(t_max.copy()).to("cuda:0"), fresh((n,), torch.float64, 0.0)
    hits, rgba, rec = fresh((n, 6), torch.float64, float("nan")), fresh((n, 4), torch.float32, float("nan")), fresh((n, 6), torch.float64, float("nan"))
    blocked, blocked_all = fresh((n,), torch.int32, -7), fresh((n,), torch.int32, -7)
    seg, last, ends = fresh((m * n, 6), torch.float64, float("nan")), fresh((n, 6), torch.float64, float("nan")), fresh((n, 4), torch.int32, -1)
    torch.cuda.synchronize()
    r.permute_into(perm, n, d_tmax.data_ptr(), g_tmax.data_ptr(), 8)
    r.trace_into(srt, n, hits.data_ptr())
    r.occluded_into(srt, g_tmax.data_ptr(), n, blocked.data_ptr())
    r.occluded_into(srt, None, n, blocked_all.data_ptr())
    r.shade_into(srt, n, rgba.data_ptr(), rec.data_ptr())
    r.paths_into(srt, n, m, seg.data_ptr(), last.data_ptr(), ends.data_ptr())
    torch.cuda.synchronize()
    assert g_tmax.cpu().numpy().tobytes() == t_max[s.perm].tobytes()
    return {"rt_trace_rays": hits_of(back(hits, 48)), "rt_occluded_rays, t_max": back(blocked, 4).cpu().numpy(), "rt_occluded_rays, NULL": back(blocked_all, 4).cpu().numpy(),
            "rt_shade_rays": back(rgba, 16).cpu().numpy(), "rt_shade_rays, hits": hits_of(back(rec, 48)),
            "rt_trace_paths, segments": hits_of(back(seg, 48, planes=m)).reshape(m, n), "rt_trace_paths, last": hits_of(back(last, 48)), "rt_trace_paths, ends": ends_of(back(ends, 16))}


def result_contexts(pkg):
    f = four(pkg)
    out = [("beyond", "four flags", f), ("beyond", "four flags, FAST", f | pkg.RT_FLAG_FAST), ("beyond", "without RT_FLAG_STREAM_CULL_RAYS", f & ~pkg.RT_FLAG_STREAM_CULL_RAYS)]
    out += [("stats", what, flags) for _, what, flags in out[:3]] + [("stats", "plain staged", 0)]
    return out


@pytest.mark.parametrize("case", range(7))
def test_results_are_unchanged(pkg, case):
    """Sort, query on the sorted rays, scatter == the direct call on the caller's order, bit for bit: the aimed rays (odd kinds among them)
    and t_max of the 2 562-sphere field and of the statistics scene, shuffled."""
    scene, what, flags = result_contexts(pkg)[case]
    c = B.beyond(B.BEYOND[0]) if scene == "beyond" else stats_case()
    rays, t_max = shuffled_case(c, 90 + case)
    assert not SL.class0(rays).all() and np.isnan(t_max).any()      # (odd kinds are there)
    r = pkg.Renderer(c.sc, device=0, flags=flags)
    try:
        assert r.stream_cull_rays is (what.startswith("four")) and (flags != 0 or not r.streamed_queries)
        direct = ray_outputs(r, rays, t_max)
        assert (direct["rt_trace_rays"]["object"] >= 0).sum() > len(rays) // 2
        assert_same_outputs(sorted_outputs(r, rays, t_max), direct, (scene, what))
    finally:
        r.cleanup_update()


# ---- 5. the keywords ----------------------------------------------------------------------------------------------------------------------
def test_the_sort_keywords_return_the_same_bytes(pkg):
    e = RL.expectation("shuffled")
    rays = e["rays"]
    o, d = rays["o"], rays["d"]
    t_max = np.where(np.arange(len(rays)) % 3 == 0, 20.0, 1e6)
    r = pkg.Renderer(BL.bounce_scene(pkg), device=0, flags=four(pkg))
    try:
        a, b = r.trace(o, d), r.trace(o, d, sort=True)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() and (a["object"] >= 0).any()
        for tm in (None, t_max):
            (a, ms_a), (b, ms_b) = r.occluded(o, d, tm), r.occluded(o, d, tm, sort=True)
            assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and ms_a >= 0.0 and ms_b >= 0.0
        assert r.occluded(o, d, sort=True, timed=False)[1] is None
        a, b = r.shade(o, d), r.shade(o, d, sort=True)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        for m in (None, 0, 1):
            for a, b in zip(r.paths(o, d, m), r.paths(o, d, m, sort=True)):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), m
        srt, perm, keys = r.sort_rays(o, d)
        assert srt.dtype == pkg.RAY_DTYPE and perm.dtype == keys.dtype == np.uint32
        assert np.array_equal(perm, SL.host_perm(rays)) and srt.tobytes() == rays[perm].tobytes() and np.array_equal(keys, SL.keys(rays)[perm])
    finally:
        r.cleanup_update()


# ---- 6. work words ------------------------------------------------------------------------------------------------------------------------
def test_work_words(pkg, monkeypatch):
    """The statistics scene's 64 x 48 primary rays, shuffled: one four-flag context traces them as they are (words s), a fresh one after
    rt_sort_rays (words w).  [0] == D = 240 exactly; the pairs left unstaged are at least the CPU's L for the sorted rays (210 by the
    distance rule; 26 for the shuffled rays, 184 for row order); fewer chunks staged than for the shuffled rays; every wave has a lane that
    can be culled for."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    e, shuffled = SL.sorted_expectation("shuffled"), RL.expectation("shuffled")
    rays = shuffled["rays"]
    sc = BL.bounce_scene(pkg)
    a, b = pkg.Renderer(sc, device=0, flags=four(pkg)), pkg.Renderer(sc, device=0, flags=four(pkg))
    try:
        assert a.stream_cull_rays and b.stream_cull_rays
        direct = trace_dev(a, rays)
        s = a.stream_cull_rays_stats()
        srt = Sorted(b, rays)
        assert np.array_equal(srt.perm, SL.host_perm(rays)) and srt.sorted.tobytes() == e["rays"].tobytes()
        got = trace_dev(b, srt.sorted)
        w = b.stream_cull_rays_stats()
        print("work words, shuffled rays", s, "sorted", w, "CPU proxy: L sorted", e["L"], "L shuffled", shuffled["L"])
        assert w[0] == 240 == e["D"], w
        assert w[0] - w[1] >= e["L"], (w, e["L"])
        assert w[1] < s[1], (w, s)
        assert w[4] == 0, w
        assert rays_ref.same_records(got, direct[srt.perm])
    finally:
        a.cleanup_update()
        b.cleanup_update()


# ---- 7. graph -----------------------------------------------------------------------------------------------------------------------------
def test_one_graph_of_sort_trace_and_scatter(pkg):
    """rt_sort_rays, rt_trace_rays and rt_permute (scatter), all with ms == NULL, as a linear chain on one stream: replayed for the rays it
    was captured with and again after the ray buffer was overwritten with another set of the same count, the graph gives what the direct
    call on each set gives."""
    import torch
    first = RL.expectation("shuffled")["rays"]
    second = np.ascontiguousarray(RL.expectation("block")["rays"][::-1])
    n = len(first)
    assert len(second) == n and not np.array_equal(SL.host_perm(first), SL.host_perm(second))
    r = pkg.Renderer(BL.bounce_scene(pkg), device=0, flags=four(pkg))
    s = torch.cuda.Stream()
    try:
        want = [trace_dev(r, rays) for rays in (first, second)]
        assert want[0].tobytes() != want[1].tobytes()
        need = r.sort_work_bytes(n)
        with torch.cuda.stream(s):
            d_rays = to_device(first)
            srt = torch.zeros((n, 6), dtype=torch.float64, device="cuda:0")
            perm = torch.zeros((n,), dtype=torch.int32, device="cuda:0")
            work = torch.zeros((need,), dtype=torch.uint8, device="cuda:0")
            hits = torch.zeros((n, 6), dtype=torch.float64, device="cuda:0")
            out = torch.zeros((n, 6), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()

        def chain():
            r.sort_rays_into(d_rays.data_ptr(), n, srt.data_ptr(), perm.data_ptr(), None, work.data_ptr(), need, stream=s.cuda_stream, timed=False)
            r.trace_into(srt.data_ptr(), n, hits.data_ptr(), stream=s.cuda_stream, timed=False)
            r.permute_into(perm.data_ptr(), n, hits.data_ptr(), out.data_ptr(), 48, scatter=True, stream=s.cuda_stream, timed=False)
        chain()      # (uncaptured once, on the same stream)
        s.synchronize()
        assert hits_of(out).tobytes() == want[0].tobytes()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            chain()
        for k, rays in enumerate((first, second, first)):
            with torch.cuda.stream(s):
                d_rays.copy_(torch.from_numpy(np.ascontiguousarray(rays).view(np.float64).reshape(-1, 6)))
                for t in (srt, hits, out, work):
                    t.view(torch.uint8).fill_(0xAB)
                perm.fill_(-1)
                g.replay()
            s.synchronize()
            assert hits_of(out).tobytes() == want[k % 2].tobytes(), ("replay", k)
            assert np.array_equal(perm.cpu().numpy().view(np.uint32), SL.host_perm(rays)), ("replay", k)
        del g
    finally:
        torch.cuda.synchronize()
        r.cleanup_update()


# ---- 8. past one trip of the bounded grids -------------------------------------------------------------------------------------------------
# Every kernel of csrc/rt_sort_rays.hip runs at most G workgroups and loops over the rest; G = 4 per CU, as tests/test_rays_gpu.py computes
# it.  The sizes below are derived from G, never from a CU count.
def cap():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def big_sizes():
    """T G + T + 1: G + 2 tiles, so workgroups 0 and 1 of histogram_kernel and scatter_kernel make two trips of their tile loop and the
    others one; 8 G + 9 workgroups of 256 rays, so the per-ray kernels (box, keys, gather) make nine and eight trips; two scan levels.
    2 T G + T + 1: 2 G + 2 tiles, three and two trips."""
    return [T * cap() + T + 1, 2 * T * cap() + T + 1]


def tiled_on_the_device(base, n):
    """[n, 6] float64 on the device: the rays `base` tiled.  Every copy is the same rays, so the box is base's and the keys are
    SL.keys(base) tiled: P keys are uploaded and tiled on the device as well (int64, as torch sorts them)."""
    import torch
    assert n >= len(base)
    reps = -(-n // len(base))
    d_base = to_device(base)
    d_keys = torch.from_numpy(SL.keys(base).astype(np.int64)).to("cuda:0")
    return d_base.repeat(reps, 1)[:n].contiguous(), d_keys.repeat(reps)[:n].contiguous()


def check_big_sort(r, base, n, want_sorted, host_argsort=False):
    """rt_sort_rays of n tiled rays against torch's own stable device sort of the tiled host keys; returns the wall seconds of the call."""
    import time
    import torch
    d_rays, d_keys = tiled_on_the_device(base, n)
    want_keys, want_perm = torch.sort(d_keys, stable=True)
    if host_argsort:      # the torch reference itself, once, against numpy's stable argsort
        k = np.tile(SL.keys(base), -(-n // len(base)))[:n]
        assert np.array_equal(want_perm.cpu().numpy(), np.argsort(k, kind="stable")), "torch.sort(stable=True) is numpy's stable argsort"
    b_sorted, b_perm, b_keys = (guarded(48 * n) if want_sorted else None), guarded(4 * n), guarded(4 * n)
    need = r.sort_work_bytes(n)
    b_work = guarded(need)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r.sort_rays_into(d_rays.data_ptr(), n, b_sorted.data_ptr() if want_sorted else None, b_perm.data_ptr(), b_keys.data_ptr(), b_work.data_ptr(), need, timed=False)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    perm = b_perm[:4 * n].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    keys = b_keys[:4 * n].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(keys, want_keys), (n, "keys", int((keys != want_keys).sum()))
    assert torch.equal(perm, want_perm), (n, "perm", int((perm != want_perm).sum()))
    assert guard_untouched(b_perm, 4 * n) and guard_untouched(b_keys, 4 * n) and guard_untouched(b_work, need), (n, "guard bands")
    if want_sorted:
        at = torch.arange(0, n, max(1, n // (1 << 16)), device="cuda:0")[:1 << 16]
        got = b_sorted[:48 * n].view(torch.int64).reshape(n, 6)[at]
        assert torch.equal(got, d_rays.view(torch.int64)[want_perm[at]]), (n, "sorted == rays[perm] on a strided sample")
        assert guard_untouched(b_sorted, 48 * n), (n, "guard band of sorted")
    return seconds


@pytest.mark.parametrize("which", [0, 1])
def test_sizes_past_the_cap(any_ctx, which):
    """big_sizes(): the tile loop of histogram_kernel and scatter_kernel iterates twice (which = 0) and three times (1) in the first
    workgroups and once less in the rest, its trailing barrier and the re-zeroed LDS counts are needed; the per-ray loops make more than
    eight trips.  The base is the "quarter odd" set (2 T + 1 rays, a quarter of them class 1), so every key recurs in every copy and a
    stable order has to hold across tiles and trips.  Reference: torch's stable device sort of the tiled host keys, at the first size held
    to numpy's stable argsort."""
    n = big_sizes()[which]
    G = cap()
    tiles = -(-n // T)
    assert n % 2 == 1 and tiles == (which + 1) * G + 2 and -(-tiles // G) == which + 2 and tiles // G == which + 1
    assert W < 256 * tiles <= W * W      # the table of 256 x tiles entries takes two scan levels
    base = SL.adversarial("quarter odd")
    assert (T * G) % len(base) != 0      # (a copy does not start where a trip does)
    seconds = check_big_sort(any_ctx, base, n, want_sorted=True, host_argsort=which == 0)
    print(f"rt_sort_rays of {n} rays ({tiles} tiles, cap {G}): {seconds:.3f} s")


def test_three_scan_levels(any_ctx):
    """16 384 T + 1 rays = 16 385 tiles: the digit-major table has 16 385 x 256 entries = 2 049 scan chunks, which is more than one chunk of
    sums -- the first size at which the levelled scan has three levels (reduce_chunks_kernel twice, scan_chunks_kernel three times per pass,
    the middle level with a partial second chunk).  The tile loop makes ceil(16 385 / G) trips and the scan's chunk loop ceil(2 049 / G).
    sorted = NULL (the rays alone are 1.6 GB); the host uploads the 2 T + 1 base rays and keys, everything else is formed on the device."""
    n = 16384 * T + 1
    assert -(-n // T) == 16385
    chunk = W      # RS_SCAN_CHUNK: the entries of the digit-major table one scan workgroup covers in one step
    level0 = 16385 * 256
    level1 = -(-level0 // chunk)
    assert level1 == 2049 > chunk and -(-level1 // chunk) == 2      # three levels: 4 194 560 -> 2 049 -> 2
    seconds = check_big_sort(any_ctx, SL.adversarial("quarter odd"), n, want_sorted=False)
    print(f"rt_sort_rays of {n} rays (16385 tiles, three scan levels, cap {cap()}): {seconds:.3f} s")


@pytest.mark.parametrize("elem", (4, 8, 16, 48))
def test_permute_past_the_cap(any_ctx, elem):
    """n = 2 x 256 G + 257 records: permute_kernel's grid is capped at G workgroups of 256 lanes and one lane moves one 4-byte or 16-byte
    element, so its loop makes three trips for 4-byte records (2 G + 2 workgroups of work: workgroups 0 and 1 three, the others two), about
    2 per x that many for records of `per` elements, the last one partial.  Gather == numpy's fancy indexing, gather then scatter == the
    identity, guard bands untouched, planes 1 and 3; 48-byte records also on pointers that only allow words (per = 12, > 24 trips)."""
    import torch
    r, G = any_ctx, cap()
    n = 2 * 256 * G + 257
    assert -(-n // 256) == 2 * G + 2 and n % 64 != 0
    rng = np.random.default_rng(700 + elem)
    perm = rng.permutation(n).astype(np.uint32)
    d_perm = torch.from_numpy(perm.view(np.int32)).to("cuda:0")
    pool = rng.integers(0, 256, 3 * n * elem + 4, dtype=np.uint8)
    for planes in (1, 3):
        src = pool[:planes * n * elem].reshape(planes, n, elem)
        nbytes = src.size
        d_src = torch.from_numpy(src).to("cuda:0")
        mid, back = guarded(nbytes), guarded(nbytes)
        torch.cuda.synchronize()
        r.permute_into(d_perm.data_ptr(), n, d_src.data_ptr(), mid.data_ptr(), elem, planes=planes)
        r.permute_into(d_perm.data_ptr(), n, mid.data_ptr(), back.data_ptr(), elem, planes=planes, scatter=True, timed=False)
        torch.cuda.synchronize()
        assert np.array_equal(mid[:nbytes].cpu().numpy().reshape(planes, n, elem), src[:, perm]), (elem, planes, "gather is numpy's fancy indexing")
        assert torch.equal(back[:nbytes], d_src.reshape(-1)), (elem, planes, "gather then scatter")
        assert guard_untouched(mid, nbytes) and guard_untouched(back, nbytes), (elem, planes)
    if elem == 48:      # the uint32_t path with per = 12
        src = pool[4:4 + 48 * n].reshape(n, 48)
        d_src, out = guarded(48 * n + 4), guarded(48 * n + 4)
        d_src[4:4 + 48 * n] = torch.from_numpy(src.reshape(-1)).to("cuda:0")
        torch.cuda.synchronize()
        r.permute_into(d_perm.data_ptr(), n, d_src.data_ptr() + 4, out.data_ptr() + 4, 48)
        torch.cuda.synchronize()
        assert np.array_equal(out[4:4 + 48 * n].cpu().numpy().reshape(n, 48), src[perm]) and guard_untouched(out, 48 * n + 4) and (out[:4] == FILL).all().item()


def test_the_sort_keywords_past_the_cap(pkg):
    """r.trace(o, d, sort=True) and r.shade(o, d, sort=True) on the four-flag statistics scene for 2 x 256 G + 613 shuffled tiled rays:
    rt_sort_rays (per-ray loops: workgroups 0 .. 2 three trips, the others two; 2 G / 8 + 1 tiles), the culled kernel (three and two
    trips, the last workgroup with a full wave, a wave of 37 rays and two waves without a ray) and the scatter of rt_permute (48-byte and
    16-byte records), in one chain: the bytes are the unsorted call's."""
    G = cap()
    n = 2 * 256 * G + 613
    assert n > 2 * 256 * G + 256 and n % 64 == 37
    rays = SL.tiled_shuffled(n, 43)
    o, d = rays["o"], rays["d"]
    r = pkg.Renderer(BL.bounce_scene(pkg), device=0, flags=four(pkg))
    try:
        assert r.stream_cull_rays
        a, b = r.trace(o, d), r.trace(o, d, sort=True)
        assert a.dtype == b.dtype and a.shape == b.shape == (n,) and a.tobytes() == b.tobytes() and (a["object"] >= 0).any() and (a["object"] < 0).any()
        a, b = r.shade(o, d), r.shade(o, d, sort=True)
        assert a.dtype == b.dtype and a.shape == b.shape == (n, 4) and a.tobytes() == b.tobytes()
    finally:
        r.cleanup_update()


# ---- 9. the key where one rounding decides the cell -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 4])
def test_edge_values(any_ctx, seed):
    """SL.edge_rays: origins one representable value around every sixteenth of a box with an axis from 0.0, one 2e-300 wide and one of
    sub-normal width, directions one value around the cell boundaries of the octahedral map, the clamp, the fold at n.z == +-0.0.  The
    device's key (FP64 division, floor, no contraction on gfx950) is the header's compiled for the host, bit for bit."""
    rays = SL.edge_rays(2 * T + 1, seed)
    assert SL.class0(rays).all()
    check_sort(any_ctx, rays, ("edge values", seed))
