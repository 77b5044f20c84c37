"""The streamed and the culled ray kernels past two trips of their bounded grid (csrc/rt_ray_kernels.hpp; DESIGN.md section 8, "Past one
grid trip").  Every kernel for caller-supplied rays runs at most G = 4 workgroups per CU and loops over the rest with a workgroup-uniform
trip count; a trip is 256 G rays.  The staged kernels leave the first trip in tests/test_rays_gpu.py, test_shade_gpu.py and
test_paths_gpu.py; here the query objects that live across the loop's iterations do -- SqQuery's wave-private LDS slice, re-staged from one
trip to the next (also behind an occlusion sweep that returned early and left it half used), ScRayQuery's work words, the HAS_GQ and
HAS_CUBIC instantiations with their index lists, and the (uint64_t) k * n + i addressing of the path planes.

Ray sets: the P aimed rays of a scene (odd kinds among them, so plain and table lanes share waves), tiled and cut at n = 2 x 256 G + 613:
2 G + 3 workgroups of work, so workgroups 0, 1 and 2 make three trips and every other one two; the last workgroup of the last trip holds
a full wave, a wave of 37 rays and two waves without a ray.  256 G is no multiple of P (asserted), so a later trip's rays are not the first
trip's: a kernel that reads trip 0's ray again does not pass.  G is computed as the three staged tests compute it; nothing here assumes a
CU count.

References: strict contexts of degree <= 2 are held to the CPU composers' answers for the P rays, tiled, with the comparison functions
of the small tests; RT_FLAG_FAST contexts and the degree-3 field to the same context's call on the P rays alone, tiled, bit for bit
(tests/test_fast_truth_gpu.py and tests/test_cubic_chunks_gpu.py hold those to exact arithmetic and to the oracle).  Every output buffer of a
big call has a guard band behind it and starts as 0xA5 bytes.  "Four flags" is RT_FLAG_STREAM | RT_FLAG_STREAM_QUERIES |
RT_FLAG_STREAM_CULL | RT_FLAG_STREAM_CULL_RAYS; "by size" is the same without RT_FLAG_STREAM."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import bounce_cull_lab as BL  # noqa: E402
import cubic_field_scenes as F  # noqa: E402
import paths_ref  # noqa: E402
import query_table_scenes as Q  # noqa: E402
import raw_desc_scenes as R  # noqa: E402
import ray_cull_lab as RL  # noqa: E402
import rays_ref  # noqa: E402
import stream_query_scenes as B  # noqa: E402
import test_paths_gpu as P  # noqa: E402
import test_rays_gpu as T  # noqa: E402
import test_shade_gpu as H  # noqa: E402
from test_query_tables_gpu import Composed  # noqa: E402
from test_rays_gpu import to_device  # noqa: E402
from test_sort_rays_gpu import guard_untouched, guarded  # noqa: E402
from test_stream_queries_gpu import assert_same_outputs  # noqa: E402

pytestmark = pytest.mark.gpu


def cap():
    """G: the most workgroups a ray kernel is launched with (rays_max_grid), as tests/test_rays_gpu.py::test_arbitrary_rays computes it."""
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def four(pkg):
    return pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_QUERIES | pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_RAYS


def flags_of(pkg, scene, culled, fast):
    f = four(pkg) if scene == CUBIC else four(pkg) & ~pkg.RT_FLAG_STREAM      # (the beyond scenes are streamed by their size)
    return (f if culled else f & ~pkg.RT_FLAG_STREAM_CULL_RAYS) | (pkg.RT_FLAG_FAST if fast else 0)


# ---- the entry points on guarded buffers -----------------------------------------------------------------------------------------------
def outputs(r, rays, t_max):
    """Every output of rt_trace_rays, rt_occluded_rays (t_max and NULL), rt_shade_rays with hit records and rt_trace_paths with
    max_segments = 1 and = every segment a path can have, out_last both times, by name.  Each buffer starts as 0xA5 bytes with a guard
    band behind it, which is asserted untouched."""
    import torch
    n, m = len(rays), r._max_segments(None)
    d_rays, d_tmax = to_device(rays), torch.from_numpy(np.ascontiguousarray(t_max)).to("cuda:0")
    sizes = {"rt_trace_rays": 48 * n, "rt_occluded_rays, t_max": 4 * n, "rt_occluded_rays, NULL": 4 * n, "rt_shade_rays": 16 * n, "rt_shade_rays, hits": 48 * n}
    for k in sorted({1, m}):
        sizes.update({f"rt_trace_paths({k}), segments": 48 * k * n, f"rt_trace_paths({k}), last": 48 * n, f"rt_trace_paths({k}), ends": 16 * n})
    b = {key: guarded(size) for key, size in sizes.items()}
    p = {key: buf.data_ptr() for key, buf in b.items()}
    torch.cuda.synchronize()
    r.trace_into(d_rays.data_ptr(), n, p["rt_trace_rays"])
    r.occluded_into(d_rays.data_ptr(), d_tmax.data_ptr(), n, p["rt_occluded_rays, t_max"])
    r.occluded_into(d_rays.data_ptr(), None, n, p["rt_occluded_rays, NULL"])
    r.shade_into(d_rays.data_ptr(), n, p["rt_shade_rays"], p["rt_shade_rays, hits"])
    for k in sorted({1, m}):
        r.paths_into(d_rays.data_ptr(), n, k, p[f"rt_trace_paths({k}), segments"], p[f"rt_trace_paths({k}), last"], p[f"rt_trace_paths({k}), ends"])
    torch.cuda.synchronize()
    out = {}
    for key, size in sizes.items():
        assert guard_untouched(b[key], size), (key, "guard band")
        raw = b[key][:size].cpu().numpy()
        if key.startswith("rt_occluded"):
            out[key] = raw.view(np.int32)
        elif key == "rt_shade_rays":
            out[key] = raw.view(np.float32).reshape(n, 4)
        elif key.endswith("ends"):
            out[key] = raw.view(paths_ref.END_DTYPE)
        elif key.endswith("segments"):
            out[key] = raw.view(rays_ref.HIT_DTYPE).reshape(-1, n)
        else:
            out[key] = raw.view(rays_ref.HIT_DTYPE)
    return out


def tiled(out, reps, cut):
    """The outputs for some rays as the outputs for those rays tiled `reps` times and cut at `cut`."""
    def one(v):
        if v.ndim == 2 and v.dtype == rays_ref.HIT_DTYPE:      # planes [m, n]
            return np.ascontiguousarray(np.tile(v, (1, reps))[:, :cut])
        return np.ascontiguousarray(np.tile(v, (reps, 1))[:cut] if v.ndim == 2 else np.tile(v, reps)[:cut])
    return {key: one(v) for key, v in out.items()}


def composer_outputs(want, m):
    """A Composed as the dict `outputs` returns (max_segments only limits what is stored: the planes of 1 are the first plane of m)."""
    seg, last, ends = want.paths
    assert len(seg) == m
    out = {"rt_trace_rays": want.hits, "rt_occluded_rays, t_max": want.blocked, "rt_occluded_rays, NULL": want.blocked_all, "rt_shade_rays": want.colours,
           "rt_shade_rays, hits": want.first}
    for k in sorted({1, m}):
        out.update({f"rt_trace_paths({k}), segments": seg[:k], f"rt_trace_paths({k}), last": last, f"rt_trace_paths({k}), ends": ends})
    return out


def assert_as_composers(got, want, m, what):
    """got against the composers' dict with the comparison functions of the small tests (check_ray_queries of tests/test_query_tables_gpu.py)."""
    assert got.keys() == want.keys()
    T.assert_records(got["rt_trace_rays"], want["rt_trace_rays"], (what, "rt_trace_rays"))
    for key in ("rt_occluded_rays, t_max", "rt_occluded_rays, NULL"):
        assert np.array_equal(got[key], want[key]), (what, key, int((got[key] != want[key]).sum()))
    H.assert_colours(got["rt_shade_rays"], want["rt_shade_rays"], (what, "rt_shade_rays"))
    H.assert_records_as_composer(got["rt_shade_rays, hits"], want["rt_shade_rays, hits"], (what, "rt_shade_rays, hits"))
    for k in sorted({1, m}):
        names = [f"rt_trace_paths({k}), {part}" for part in ("segments", "last", "ends")]
        P.assert_composer(tuple(got[x] for x in names), tuple(want[x] for x in names), (what, f"rt_trace_paths({k})"))


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------------
CUBIC = "65 spheres"      # tests/tools/cubic_field_scenes.py: 65 bent ellipsoids and the mirrored 65-sphere field


@functools.lru_cache(maxsize=None)
def scene(name):
    """(product scene, rays, t_max, the composers' dict or None, max segments), formed once per process and left unchanged."""
    import __graft_entry__ as graft
    pkg = graft.load_package()
    if name == CUBIC:
        osc = F.scene(CUBIC)
        rays = np.concatenate([rays_ref.primary_rays(osc), F.aimed_rays(osc)])
        rng = np.random.default_rng(Q.TMAX_SEED)
        t_max = np.where(rng.random(len(rays)) < 0.5, Q.K_MAX_T, rng.uniform(5.0, 60.0, len(rays)))
        return R.desc(pkg, osc), rays, t_max, None, osc.max_reflections + 1
    c = B.beyond(name)
    m = c.osc.max_reflections + 1
    return c.sc, c.rays, c.t_max, composer_outputs(Composed(c.osc, c.rays, c.t_max), m), m


def cut_of(G):
    return 2 * 256 * G + 613


CASES = [(name, culled, fast) for name in B.BEYOND[:2] for culled in (False, True) for fast in (False, True)]
CASES += [(name, culled, False) for name in (B.BEYOND[2], CUBIC) for culled in (False, True)]


# ---- 1. every entry point, every context -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,culled,fast", CASES, ids=lambda v: ("on" if v else "off") if isinstance(v, bool) else v.replace(" ", "_"))
def test_three_trips(pkg, name, culled, fast):
    """n = 2 x 256 G + 613 tiled rays through rk_ray_query (closest hit; occlusion with t_max and with NULL), rk_shade_rays and
    rk_path_query / path_query_stream_kernel (max_segments 1 and all) of a streamed (SqQuery) or culled (ScRayQuery) context: workgroups
    0 .. 2 make three trips of the grid-stride loop, the other G - 3 two.  The 2 562-sphere field (depth 0), the mirror field (depth 2:
    the bounce loops past k = 0 on later trips), the mixed field (<HAS_GQ = 1>) and the 65-object degree-3 field with 65 spheres
    (<HAS_CUBIC = 1>, sq_stage_indices on later trips)."""
    sc, rays, t_max, composed, m = scene(name)
    G, n_small = cap(), len(rays)
    cut = cut_of(G)
    reps = -(-cut // n_small)
    assert cut > 2 * 256 * G + 256 and cut % 64 == 37 and -(-cut // 256) == 2 * G + 3      # three trips for workgroups 0 .. 2, two for the rest
    assert (256 * G) % n_small != 0      # a trip does not start where a copy does
    big, big_t = np.tile(rays, reps)[:cut], np.tile(t_max, reps)[:cut]
    r = pkg.Renderer(sc, device=0, flags=flags_of(pkg, name, culled, fast))
    try:
        assert r.streamed and r.streamed_queries and r.stream_cull_rays is culled and r._max_segments(None) == m
        got = outputs(r, big, big_t)
        if composed is not None and not fast:
            assert_as_composers(got, tiled(composed, reps, cut), m, (name, culled, "against the composers, tiled"))
        else:
            small = outputs(r, rays, t_max)
            assert (small["rt_trace_rays"]["object"] >= 0).sum() > n_small // 4
            assert_same_outputs(got, tiled(small, reps, cut), (name, culled, fast, "against the call on one copy, tiled"))
    finally:
        r.cleanup_update()
    if m > 1:      # some path of a later trip has a second segment, and ends past it
        later = got[f"rt_trace_paths({m}), segments"][1, 2 * 256 * G:]
        assert (later["object"] >= 0).any() and (got[f"rt_trace_paths({m}), ends"]["segments"][2 * 256 * G:] > 1).any()


# ---- 2. the work words across trips ----------------------------------------------------------------------------------------------------------
def words_of(r, call):
    before = r.stream_cull_rays_stats()
    call()
    return [b - a for a, b in zip(before, r.stream_cull_rays_stats())]


def test_work_words_of_tiled_rays(pkg, monkeypatch):
    """MI355RT_STREAM_CULL_STATS=1, the four-flag context of the statistics scene, its 3 072 primary rays in row order (48 whole waves),
    tiled to reps copies with reps x 3 072 > 2 x 256 G: the culled kernels make three trips, and the eight work words ScRayQuery carries
    across them are, exactly, reps times the words of a call on one copy (rt_trace_rays: [0] == reps x 240, the CPU's D), and additive
    at a cut a = 256 G + 192 (a multiple of 64, not of 256, past one trip): words(big[:a]) + words(big[a:]) == words(big) -- a wave that
    holds no ray counts nothing.  The same for rt_occluded_rays with NULL and for rt_shade_rays, whose words are deterministic per wave."""
    import torch
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    e = RL.expectation("row")
    base = e["rays"]
    G = cap()
    reps = (2 * 256 * G) // len(base) + 1
    n, a = reps * len(base), 256 * G + 192
    assert len(base) == 3072 and e["D"] == 240 and n > 2 * 256 * G and (256 * G) % len(base) != 0 and a % 64 == 0 and a % 256 != 0 and 256 * G < a < n
    r = pkg.Renderer(BL.bounce_scene(pkg), device=0, flags=four(pkg))
    try:
        assert r.stream_cull_rays and r.stream_cull_rays_stats() == [0] * 8
        d_rays = to_device(np.tile(base, reps))
        hits, flags, rgba = guarded(48 * n), guarded(4 * n), guarded(16 * n)
        torch.cuda.synchronize()
        at = d_rays.data_ptr()
        calls = {"rt_trace_rays": lambda first, count: r.trace_into(at + 48 * first, count, hits.data_ptr()),
                 "rt_occluded_rays": lambda first, count: r.occluded_into(at + 48 * first, None, count, flags.data_ptr()),
                 "rt_shade_rays": lambda first, count: r.shade_into(at + 48 * first, count, rgba.data_ptr())}
        for which, call in calls.items():
            one = words_of(r, lambda: call(0, len(base)))
            whole = words_of(r, lambda: call(0, n))
            head, tail = words_of(r, lambda: call(0, a)), words_of(r, lambda: call(a, n - a))
            print(f"work words of {which}: one copy {one}, {reps} copies ({n} rays, cap {G}) {whole}, first {a} {head}, the rest {tail}")
            assert whole == [reps * w for w in one], (which, whole, one)
            assert [x + y for x, y in zip(head, tail)] == whole, (which, head, tail, whole)
            assert one[0] > 0 and one[1] < one[0] and one[4] == 0, (which, one)
            if which == "rt_trace_rays":
                assert one[0] == e["D"] and whole[0] == reps * 240, (one, whole)
        assert guard_untouched(hits, 48 * n) and guard_untouched(flags, 4 * n) and guard_untouched(rgba, 16 * n)
    finally:
        r.cleanup_update()
