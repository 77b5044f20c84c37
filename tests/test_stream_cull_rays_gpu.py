"""Culled ray queries on the GPU (RT_FLAG_STREAM_CULL_RAYS; csrc/rt_stream_cull_rays.hip): rt_trace_rays,
rt_occluded_rays, rt_shade_rays, rt_trace_paths, rt_pick_paths and the _host forms with the unit-sphere chunks culled per caller-supplied
ray.  The outputs are the streamed queries' by definition: every strict output of degree <= 2 here is compared bit for bit with the CPU
composers (the checks of tests/test_query_tables_gpu.py, imported), with the same context without the new flag and, where a staged kernel
takes the scene, with the unflagged staged context.  "Four flags" is RT_FLAG_STREAM | RT_FLAG_STREAM_QUERIES | RT_FLAG_STREAM_CULL |
RT_FLAG_STREAM_CULL_RAYS.  The host-side conditions (the predicate against the oracle for a caller's rays, the statistics scene's
L >= D / 2) are in tests/test_stream_cull_rays_host.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import bounce_cull_lab as BL  # noqa: E402
import query_table_scenes as Q  # noqa: E402
import ray_cull_lab as RL  # noqa: E402
import rays_ref  # noqa: E402
import stream_query_scenes as B  # noqa: E402
import stream_scenes as S  # noqa: E402
import test_paths_gpu as P  # noqa: E402
import test_shade_gpu as H  # noqa: E402
from test_query_tables_gpu import Composed, check_ray_queries  # noqa: E402
from test_rays_gpu import occluded_dev, to_device, trace_dev  # noqa: E402
from test_stream_cull_bounce_gpu import cubic_mirror_and_field  # noqa: E402
from test_stream_queries_gpu import all_pixels, assert_same_outputs, ray_outputs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def the_feature(pkg):
    assert pkg.RT_FLAG_STREAM_CULL_RAYS == 2097152


def four(pkg):
    return pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_QUERIES | pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_RAYS


def by_size(pkg):
    """The flags of a scene that is streamed by its size, without RT_FLAG_STREAM."""
    return four(pkg) & ~pkg.RT_FLAG_STREAM


def renderer(pkg, sc, flags, expect=True):
    r = pkg.Renderer(sc, device=0, flags=flags)
    assert r.stream_cull_rays is expect, (r.stream_cull_rays, r.stream_cull, r.streamed_queries, r.streamed)
    return r


def check_case(pkg, sc, osc, c, what, flags=None, staged=True):
    """The flagged context against the composers, against the same context without the new flag and (staged) against the unflagged staged
    context: every output of the four entry points."""
    flags = four(pkg) if flags is None else flags
    r, twin = renderer(pkg, sc, flags), renderer(pkg, sc, flags & ~pkg.RT_FLAG_STREAM_CULL_RAYS, False)
    plain = pkg.Renderer(sc, device=0) if staged else None
    try:
        assert twin.streamed_queries and twin.stream_cull and (plain is None or not plain.streamed_queries)
        check_ray_queries(r, c, Composed(osc, c.rays, c.t_max), what)
        got = ray_outputs(r, c.rays, c.t_max)
        assert_same_outputs(got, ray_outputs(twin, c.rays, c.t_max), (what, "without the flag"))
        if plain is not None:
            assert_same_outputs(got, ray_outputs(plain, c.rays, c.t_max), (what, "staged"))
    finally:
        for x in (r, twin, plain):
            if x is not None:
                x.cleanup_update()


# ---- 1. chunk boundaries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 128, 129, 193])
def test_chunk_boundaries(pkg, n):
    """65: the second chunk holds one entry; 128: a full last chunk (the field of tests/tools/stream_scenes.py); 129 / 193: one entry behind
    two and three full chunks.  The aimed rays (one per sphere, odd kinds among them) at depths 0, 1 and 4."""
    if n == 128:
        sc = S.field(pkg, 128, S.FIELD_SEED, mirrors=True, depth=1)
        c = Q.Case(sc, S.oracle_of(pkg, sc), True)
    else:
        assert ("sphere", n) in Q.SMALL
        c = Q.small_case(pkg, ("sphere", n))
    for depth in Q.DEPTHS:
        check_case(pkg, c.sc.set_max_reflections(depth), c.at_depth(depth), c, (n, "depth", depth))


# ---- 2. more than 64 chunks ---------------------------------------------------------------------------------------------------------------
def test_more_than_64_chunks(pkg):
    """4 100 spheres, 65 chunks, mirrors at depth 2: beyond what a staged query kernel takes."""
    sc = S.field(pkg, 4100, 3, mirrors=True, depth=2)
    c = Q.Case(sc, S.oracle_of(pkg, sc), False)
    check_case(pkg, sc, c.osc, c, "4100 spheres", staged=False)


# ---- 3. beyond the staged limit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.BEYOND)
def test_beyond_the_staged_limit(pkg, name):
    """2 562 spheres, 2 625 spheres with mirrors at depth 2, and 1 050 spheres among 1 050 general quadrics and two planes: streamed by
    size, without RT_FLAG_STREAM."""
    c = B.beyond(name)
    check_case(pkg, c.sc, c.osc, c, name, flags=by_size(pkg), staged=False)


# ---- 4. ray counts ------------------------------------------------------------------------------------------------------------------------
def test_prefixes_of_the_rays(pkg):
    """1, 63, 64, 65 and 257 of the aimed rays of the 2 562-sphere field (plain and table lanes share waves; waves without a ray): each entry
    point returns the same prefix of the full run's result, which is the unflagged context's."""
    c = B.beyond(B.BEYOND[0])
    assert not np.isfinite(c.rays["d"]).all() and (np.abs(c.rays["d"]).max(axis=1) == 0).any()
    r, twin = renderer(pkg, c.sc, by_size(pkg)), renderer(pkg, c.sc, by_size(pkg) & ~pkg.RT_FLAG_STREAM_CULL_RAYS, False)
    try:
        full = ray_outputs(r, c.rays, c.t_max)
        assert_same_outputs(full, ray_outputs(twin, c.rays, c.t_max), "all rays")
        for n in B.FIELD_PREFIXES:
            got = ray_outputs(r, c.rays[:n], c.t_max[:n])
            want = {k: (v[:, :n] if k == "rt_trace_paths, segments" else v[:n]) for k, v in full.items()}
            assert_same_outputs(got, want, n)
    finally:
        r.cleanup_update()
        twin.cleanup_update()


# ---- 5. other classes ---------------------------------------------------------------------------------------------------------------------
def test_large_mixed_scene(pkg):
    """Spheres among ellipsoids and planes, mirrors at depth 2: the <HAS_GQ = 1> instantiations against the composers."""
    sc = S.mixed_large(pkg, 2000, S.MIXED_SEED, depth=2)
    c = Q.Case(sc, S.oracle_of(pkg, sc), False)
    check_case(pkg, sc, c.osc, c, "large mixed", flags=by_size(pkg) | pkg.RT_FLAG_STREAM, staged=False)


def primary_as_rays(r):
    """The context's own primary rays (rt_primary_rays) as a host array of RAY_DTYPE."""
    rays, _ = r.primary_rays()
    return np.ascontiguousarray(rays.cpu().numpy().reshape(-1, 6)).view(rays_ref.RAY_DTYPE).reshape(-1)


@pytest.mark.parametrize("with_quadric", [False, True], ids=["cubic", "cubic+quadric"])
@pytest.mark.parametrize("name", ["clebsch", "cayley"])
def test_cubic_mirrors_with_a_field(pkg, monkeypatch, name, with_quadric):
    """The HAS_CUBIC instantiations, <0, 1> and <1, 1>, strict and fast: a degree-3 mirror over the mirrored 65-sphere field, the frame's own
    primary rays as caller-supplied rays.  Degree 3 is held to the library's own outputs: the flagged context's equal those of the context
    without the new flag and of the unflagged staged context, the FAST ones their unflagged twins'; chunks are left unstaged."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    d = cubic_mirror_and_field(pkg, name, 48, 36, with_quadric)
    f = pkg
    for fast in (0, f.RT_FLAG_FAST):
        r, twin, plain = renderer(pkg, d, four(pkg) | fast), renderer(pkg, d, (four(pkg) & ~f.RT_FLAG_STREAM_CULL_RAYS) | fast, False), pkg.Renderer(d, device=0, flags=fast)
        try:
            rays = primary_as_rays(r)
            t_max = np.where(np.arange(len(rays)) % 3 == 0, 20.0, Q.K_MAX_T)
            got = ray_outputs(r, rays, t_max)
            assert (got["rt_trace_rays"]["object"] == 0).sum() > 50      # the degree-3 mirror (object 0) is seen
            assert_same_outputs(got, ray_outputs(twin, rays, t_max), (name, fast, "without the flag"))
            assert not plain.streamed_queries
            assert_same_outputs(got, ray_outputs(plain, rays, t_max), (name, fast, "staged"))
            w = r.stream_cull_rays_stats()
            print("work words", w)
            assert w[0] > 0 and w[1] < w[0] and 0 < w[3] < w[2]
        finally:
            for x in (r, twin, plain):
                x.cleanup_update()


# ---- 6. odd rays --------------------------------------------------------------------------------------------------------------------------
def uncullable_rays(n=64):
    """Rays nothing can be culled for, proven and unproven ones in turn: zero direction, |d|^2 <= 1e-7, a NaN origin, a component beyond 1e100."""
    rays = np.zeros(n, dtype=rays_ref.RAY_DTYPE)
    rays["o"] = np.array([0.0, 0.0, -2.0]) + np.arange(n)[:, None] * 1e-3
    for i in range(n):
        rays["d"][i] = [(0.0, 0.0, 0.0), (1e-4, 0.0, 2e-4), (0.0, 0.0, 1.0), (1e120, 0.0, 1.0)][i % 4]
        if i % 4 == 2:
            rays["o"][i, i % 3] = np.nan
    return rays


def test_a_wave_of_rays_nothing_can_be_culled_for(pkg, monkeypatch):
    """64 such rays are one wave and one query: it counts in word [4], stages every chunk (its proven lanes reach every bound) and asks about
    no (lane, chunk) pair; an ordinary 65th ray makes a second wave that does not count there.  The answers are the unflagged context's."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    c = Q.small_case(pkg, ("sphere", 193))
    odd = uncullable_rays()
    keep = set(c.keep)
    i = next(i for i, t in enumerate(c.targets) if t in keep)      # (an aimed ray that is never of an odd kind)
    more = np.concatenate([odd, c.rays[i:i + 1]])
    assert np.isfinite(more["d"][-1]).all() and (more["d"][-1] ** 2).sum() > 1e-7
    r, twin = renderer(pkg, c.sc, four(pkg)), renderer(pkg, c.sc, four(pkg) & ~pkg.RT_FLAG_STREAM_CULL_RAYS, False)
    try:
        nc = len(r.stream_bounds()) // 64
        assert nc == 4 and r.stream_cull_rays_stats() == [0] * 8
        got = trace_dev(r, odd)
        assert r.stream_cull_rays_stats() == [nc, nc, 0, 0, 1, 0, 0, 0]
        assert rays_ref.same_records(got, trace_dev(twin, odd))
        got = trace_dev(r, more)      # the same wave again, and a wave whose one lane stages exactly the chunks it reaches
        w = r.stream_cull_rays_stats()
        print("work words", w)
        assert w[0] == 3 * nc and w[4] == 2 and w[2] == nc and 0 < w[3] <= nc and w[1] == 2 * nc + w[3], w
        assert rays_ref.same_records(got, trace_dev(twin, more)) and got["object"][-1] >= 0
        assert_same_outputs(ray_outputs(r, more, None), ray_outputs(twin, more, None), "odd rays")
    finally:
        r.cleanup_update()
        twin.cleanup_update()


# ---- 7. t_max -----------------------------------------------------------------------------------------------------------------------------
def test_t_max_bounds_the_roots_not_the_verdicts(pkg):
    """The aimed t_max -- 0.9 ... 1.1 of a ray's own root, NaN and +inf among them -- and NULL, on the 193-sphere field and on the 2 562-sphere
    one: rt_occluded_rays answers as the composer does and as the unflagged context."""
    for c, flags in ((Q.small_case(pkg, ("sphere", 193)), four(pkg)), (B.beyond(B.BEYOND[0]), by_size(pkg))):
        assert np.isnan(c.t_max).any() and np.isinf(c.t_max).any() and ((c.t_max > 0) & (c.t_max < 100)).any()
        r, twin = renderer(pkg, c.sc, flags), renderer(pkg, c.sc, flags & ~pkg.RT_FLAG_STREAM_CULL_RAYS, False)
        try:
            want, want_all = rays_ref.occluded(c.osc, c.rays, c.t_max), rays_ref.occluded(c.osc, c.rays)
            assert not np.array_equal(want, want_all)      # (t_max decides some ray)
            for t_max, w in ((c.t_max, want), (None, want_all)):
                got = occluded_dev(r, c.rays, t_max)
                assert np.array_equal(got, w) and np.array_equal(got, occluded_dev(twin, c.rays, t_max))
        finally:
            r.cleanup_update()
            twin.cleanup_update()


# ---- 8. rt_set_scene ----------------------------------------------------------------------------------------------------------------------
def test_after_rt_set_scene_the_queries_are_the_moved_scenes(pkg):
    sc, coefs, c = B.moved_beyond(pkg)
    r, fresh = renderer(pkg, sc, by_size(pkg)), renderer(pkg, c.sc, by_size(pkg) & ~pkg.RT_FLAG_STREAM_CULL_RAYS, False)
    try:
        before = trace_dev(r, c.rays)
        r.set_scene(coefs=coefs)
        assert r.stream_cull_rays and r.set_scene_status()["applied"] == 1
        got = ray_outputs(r, c.rays, c.t_max)
        assert not rays_ref.same_records(got["rt_trace_rays"], before)
        assert_same_outputs(got, ray_outputs(fresh, c.rays, c.t_max), "moved")
        check_ray_queries(r, c, Composed(c.osc, c.rays, c.t_max), "moved")
    finally:
        r.cleanup_update()
        fresh.cleanup_update()


def test_one_graph_of_an_update_and_the_four_entry_points(pkg):
    """rt_set_scene, rt_trace_rays, rt_occluded_rays, rt_shade_rays and rt_trace_paths, all with ms == NULL, as a linear chain on one stream:
    replayed twice, with the moved and then with the first coefficients, the graph gives what the uncaptured calls give."""
    import torch
    sc, moved, c = B.moved_beyond(pkg)
    first = sc.arrays()["coefs"].copy()
    r = renderer(pkg, sc, by_size(pkg))
    s = torch.cuda.Stream()
    nr = len(c.rays)
    m = r._max_segments(None)
    try:
        with torch.cuda.stream(s):
            d_coefs, d_rays = torch.from_numpy(moved.copy()).to("cuda:0"), to_device(c.rays)
            d_tmax = torch.from_numpy(c.t_max.copy()).to("cuda:0")
            hits = torch.zeros((nr, 6), dtype=torch.float64, device="cuda:0")
            blocked = torch.zeros((nr,), dtype=torch.int32, device="cuda:0")
            rgba = torch.zeros((nr, 4), dtype=torch.float32, device="cuda:0")
            seg = torch.zeros((m * nr, 6), dtype=torch.float64, device="cuda:0")
            last = torch.zeros((nr, 6), dtype=torch.float64, device="cuda:0")
            ends = torch.zeros((nr, 4), dtype=torch.int32, device="cuda:0")
        outs = (hits, blocked, rgba, seg, last, ends)
        torch.cuda.synchronize()

        def chain():
            r.set_scene_into(coefs=d_coefs.data_ptr(), stream=s.cuda_stream)
            r.trace_into(d_rays.data_ptr(), nr, hits.data_ptr(), stream=s.cuda_stream, timed=False)
            r.occluded_into(d_rays.data_ptr(), d_tmax.data_ptr(), nr, blocked.data_ptr(), stream=s.cuda_stream, timed=False)
            r.shade_into(d_rays.data_ptr(), nr, rgba.data_ptr(), stream=s.cuda_stream, timed=False)
            r.paths_into(d_rays.data_ptr(), nr, m, seg.data_ptr(), last.data_ptr(), ends.data_ptr(), stream=s.cuda_stream, timed=False)

        plain = []
        for coefs in (moved, first):   # the uncaptured calls, on the same stream
            with torch.cuda.stream(s):
                d_coefs.copy_(torch.from_numpy(coefs.copy()))
            chain()
            s.synchronize()
            plain.append([o.cpu().numpy().tobytes() for o in outs])
        assert all(a != b for a, b in zip(*plain))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            chain()
        for k, coefs in enumerate((moved, first)):
            with torch.cuda.stream(s):
                d_coefs.copy_(torch.from_numpy(coefs.copy()))
                for o in outs:
                    o.view(torch.uint8).fill_(0xAB)
                g.replay()
            s.synchronize()
            assert [o.cpu().numpy().tobytes() for o in outs] == plain[k], ("replay", k)
        del g
    finally:
        torch.cuda.synchronize()
        r.cleanup_update()
    # ... and what the chain gave for the moved scene is what a fresh unflagged context of that scene gives
    fresh = renderer(pkg, c.sc, by_size(pkg) & ~pkg.RT_FLAG_STREAM_CULL_RAYS, False)
    try:
        assert plain[0][0] == trace_dev(fresh, c.rays).tobytes() and plain[0][1] == occluded_dev(fresh, c.rays, c.t_max).tobytes()
        assert plain[0][2] == H.shade_dev(fresh, c.rays)[0].tobytes()
    finally:
        fresh.cleanup_update()


# ---- 9. plumbing --------------------------------------------------------------------------------------------------------------------------
def test_host_forms_and_pick_paths(pkg):
    """rt_trace_rays_host, rt_shade_rays_host and rt_trace_paths_host go through the same launch sites, rt_pick_paths through the path one:
    each equals the unflagged context's, the path planes of every pixel included."""
    c = Q.small_case(pkg, ("sphere", 193))
    sc = c.sc.set_max_reflections(4)
    xy = all_pixels(64, 48)
    r, twin = renderer(pkg, sc, four(pkg)), renderer(pkg, sc, four(pkg) & ~pkg.RT_FLAG_STREAM_CULL_RAYS, False)
    try:
        o, d = c.rays["o"], c.rays["d"]
        got = {"rt_trace_rays_host": r.trace(o, d), "rt_shade_rays_host": r.shade(o, d)}
        want = {"rt_trace_rays_host": twin.trace(o, d), "rt_shade_rays_host": twin.shade(o, d)}
        for k, (a, b) in enumerate(zip(r.paths(o, d), twin.paths(o, d))):
            got[("rt_trace_paths_host", k)], want[("rt_trace_paths_host", k)] = a, b
        for k, (a, b) in enumerate(zip(r.pick_paths(xy), twin.pick_paths(xy))):
            got[("rt_pick_paths", k)], want[("rt_pick_paths", k)] = a, b
        assert_same_outputs(got, want, "host forms")
        assert (got[("rt_pick_paths", 0)][1]["object"] >= 0).any()      # (some pixel's path has a second segment)
        assert rays_ref.same_records(got["rt_trace_rays_host"], trace_dev(r, c.rays))
    finally:
        r.cleanup_update()
        twin.cleanup_update()


def test_multi_renderer(pkg):
    c = Q.small_case(pkg, ("sphere", 193))
    one = renderer(pkg, c.sc, four(pkg) & ~pkg.RT_FLAG_STREAM_CULL_RAYS, False)
    try:
        want = trace_dev(one, c.rays)
        want_rgba = one.shade(c.rays["o"], c.rays["d"])
    finally:
        one.cleanup_update()
    m = pkg.MultiRenderer(c.sc, [0, 0], band_rows=8, parts=2, flags=four(pkg))
    try:
        assert m.stream_cull_rays is True and m.query.streamed_queries
        assert rays_ref.same_records(m.trace(c.rays["o"], c.rays["d"]), want), "rt_trace_rays on rt_multi_query_ctx"
        assert np.ascontiguousarray(m.shade(c.rays["o"], c.rays["d"])).tobytes() == np.ascontiguousarray(want_rgba).tobytes()
    finally:
        m.cleanup_update()
    m = pkg.MultiRenderer(c.sc, [0, 0], band_rows=8, parts=2, flags=four(pkg) & ~pkg.RT_FLAG_STREAM_CULL)
    try:
        assert m.stream_cull_rays is False
    finally:
        m.cleanup_update()


ADAPTER = r"""
import ctypes as C, os, re, subprocess, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "tools"))
import __graft_entry__ as g
import query_table_scenes as Q, rays_ref
pkg = g.load_package()
c = Q.small_case(pkg, ("sphere", 193))
upd = C.CDLL(pkg.UPDATE_LIB_PATH)
names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
update = getattr(upd, re.search(r"\b(_Z\d+updateRKN3glm3matI\S*)\b", names).group(1))
cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
update.argtypes, update.restype = [C.c_void_p], C.c_float
upd.mi355rt_update_context.restype = C.c_void_p
upd.mi355rt_update_trace.argtypes = [C.c_void_p, C.c_uint, C.c_void_p]
cam = np.ascontiguousarray(pkg.IDENTITY, dtype=np.float64)
init(7, c.sc._h)
update(cam.ctypes.data)
on = C.c_uint32(9)
rc_on = pkg.lib().rt_get_stream_cull_rays(C.c_void_p(upd.mi355rt_update_context()), C.byref(on))
rays = np.ascontiguousarray(c.rays)
got = np.zeros(len(rays), dtype=rays_ref.HIT_DTYPE)
rc = upd.mi355rt_update_trace(C.c_void_p(rays.ctypes.data), len(rays), C.c_void_p(got.ctypes.data))
cleanup()
print("trace", rc_on, on.value, rc, bool(rays_ref.same_records(got, rays_ref.closest(c.osc, c.rays))))
"""


def test_init_update_with_the_environment_switch():
    """The reference's back-end contract in a fresh process, on the 193-sphere field: with all four switches the adapter's context culls
    its ray hooks' rays and mi355rt_update_trace returns the composer's records; without MI355RT_STREAM_CULL the switch is simply nothing."""
    def run(**env):
        return subprocess.run([sys.executable, "-c", ADAPTER, ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))
    out = run(MI355RT_STREAM="1", MI355RT_STREAM_QUERIES="1", MI355RT_STREAM_CULL="1", MI355RT_STREAM_CULL_RAYS="1")
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "trace 0 1 0 True", out.stdout
    out = run(MI355RT_STREAM="1", MI355RT_STREAM_QUERIES="1", MI355RT_STREAM_CULL_RAYS="1")
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "trace 0 0 0 True", out.stdout
    out = run(MI355RT_STREAM_CULL_RAYS="yes")
    assert out.returncode != 0 and "mi355rt: MI355RT_STREAM_CULL_RAYS: expected 0 or 1" in out.stderr, (out.stdout, out.stderr)


# ---- 10. the decision ---------------------------------------------------------------------------------------------------------------------
def decision_cases(pkg):
    f = pkg
    c193, c64 = Q.small_case(pkg, ("sphere", 193)), Q.small_case(pkg, ("sphere", 64))
    return [("without RT_FLAG_STREAM_CULL", c193, four(pkg) & ~f.RT_FLAG_STREAM_CULL),
            ("without RT_FLAG_STREAM_QUERIES", c193, four(pkg) & ~f.RT_FLAG_STREAM_QUERIES),
            ("with RT_FLAG_NOCULL", c193, four(pkg) | f.RT_FLAG_NOCULL),
            ("one chunk", c64, four(pkg)),
            ("not streamed", c193, four(pkg) & ~f.RT_FLAG_STREAM)]


@pytest.mark.parametrize("case", range(5))
def test_decision_false_is_the_context_without_the_flag(pkg, monkeypatch, case):
    """The getter says 0, rt_debug_stream_cull_rays is refused, the blob and the bounds are the unflagged context's and so is every output.
    (No instantiation is excluded, so no scene is.)"""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    what, c, flags = decision_cases(pkg)[case]
    r, p = renderer(pkg, c.sc, flags, False), renderer(pkg, c.sc, flags & ~pkg.RT_FLAG_STREAM_CULL_RAYS, False)
    try:
        assert r.stream_cull == p.stream_cull and r.streamed == p.streamed and r.streamed_queries == p.streamed_queries, what
        with pytest.raises(pkg.RtError) as e:
            r.stream_cull_rays_stats()
        assert e.value.code == -1 and "rt_debug_stream_cull_rays" in e.value.message and "MI355RT_STREAM_CULL_STATS" in e.value.message
        assert r.debug_scene_blob().tobytes() == p.debug_scene_blob().tobytes(), what
        if r.stream_cull:
            assert np.ascontiguousarray(r.stream_bounds()).tobytes() == np.ascontiguousarray(p.stream_bounds()).tobytes(), what
        assert_same_outputs(ray_outputs(r, c.rays, c.t_max), ray_outputs(p, c.rays, c.t_max), what)
    finally:
        r.cleanup_update()
        p.cleanup_update()


def test_decision_true_otherwise(pkg):
    c = Q.small_case(pkg, ("sphere", 65))
    for flags in (four(pkg), four(pkg) | pkg.RT_FLAG_FAST, four(pkg) | pkg.RT_FLAG_NOLEAN, four(pkg) | pkg.RT_FLAG_STREAM_CULL_BOUNCE):
        renderer(pkg, c.sc, flags).cleanup_update()


def test_without_the_environment_switch_there_are_no_work_words(pkg, monkeypatch):
    monkeypatch.delenv("MI355RT_STREAM_CULL_STATS", raising=False)
    c = Q.small_case(pkg, ("sphere", 129))
    r = renderer(pkg, c.sc, four(pkg))
    try:
        trace_dev(r, c.rays)
        with pytest.raises(pkg.RtError) as e:
            r.stream_cull_rays_stats()
        assert e.value.code == -1 and "MI355RT_STREAM_CULL_STATS" in e.value.message
    finally:
        r.cleanup_update()


# ---- 11. statistics -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expectation():
    return RL.expectation("row")


def stats_contexts(pkg):
    sc = BL.bounce_scene(pkg)
    return renderer(pkg, sc, four(pkg)), renderer(pkg, sc, four(pkg) & ~pkg.RT_FLAG_STREAM_CULL_RAYS, False)


def test_statistics_of_rt_trace_rays(pkg, monkeypatch):
    """bounce_cull_lab's 320 clustered spheres (5 chunks), the 64 x 48 frame's own primary rays in row order, a wave being 64 consecutive
    rays: [0] == D exactly (48 waves x 5 chunks = 240); [0] - [1] >= L (184 by the CPU's distance rule); fewer pairs reach than were asked;
    every query had a lane that can be culled for; cumulative over two calls.  (An MI355X gave the words [240, 53, 15360, 462, 0, 0, 0, 0]
    for one call.)"""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    e = expectation()
    assert e["D"] == 240 and e["L"] >= e["D"] / 2
    r, p = stats_contexts(pkg)
    try:
        assert r.stream_cull_rays_stats() == [0] * 8
        got = trace_dev(r, e["rays"])
        w = r.stream_cull_rays_stats()
        print("work words of rt_trace_rays", w, "expected D", e["D"], "L", e["L"])
        assert w[0] == e["D"], w
        assert w[0] - w[1] >= e["L"], w
        assert w[2] == len(e["rays"]) * e["n_chunks"] and w[3] < w[2], w
        assert w[4] == 0 and w[5:] == [0, 0, 0]
        assert rays_ref.same_records(got, trace_dev(p, e["rays"])) and (got["object"] >= 0).any()
        trace_dev(r, e["rays"])
        assert r.stream_cull_rays_stats() == [2 * x for x in w]      # cumulative
    finally:
        r.cleanup_update()
        p.cleanup_update()


def test_statistics_of_rt_occluded_rays(pkg, monkeypatch):
    """... with NULL t_max: [1] <= D - L -- a blocked lane asks about no further bound and a wave stops behind the chunk that blocks its
    last undecided lane, so fewer chunks still are staged."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    e = expectation()
    r, p = stats_contexts(pkg)
    try:
        got = occluded_dev(r, e["rays"])
        w = r.stream_cull_rays_stats()
        print("work words of rt_occluded_rays", w)
        assert w[1] <= e["D"] - e["L"] and 0 < w[0] <= e["D"] and w[4] == 0, w
        assert np.array_equal(got, occluded_dev(p, e["rays"])) and got.any() and not got.all()
    finally:
        r.cleanup_update()
        p.cleanup_update()


@pytest.mark.parametrize("which", ["rt_shade_rays", "rt_trace_paths"])
def test_statistics_of_the_shading_and_the_path_loop(pkg, monkeypatch, which):
    """Chunks are left unstaged ([0] - [1] > 0) and the outputs are the unflagged context's."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    e = expectation()
    r, p = stats_contexts(pkg)
    try:
        if which == "rt_shade_rays":
            got, want = H.shade_dev(r, e["rays"], hits=True), H.shade_dev(p, e["rays"], hits=True)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        else:
            got, want = P.paths_dev(r, e["rays"]), P.paths_dev(p, e["rays"])
            assert all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(got, want))
            assert (got[0][1]["object"] >= 0).any()      # (some ray bounces)
        w = r.stream_cull_rays_stats()
        print("work words of", which, w)
        assert w[0] - w[1] > 0 and w[0] > e["D"] and w[3] < w[2], w
    finally:
        r.cleanup_update()
        p.cleanup_update()
