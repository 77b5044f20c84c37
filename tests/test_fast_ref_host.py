"""The instrument that holds the RT_FLAG_FAST kernels (tests/tools/fast_ref.py: exact arithmetic, the running-error bound B, the
"decided" classification) is itself held here, on the CPU, before it judges a kernel (tests/test_fast_truth_gpu.py uses the same
scenes, rays and checks):
  * the reference's own float64 arithmetic (the oracle) passes: rho = |t - t_exact| / B <= 1 on every decided ray, the exact winner;
  * the kernels' arithmetic compiled for the host with FMA contraction (tests/tools/fast_host_lab.cpp) passes, dense and class-table form;
  * six wrong kernels are rejected on at least one decided ray of every set;
  * the share of rays the check leaves out is within its cap (1 % of a query set, 0.2 % of a frame's pixels) with the reference alone.
Degree 3 (the second half of this file; fast_ref.py, "DEGREE 3") the same way on its own sets: the oracle within B3 on every winner and
on every ray/object pair of a part of the grid, the contracted host build in its dense and its guarded form (guarded answers to
B3 + CUB_TOL |t|) with results that differ from the strict host build's bits, eight wrong kernels rejected, the caps met by the
reference alone -- and scenes/cayley.yml from the origin, where no ray is decided, failing its cap."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import fast_ref as F  # noqa: E402
import rays_ref  # noqa: E402
import stream_scenes as S  # noqa: E402

@functools.lru_cache(maxsize=None)
def case(name):
    """(oracle scene, the 2 048 query rays, their per-ray t_max, the oracle's closest hits, its blocked flags without and with t_max)."""
    import __graft_entry__ as graft
    pkg = graft.load_package()
    osc = S.oracle_of(pkg, F.scene(pkg, name))
    rays = F.query_rays(osc, F.RAY_SEED)
    t_max = F.query_t_max(osc, rays, F.TMAX_SEED)
    return osc, rays, t_max, rays_ref.closest(osc, rays), rays_ref.occluded(osc, rays), rays_ref.occluded(osc, rays, t_max)


@functools.lru_cache(maxsize=None)
def frame_case(name):
    """(oracle scene, the primary rays of its 96 x 72 frame, the oracle's closest hits): the G-buffer's and rt_pick's set."""
    osc = case(name)[0]
    rays = rays_ref.primary_rays(osc)
    return osc, rays, rays_ref.closest(osc, rays)


def passes(rep, cap=F.QUERY_CAP):
    print(rep)
    assert rep.passed(cap), str(rep)
    return rep


def rejected(rep):
    """The check fails, and on a decided ray: failures are only ever raised for those."""
    print(f"{rep.what}: " + (f"rejected: {rep.failures[0]}" if rep.failures else "NOT rejected"))
    assert rep.failures, f"{rep.what}: the check let a wrong result pass"


@pytest.mark.parametrize("name", F.SCENES)
def test_the_sets_reach_what_they_are_for(pkg, name):
    osc, rays, t_max, want, blocked, blocked_tm = case(name)
    coefs = np.asarray(osc.coefs).reshape(-1, 20)
    assert len(rays) == F.N_RAYS and not coefs[:, :10].any()
    hit = want["object"] >= 0
    assert hit.sum() > F.N_RAYS // 4 and (~hit).sum() > 20
    assert len(set(want["object"][hit].tolist())) >= (24 if name != "chunked" else 128)
    assert 0 < blocked_tm.sum() < blocked.sum() < F.N_RAYS
    pr = F.pairs(coefs, rays["o"], rays["d"])
    inside = (pr["t0"] < 0).any(axis=1)            # an origin inside some closed surface: the solver's second root
    assert inside[F.N_RAYS // 2:].sum() > 200
    if name == "spheres":
        assert all(ob.reflection_ratio == 0.0 for ob in osc.objects) and len(coefs) == 24
    else:
        kinds = [(q[10:13] == 1.0).all() and not q[13:16].any() for q in coefs]
        assert sum(kinds) >= 11 and sum(1 for q in coefs if q[13:16].any()) >= 5 and sum(1 for q in coefs if not q[10:16].any()) == 2
        assert sum(1 for ob in osc.objects if ob.reflection_ratio > 0) >= 2 and {int(lt.is_spherical) for lt in osc.lights} == {0, 1}
    if name == "chunked":
        assert sum(kinds) == 65 and len(coefs) - 2 - sum(kinds) == 65


@pytest.mark.parametrize("name", F.SCENES)
def test_the_references_arithmetic_passes(pkg, name):
    osc, rays, t_max, want, blocked, blocked_tm = case(name)
    rep = passes(F.check_closest(osc, rays, want, f"oracle, {name}, closest"))
    assert rep.worst_rho > 0.0   # (it measured something)
    passes(F.check_occluded(osc, rays, None, blocked, f"oracle, {name}, occluded"))
    passes(F.check_occluded(osc, rays, t_max, blocked_tm, f"oracle, {name}, occluded with t_max"))
    osc, rays, want = frame_case(name)
    passes(F.check_closest(osc, rays, want, f"oracle, {name}, the frame's primary rays", pixel_dirs=True), F.FRAME_CAP)


@pytest.mark.parametrize("name", F.SCENES)
def test_frame_sets_meet_their_caps(pkg, name):
    """The primary rays of the 96 x 72 frame: the G-buffer's and rt_pick's set (direction term on) and the frames' (whole paths)."""
    osc, rays, _ = frame_case(name)
    n = len(rays)
    first = F.decided_closest(osc, rays, pixel_dirs=True)
    paths = F.decided_paths(osc, rays, pixel_dirs=True)
    print(f"{name}: {int((~first[3]).sum())} of {n} primary rays and {int((~paths).sum())} of {n} paths not decided")
    assert (~first[3]).sum() <= F.FRAME_CAP * n and (~paths).sum() <= F.FRAME_CAP * n
    assert not (paths & ~first[3]).any()
    assert (first[0] >= 0).sum() > n // 10
    with_dirs = F.decided_closest(osc, rays, pixel_dirs=True)[2]
    hit = first[0] >= 0
    assert (with_dirs[hit] > F.decided_closest(osc, rays)[2][hit]).all()   # the direction term is there


# ---- the kernels' arithmetic, contracted, on the host ----------------------------------------------------------------------------------------
def host_has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read().replace("\n", " ")
    except OSError:
        return False


@functools.lru_cache(maxsize=None)
def lab(contract="fast"):
    """tests/tools/fast_host_lab.cpp, contracted (what the tests hold) or strict (only to show that the other build is contracted)."""
    out = os.path.join(ROOT, "tests", "tools", "bin", "libfast_host_lab.so" if contract == "fast" else f"libfast_host_lab_{contract}.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O2", "-mfma", "-ffp-contract=" + contract, "-DRT_FAST=1", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tools", "flopcount_shim"),
                    "-I" + os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc"), os.path.join(ROOT, "tests", "tools", "fast_host_lab.cpp"), "-o", out], check=True)
    lib = C.CDLL(out)
    lib.lab_root.restype = C.c_double
    lib.lab_closest.restype = lib.lab_occluded.restype = C.c_int64
    return lib


def _p(a, ct=C.c_double):
    return a.ctypes.data_as(C.POINTER(ct))


def lab_closest(osc, rays, form, contract="fast", more=False):
    """HIT_DTYPE records; more: also (guarded [n] bool, branch [n], the number of degree-3 tests cubic_guarded refused)."""
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, 20)
    flat = np.ascontiguousarray(rays).view(np.float64).reshape(-1, 6)
    out = np.zeros(len(rays), dtype=rays_ref.HIT_DTYPE)
    obj, t, p, nv = np.zeros(len(rays), dtype=np.int32), np.zeros(len(rays)), np.zeros((len(rays), 3)), np.zeros((len(rays), 3), dtype=np.float32)
    guarded, branch = np.zeros(len(rays), dtype=np.int32), np.zeros(len(rays), dtype=np.int32)
    refused = lab(contract).lab_closest(_p(coefs), len(coefs), _p(flat), len(rays), form, _p(obj, C.c_int32), _p(t), _p(p), _p(nv, C.c_float), _p(guarded, C.c_int32),
                                        _p(branch, C.c_int32))
    out["object"], out["t"], out["point"], out["normal"] = obj, t, p, nv
    return (out, guarded != 0, branch, int(refused)) if more else out


def lab_occluded(osc, rays, t_max, form):
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, 20)
    flat = np.ascontiguousarray(rays).view(np.float64).reshape(-1, 6)
    tm = np.ascontiguousarray(np.broadcast_to(np.asarray(F.MAX_T if t_max is None else t_max, dtype=np.float64), (len(rays),)))
    out = np.zeros(len(rays), dtype=np.int32)
    lab().lab_occluded(_p(coefs), len(coefs), _p(flat), _p(tm), len(rays), form, _p(out, C.c_int32))
    return out


@pytest.mark.skipif(not host_has_fma(), reason="the host CPU has no FMA: a contracted host build cannot run here")
@pytest.mark.parametrize("form", [0, 1], ids=["dense", "class tables"])
@pytest.mark.parametrize("name", F.SCENES)
def test_a_contracted_host_build_passes(pkg, name, form):
    osc, rays, t_max, want, _, _ = case(name)
    got = lab_closest(osc, rays, form)
    both = (got["object"] >= 0) & (got["object"] == want["object"])
    differ = int((got["t"][both] != want["t"][both]).sum())
    print(f"{name}, form {form}: t differs from the strict oracle's in {differ} of {int(both.sum())} hits")
    assert differ > 0, "this build is not contracted: it says nothing about FMA"
    passes(F.check_closest(osc, rays, got, f"contracted host build, {name}, form {form}, closest"))
    passes(F.check_occluded(osc, rays, None, lab_occluded(osc, rays, None, form), f"contracted host build, {name}, form {form}, occluded"))
    passes(F.check_occluded(osc, rays, t_max, lab_occluded(osc, rays, t_max, form), f"contracted host build, {name}, form {form}, occluded with t_max"))
    osc, rays, _ = frame_case(name)
    passes(F.check_closest(osc, rays, lab_closest(osc, rays, form), f"contracted host build, {name}, form {form}, the frame's primary rays", pixel_dirs=True), F.FRAME_CAP)


# ---- wrong kernels ---------------------------------------------------------------------------------------------------------------------------
def records_from(osc, rays, win, t):
    """HIT_DTYPE records of a closest-hit answer (object, t) with point = o + t d and the float64 normal there."""
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, 20)
    out = np.zeros(len(rays), dtype=rays_ref.HIT_DTYPE)
    out["object"], out["t"] = win, np.where(win >= 0, t, np.inf)
    hit = win >= 0
    p = rays["o"][hit] + t[hit][:, None] * rays["d"][hit]
    out["point"][hit] = p
    out["normal"][hit] = F._normals(coefs[win[hit]], p).astype(np.float32)
    return out


def closest_mutations(osc, rays, want, what, pixel_dirs):
    """The five wrong closest-hit kernels on one set: each must fail the check on a decided ray."""
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, 20)
    o, d = rays["o"], rays["d"]

    def check(got, mutation):
        rejected(F.check_closest(osc, rays, got, f"{what}: {mutation}", pixel_dirs=pixel_dirs, stop_at_first=True))
    # t scaled by 1 + 2^-40
    m = want.copy()
    m["t"] = np.where(m["object"] >= 0, m["t"] * (1.0 + 2.0 ** -40), m["t"])
    check(m, "t scaled by 1 + 2^-40")
    # the other root of the winner's quadratic (where the winner has one)
    win, t, _, _, second, pr = F.closest_arrays(coefs, o, d)
    rows = np.arange(len(rays))
    other = pr["other"][rows, np.maximum(win, 0)]
    m = want.copy()
    swap = (win >= 0) & np.isfinite(other)
    m["t"] = np.where(swap, other, m["t"])
    assert swap.sum() > 100
    check(m, "the other root")
    # one product dropped from t1; t0 through float32: the nearest-hit search over the wrong roots
    for kind, mutation in (("drop", "a product dropped from t1"), ("f32", "t0 through float32")):
        w2, t2 = F.closest_arrays(coefs, o, d, mutate=kind)[:2]
        check(records_from(osc, rays, w2, t2), mutation)
    # the second-lowest object on rays that have one (a set without ties: no ray is excluded)
    two = second >= 0
    assert two.sum() > 20
    t_second = pr["t"][rows, np.maximum(second, 0)]
    check(records_from(osc, rays, np.where(two, second, win), np.where(two, t_second, t)), "the second-lowest object")


@pytest.mark.parametrize("name", F.SCENES)
def test_mutations_are_rejected(pkg, name):
    osc, rays, t_max, want, blocked, blocked_tm = case(name)
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, 20)
    closest_mutations(osc, rays, want, f"{name}, query rays", False)
    closest_mutations(*frame_case(name), f"{name}, the frame's primary rays", True)
    for lim, flags in ((None, blocked), (t_max, blocked_tm)):
        # a product dropped from t1, in the shadow loop
        got = F.occluded_arrays(coefs, rays["o"], rays["d"], F.MAX_T if lim is None else lim, mutate="drop")[0]
        rejected(F.check_occluded(osc, rays, lim, got, f"{name}: a product dropped from t1, occluded"))
        # a blocked flag inverted: one decided ray's flag
        decided = F.decided_occluded(osc, rays, lim)[1]
        m = flags.copy()
        i = int(np.flatnonzero(decided)[len(rays) // 3])
        m[i] ^= 1
        rep = F.check_occluded(osc, rays, lim, m, f"{name}: one blocked flag inverted")
        rejected(rep)
        assert len(rep.failures) == 1 and f"ray {i} " in rep.failures[0]


# ---- degree 3 ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cubic_case(name):
    """(oracle scene, the 1 024 query rays, their per-ray t_max, the oracle's closest hits, its blocked flags without and with t_max)."""
    osc = F.cubic_scene(name)
    rays = F.cubic_query_rays(osc, name)
    t_max = F.query_t_max(osc, rays, F.TMAX_SEED)
    return osc, rays, t_max, rays_ref.closest(osc, rays), rays_ref.occluded(osc, rays), rays_ref.occluded(osc, rays, t_max)


@functools.lru_cache(maxsize=None)
def cubic_frame_case(name, frame):
    """(oracle scene, its frame's primary rays, the oracle's closest hits).  frame False: the G-buffer's and rt_pick's set, the query
    set's own scene; True: the frames' scene (F.CUBIC_FRAME_SEED)."""
    osc = F.cubic_scene(name, frame=frame)
    rays = rays_ref.primary_rays(osc)
    return osc, rays, rays_ref.closest(osc, rays)


def pair_rays(name, rays):
    """The rays whose every ray/object pair is held: every third ray of the primary grid (bent65: every 24th -- 65 objects each)."""
    return rays[:512:24] if name == "bent65" else rays[:512:3]


def oracle_pairs(osc, rays):
    """[n, m]: orc_intersect_ray of every ray against every object alone."""
    L, dp = rays_ref.O.lib(), C.POINTER(C.c_double)
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, 20)
    out = np.zeros((len(rays), len(coefs)))
    for i in range(len(rays)):
        o, d = np.ascontiguousarray(rays["o"][i]), np.ascontiguousarray(rays["d"][i])
        for k in range(len(coefs)):
            out[i, k] = L.orc_intersect_ray(_p(coefs[k]), o.ctypes.data_as(dp), d.ctypes.data_as(dp))
    return out


def lab_pairs(osc, rays, form, contract="fast"):
    """(t [n, m], refused [n, m] bool) of tests/tools/fast_host_lab.cpp: every ray against every object alone."""
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, 20)
    flat = np.ascontiguousarray(rays).view(np.float64).reshape(-1, 6)
    t, refused = np.zeros((len(rays), len(coefs))), np.zeros((len(rays), len(coefs)), dtype=np.int32)
    lab(contract).lab_pairs(_p(coefs), len(coefs), _p(flat), len(rays), form, _p(t), _p(refused, C.c_int32))
    return t, refused != 0


@pytest.mark.parametrize("name", F.CUBIC_SCENES)
def test_degree3_sets_reach_what_they_are_for(pkg, name):
    osc, rays, t_max, want, blocked, blocked_tm = cubic_case(name)
    coefs = np.asarray(osc.coefs).reshape(-1, 20)
    cubic = coefs[:, :10].any(axis=1)
    hit = want["object"] >= 0
    assert len(rays) == F.CUBIC_N_RAYS and hit.sum() > F.CUBIC_N_RAYS // 4
    assert 0 < blocked_tm.sum() < blocked.sum() <= F.CUBIC_N_RAYS
    lengths = np.linalg.norm(rays["d"][512:], axis=1)
    assert lengths.min() < 0.6 and lengths.max() > 1.9
    pr = F.pairs(coefs, rays["o"], rays["d"])
    branch = pr["branch"][np.arange(len(rays)), np.maximum(want["object"], 0)][hit & cubic[np.maximum(want["object"], 0)]]
    print(f"{name}: {int(hit.sum())} hits, winners by branch (0 Cardano, 1 trigonometric): {dict(zip(*np.unique(branch, return_counts=True)))}")
    assert (branch == 0).sum() > 20 and (branch == 1).sum() > 20
    if name == "clebsch":
        # the only set that reaches the trigonometric branch and the guard's refusals in numbers: as the kernels' own header sees it
        assert cubic.sum() == 1
        if host_has_fma():
            _, guarded, lab_branch, refused = lab_closest(osc, rays, 1, more=True)
            print(f"clebsch, host lab: {int((lab_branch == 0).sum())} Cardano winners, {int((lab_branch == 1).sum())} trigonometric winners, {refused} refused tests")
            assert (lab_branch == 0).sum() > 100 and (lab_branch == 1).sum() > 100 and refused > 10
        assert np.isfinite(pr["other"][:, 0]).sum() > 50     # three roots, the smallest at or above EPS: a root choice to get wrong
    else:
        assert cubic.sum() == (65 if name == "bent65" else 8) > 4     # more than the RT_CUB_AT_MAX records the host forms
        assert sum(1 for ob in osc.objects if ob.reflection_ratio > 0) >= 2 and {int(lt.is_spherical) for lt in osc.lights} == {0, 1}
        assert len(set(want["object"][hit].tolist())) >= (8 if name != "bent65" else 60)
    if name == "bent8 mixed":
        assert (~cubic).sum() == 9 and (~cubic[want["object"][hit]]).sum() > 20 and cubic[want["object"][hit]].sum() > 20   # winners of both kinds
    if name == "bent65":
        assert (want["object"][hit] == 64).any()   # the entry past the streamed chunk owns rays


@pytest.mark.parametrize("name", F.CUBIC_SCENES)
def test_the_references_arithmetic_passes_degree3(pkg, name):
    """The oracle under glibc: B3 alone is its bar.  Winners of every ray, every ray/object pair of a part of the grid, the flags."""
    osc, rays, t_max, want, blocked, blocked_tm = cubic_case(name)
    rep = passes(F.check_closest(osc, rays, want, f"oracle, {name}, closest"))
    assert rep.worst_rho > 0.0
    sub = pair_rays(name, rays)
    rep = passes(F.check_pairs(osc.coefs, sub, oracle_pairs(osc, sub), f"oracle, {name}, every pair of {len(sub)} rays"))
    assert rep.worst_rho > 0.0 and rep.n >= len(sub)
    passes(F.check_occluded(osc, rays, None, blocked, f"oracle, {name}, occluded"))
    passes(F.check_occluded(osc, rays, t_max, blocked_tm, f"oracle, {name}, occluded with t_max"))
    if name != "clebsch":
        osc, rays, want = cubic_frame_case(name, False)
        passes(F.check_closest(osc, rays, want, f"oracle, {name}, the frame's primary rays", pixel_dirs=True), F.FRAME_CAP)


@pytest.mark.parametrize("name", F.CUBIC_FRAME_SCENES)
def test_degree3_frame_sets_meet_their_caps(pkg, name):
    osc, rays, want = cubic_frame_case(name, True)
    n = len(rays)
    first = F.decided_closest(osc, rays, pixel_dirs=True)
    paths = F.decided_paths(osc, rays, pixel_dirs=True)
    print(f"{name}: {int((~first[3]).sum())} of {n} primary rays and {int((~paths).sum())} of {n} paths not decided")
    assert n == 32 * 24 and osc.max_reflections == 2
    assert (~first[3]).sum() <= F.FRAME_CAP * n and (~paths).sum() <= F.FRAME_CAP * n
    assert not (paths & ~first[3]).any() and (first[0] >= 0).sum() > n // 10
    coefs = np.asarray(osc.coefs).reshape(-1, 20)
    assert coefs[first[0][first[0] >= 0], :10].any(axis=1).sum() > n // 10    # degree-3 hits, whose paths decided_paths walks
    passes(F.check_closest(osc, rays, want, f"oracle, {name}, the frames' primary rays", pixel_dirs=True), F.FRAME_CAP)


def test_the_cap_check_can_fail(pkg):
    """scenes/cayley.yml from the origin: F(0) = 0, a double root at t = 0 on every ray -- no ray is decided, and the cap says so."""
    osc = rays_ref.O.load_scene(os.path.join(ROOT, "scenes", "cayley.yml")).with_size(16, 24)
    rays = F.cone_rays((0.0, 0.0, 0.0), 25.0, 24, 16)
    want = rays_ref.closest(osc, rays)
    rep = F.check_closest(osc, rays, want, "oracle, cayley from the origin")
    print(rep)
    assert rep.excluded == rep.n == 384 and not rep.failures and not rep.passed(F.QUERY_CAP)
    blocked = rays_ref.occluded(osc, rays)
    rep = F.check_occluded(osc, rays, None, blocked, "oracle, cayley from the origin, occluded")
    assert rep.excluded == rep.n and not rep.passed(F.QUERY_CAP)


@pytest.mark.skipif(not host_has_fma(), reason="the host CPU has no FMA: a contracted host build cannot run here")
@pytest.mark.parametrize("form", [0, 1], ids=["dense", "guarded"])
@pytest.mark.parametrize("name", F.CUBIC_SCENES)
def test_a_contracted_host_build_passes_degree3(pkg, name, form):
    """Dense answers (cubic_poly + solve_cubic) are held to B3; the guarded form's to B3 + CUB_TOL |t| where cubic_guarded answered and
    to B3 where it refused."""
    osc, rays, t_max, want, _, _ = cubic_case(name)
    got, guarded, _, refused = lab_closest(osc, rays, form, more=True)
    strict = lab_closest(osc, rays, form, contract="off")
    both = (got["object"] >= 0) & (got["object"] == strict["object"])
    differ = int((got["t"][both] != strict["t"][both]).sum())
    print(f"{name}, form {form}: t differs from the strict host build's in {differ} of {int(both.sum())} hits; {refused} tests refused, "
          f"{int(guarded.sum())} winners answered by the guard")
    assert differ > 0, "this build is not contracted: it says nothing about FMA"
    assert (form == 1 and guarded.sum() > 100) or (form == 0 and not guarded.any() and refused == 0)
    passes(F.check_closest(osc, rays, got, f"contracted host build, {name}, form {form}, closest", guarded=guarded))
    sub = pair_rays(name, rays)
    t_pairs, pair_refused = lab_pairs(osc, sub, form)
    passes(F.check_pairs(osc.coefs, sub, t_pairs, f"contracted host build, {name}, form {form}, every pair of {len(sub)} rays", guarded=~pair_refused if form else False))
    passes(F.check_occluded(osc, rays, None, lab_occluded(osc, rays, None, form), f"contracted host build, {name}, form {form}, occluded"))
    passes(F.check_occluded(osc, rays, t_max, lab_occluded(osc, rays, t_max, form), f"contracted host build, {name}, form {form}, occluded with t_max"))
    if name != "clebsch":
        osc, rays, _ = cubic_frame_case(name, False)
        got, guarded, _, _ = lab_closest(osc, rays, form, more=True)
        passes(F.check_closest(osc, rays, got, f"contracted host build, {name}, form {form}, the frame's primary rays", pixel_dirs=True, guarded=guarded), F.FRAME_CAP)


def degree3_closest_mutations(osc, rays, want, what, pixel_dirs):
    """The wrong closest-hit kernels on one set, at the widest bar a kernel is held to (guarded everywhere): each must fail on a decided
    ray.  Returns which of the optional ones (a root choice, a second object) the set had rays for."""
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, 20)
    o, d = rays["o"], rays["d"]
    applied = set()

    def check(got, mutation):
        rejected(F.check_closest(osc, rays, got, f"{what}: {mutation}", pixel_dirs=pixel_dirs, stop_at_first=True, guarded=True))
    m = want.copy()
    m["t"] = np.where(m["object"] >= 0, m["t"].astype(np.float32).astype(np.float64), m["t"])
    check(m, "t through float32")
    m = want.copy()
    m["t"] = np.where(m["object"] >= 0, m["t"] * (1.0 + 2.0 ** -20), m["t"])
    check(m, "t scaled by 1 + 2^-20")
    win, t, _, decided, second, pr = F.closest_arrays(coefs, o, d, pixel_dirs=pixel_dirs)
    rows = np.arange(len(rays))
    other = pr["other"][rows, np.maximum(win, 0)]
    swap = (win >= 0) & np.isfinite(other) & pr["cubic"][np.maximum(win, 0)]
    if (swap & decided).any():
        m = want.copy()
        m["t"] = np.where(swap, other, m["t"])
        check(m, "the middle root where a smaller one >= EPS exists")
        applied.add("middle root")
    for kind, mutation in (("hyz", "the product hyz dy dz left out of the Taylor t2"), ("t3term", "one degree-3 coefficient's term left out of t3")):
        w2, t2 = F.closest_arrays(coefs, o, d, mutate=kind)[:2]
        check(records_from(osc, rays, w2, t2), mutation)
    two = second >= 0
    if (two & decided).any():
        t_second = pr["t"][rows, np.maximum(second, 0)]
        check(records_from(osc, rays, np.where(two, second, win), np.where(two, t_second, t)), "the second-nearest object")
        applied.add("second object")
    return applied


@pytest.mark.parametrize("name", F.CUBIC_SCENES)
def test_degree3_mutations_are_rejected(pkg, name):
    osc, rays, t_max, want, blocked, blocked_tm = cubic_case(name)
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, 20)
    applied = degree3_closest_mutations(osc, rays, want, f"{name}, query rays", False)
    assert "second object" in applied or name == "clebsch"   # (one object: nothing is second)
    assert "middle root" in applied or name != "clebsch"
    if name != "clebsch":
        degree3_closest_mutations(*cubic_frame_case(name, False), f"{name}, the frame's primary rays", True)
    cubic = coefs[:, :10].any(axis=1)
    for lim, flags in ((None, blocked), (t_max, blocked_tm)):
        limit = F.MAX_T if lim is None else lim
        got = F.occluded_arrays(coefs, rays["o"], rays["d"], limit, mutate="hyz")[0]
        rejected(F.check_occluded(osc, rays, lim, got, f"{name}: the product hyz dy dz left out, occluded"))
        decided = F.decided_occluded(osc, rays, lim)[1]
        m = flags.copy()
        i = int(np.flatnonzero(decided)[len(rays) // 3])
        m[i] ^= 1
        rep = F.check_occluded(osc, rays, lim, m, f"{name}: one blocked flag inverted")
        rejected(rep)
        assert len(rep.failures) == 1 and f"ray {i} " in rep.failures[0]
        # a shadow decision that accepts a degree-3 root below max_t without the EPS test
        t = F.pairs(coefs, rays["o"], rays["d"])["t"]
        lim_col = np.broadcast_to(np.asarray(limit, dtype=np.float64), (len(rays),))[:, None]
        got = (((t > F.EPS) | cubic[None, :]) & (t < lim_col)).any(axis=1)
        rejected(F.check_occluded(osc, rays, lim, got, f"{name}: x0 < max_t accepted without the EPS test"))
