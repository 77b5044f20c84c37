"""The degree-3 path on gfx950, ray by ray (tests/tools/cubic_device_lab.hip: the kernels' own rt_math.hpp in plain kernels).

Every degree-3 test of a frame -- primary rays, the shadow ray of every hit towards every light, the first bounce of mirror hits, formed
from the oracle as tests/tools/cubic_guard_lab.cpp forms them -- goes through intersect_cubic_taylor (what both kernels run) on the
device and through the oracle's intersect_ray.  Where the guard answers, the decision must be the oracle's and an accepted nearest-hit
root must agree to CUB_TOL; where it refuses, the dense path must be BITWISE the oracle's under the device's cbrt / acos / cos
(oracle.under_libm), branch included.  No allowance: a single differing ray fails.  The device's cbrt / acos / cos themselves are held
to a stated ulp bound against mpmath at 60 digits on every argument these scenes produce."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cubic_device_lab as D  # noqa: E402

pytestmark = pytest.mark.gpu

EPS, CUB_TOL = D.EPS, D.CUB_TOL
W, H = 200, 150
# The bound the device's cbrt / acos / cos are held to.  ROCm's device libm (ocml) ships no per-function accuracy table with its headers, so
# the bound is the measured one rounded up to faithful rounding: on gfx950, over every argument of the scenes below, cbrt 0.50 ulp,
# acos 0.75 ulp and cos 0.78 ulp of the correctly rounded value.
ULP_BOUND = {"cbrt": 1.0, "acos": 1.0, "cos": 1.0}
# dense branch of the device (intersect_cubic_branch) -> the oracle's (orc_intersect_ray_ex)
BRANCH_MAP = {0: (4,), 1: (5,), 2: (2, 3), 3: (0, 1)}


@pytest.fixture(scope="module")
def lab(pkg):
    return D.lib(pkg)


def many_cubic_scene(pkg):
    """The scene of test_cubic_gpu.py::test_many_cubic_objects_and_mirrors (six degree-3 objects, mirrors)."""
    from test_cubic_gpu import many_cubic_objects_and_mirrors
    return many_cubic_objects_and_mirrors(pkg)


def _scene(pkg, oracle, key):
    """(oracle scene, camera, product scene or None, max share of refused primary tests or None)"""
    from test_gpu_parity import oracle_from
    repo = {"clebsch": 0.03, "dingdong": 0.4, "monkey_saddle": 0.02, "cayley": 1.0, "cubic": 1.0}   # test_cubic_guard.py's bounds
    if key in repo:
        return (oracle.load_scene(scene_path(key)).with_size(W, H), None, pkg.Scene.load_from_file(scene_path(key)).set_size(W, H), repo[key])
    if key == "cayley_moved":
        cam = oracle.camera_matrix(pos=(0.3, 0.2, -4.0), yaw_deg=90.0, pitch_deg=0.0)
        return (oracle.load_scene(scene_path("cayley")).with_size(W, H), cam, pkg.Scene.load_from_file(scene_path("cayley")).set_size(W, H), 0.1)
    if key == "many_cubic":
        s = many_cubic_scene(pkg)
        return oracle_from(pkg, oracle, s), None, s, None
    seed = int(key.split("_")[1])
    osc, cam = D.CPU.fuzz_scene(seed)
    return osc, cam, None, None


_MEMO = {}


def _mp_roots(tc):
    import mpmath
    try:
        with mpmath.workdps(60):
            return [complex(r) for r in mpmath.polyroots([mpmath.mpf(float(x)) for x in tc], maxsteps=200, extraprec=200)]
    except Exception as e:  # (a degenerate polynomial: say so instead)
        return f"no roots ({e})"


def _describe(osc, rays, where, out, t_ref, tc_ref, t_dl, br_dl, idx, limit=5):
    lines = []
    for i in list(idx)[:limit]:
        r, w, q = rays[i], where[i], out[i]
        lines.append(f"{D.KINDS[w['kind']]} ray of pixel ({w['x']}, {w['y']}) light {w['light']}: object {r['obj']} coefs {list(osc.coefs[r['obj']])}\n"
                     f"    o {list(r['o'])} d {list(r['d'])} max_t {r['max_t']!r}\n"
                     f"    device: t {q['t']!r} refused {q['refused']} guard {q['guard_ok']} t_guard {q['t_guard']!r} dense {q['t_dense']!r} branch {q['branch']} taylor t3..t0 {list(q['tc'])}\n"
                     f"    oracle: t {t_ref[i]!r} (glibc) {t_dl[i]!r} (device libm, branch {br_dl[i]}) dense t3..t0 {list(tc_ref[i])}\n"
                     f"    mpmath roots of the oracle's t3..t0: {_mp_roots(tc_ref[i])}")
    return "\n".join(lines)


def _run(pkg, oracle, lab, key):
    """Every degree-3 test of the scene on the device and in the oracle; assertions 1 and 2 of the module's docstring.  Memoised: the
    argument tables feed the mpmath test."""
    if key in _MEMO:
        return _MEMO[key]
    osc, cam, psc, max_refused = _scene(pkg, oracle, key)
    rays, where = D.enumerate_rays(osc, cam)
    assert len(rays) > 0
    out = D.device_rays(lab, osc.coefs, rays)
    t_ref, tc_ref, _ = D.oracle_rays(osc, rays)
    (t_dl, _, br_dl), libm, rounds = D.oracle_rays_device_libm(lab, osc, rays)
    show = lambda idx: _describe(osc, rays, where, out, t_ref, tc_ref, t_dl, br_dl, np.flatnonzero(idx))  # noqa: E731

    refused = out["refused"] != 0
    answered = ~refused
    decide = (rays["flags"] & D.LAB_DECIDE) != 0
    max_t = rays["max_t"]
    # the guard alone says what intersect_cubic_taylor did, and returns its root unchanged
    assert np.array_equal(out["guard_ok"] != 0, answered), show((out["guard_ok"] != 0) != answered)
    assert np.array_equal(out["t"][answered].view(np.uint64), out["t_guard"][answered].view(np.uint64)), show(answered & (out["t"] != out["t_guard"]))
    # 1. guard answered: the oracle's decision, no exception
    with np.errstate(invalid="ignore"):
        acc = np.where(decide, (out["t"] > EPS) & (out["t"] < max_t), (out["t"] >= EPS) & (out["t"] < max_t))
        acc_ref = np.where(decide, (t_ref > EPS) & (t_ref < max_t), (t_ref >= EPS) & (t_ref < max_t))
        decision_diff = answered & (acc != acc_ref)
        assert not decision_diff.any(), f"{key}: {int(decision_diff.sum())} decisions differ from the oracle's\n" + show(decision_diff)
        used = answered & ~decide & acc_ref
        rel = np.abs(out["t"][used] - t_ref[used]) / np.abs(t_ref[used])
        worst_rel = float(rel.max()) if rel.size else 0.0
        far = np.zeros(len(rays), bool)
        far[np.flatnonzero(used)[rel > CUB_TOL]] = True
        assert not far.any(), f"{key}: {int(far.sum())} accepted roots beyond CUB_TOL of the oracle's (worst {worst_rel:.3g})\n" + show(far)
    # 2. the dense path (every record, refused or not) is the oracle's under the device's libm, bit for bit, and so is the branch
    dense_diff = t_dl.view(np.uint64) != out["t_dense"].view(np.uint64)
    assert not dense_diff.any(), f"{key}: {int(dense_diff.sum())} dense roots not bitwise the device-libm oracle's\n" + show(dense_diff)
    assert np.array_equal(out["t"][refused].view(np.uint64), out["t_dense"][refused].view(np.uint64)), show(refused & (out["t"] != out["t_dense"]))
    br_ok = np.zeros(len(rays), bool)
    for dev, orc in BRANCH_MAP.items():
        br_ok |= (out["branch"] == dev) & np.isin(br_dl, orc)
    assert br_ok.all(), f"{key}: {int((~br_ok).sum())} dense branches differ\n" + show(~br_ok)

    prim = where["kind"] == 0
    res = dict(key=key, tests=len(rays), by_kind=[int((where["kind"] == k).sum()) for k in range(3)], refused=int(refused.sum()),
               refused_by_kind=[int((refused & (where["kind"] == k)).sum()) for k in range(3)], decision_diff=int(decision_diff.sum()),
               dense_diff=int(dense_diff.sum()), worst_rel=worst_rel, libm=libm, rounds=rounds, max_refused=max_refused, psc=psc, cam=cam, osc=osc,
               primary=int(prim.sum()), refused_primary=int((refused & prim).sum()), n_mirror_bounces=int((where["kind"] == 2).sum()))
    print(f"{key}: tests {res['tests']} (primary / shadow / bounce {res['by_kind']}), refused {res['refused']} {res['refused_by_kind']}, "
          f"decision diffs 0, dense bitwise mismatches 0, worst answered root {worst_rel:.2e}, libm rounds {rounds}")
    _MEMO[key] = res
    return res


def _kernel_counts(pkg, psc, cam):
    r = pkg.Renderer(psc, device=0, flags=pkg.RT_FLAG_COUNT)
    r.update(cam)
    d = r.counters_detail()
    r.cleanup_update()
    return d


REPO = ["clebsch", "cayley", "cubic", "dingdong", "monkey_saddle", "cayley_moved", "many_cubic"]


@pytest.mark.parametrize("key", REPO)
def test_degree3_rays_on_the_device(pkg, oracle, lab, key):
    res = _run(pkg, oracle, lab, key)
    # 3. refusal shares: the CPU lab's bounds; cayley from the origin (F(0) = 0: a double root at t = 0 on every primary ray) wholesale
    if res["max_refused"] is not None:
        assert res["refused_primary"] <= res["max_refused"] * res["primary"], res
    if key == "cayley":
        assert res["refused_primary"] == res["primary"]
    if key == "many_cubic":
        assert res["n_mirror_bounces"] > 0 and len(res["osc"].coefs) > 4   # (more degree-3 objects than RT_CUB_AT_MAX, bounce rays)
    # ... and where the kernel makes exactly the lab's degree-3 tests, it refuses exactly the lab's
    d = _kernel_counts(pkg, res["psc"], res["cam"])
    if d["executed_by_class"]["cubic"] == res["tests"]:
        assert d["cubic_refused"] == res["refused"], (d["cubic_refused"], res["refused"])
    print(f"{key}: kernel degree-3 tests {d['executed_by_class']['cubic']}, refused {d['cubic_refused']} (lab {res['tests']}, {res['refused']})")


def test_degree3_rays_of_random_scenes_on_the_device(pkg, oracle, lab):
    """The 12 scenes of cubic_guard_lab.fuzz_scene (test_cubic_guard.py): per-ray assertions per scene, the CPU lab's bound on refusals."""
    tests = refused = 0
    for seed in range(12):
        res = _run(pkg, oracle, lab, f"fuzz_{seed}")
        tests += res["by_kind"][0] + res["by_kind"][1]
        refused += res["refused_by_kind"][0] + res["refused_by_kind"][1]
    assert tests > 100000 and refused < 0.1 * tests


def _cases():
    """test_cubic_guard.py::test_guard_on_hand_made_polynomials, as (t3, t2, t1, t0, max_t, decide, m, what the CPU test requires:
    True answered, False refused, None either)."""
    eps = 1e-7
    c = [(1.0, -6.0, 11.0, -6.0, 1e6, False, 1e-15, True), (1.0, -4.0, 1.0, 6.0, 1e6, False, 1e-15, True), (1.0, -1.0, 3.0, -10.0, 1e6, False, 1e-15, True),
         (1.0, 1.0, 3.0, 10.0, 1e6, False, 1e-15, True), (1.0, -6.0, 11.0, -6.0, 1e6, True, 1e-15, True), (1.0, -6.0, 11.0, -6.0, 1.5, True, 1e-15, True),
         (1.0, 6.0, 11.0, 6.0, 1e6, True, 1e-15, True), (1.0, -5.0, 7.0, -3.0, 1e6, False, 1e-15, False),
         (1.0, -(eps + 5.0), 6.0 + 5.0 * eps, -6.0 * eps, 1e6, False, 1e-15, False), (1.0, -(0.5 + 5.0), 6.0 + 2.5, -3.0, 1e6, False, 1e-15, True),
         (1.5e-7, 1.0, -3.0, 2.0, 1e6, False, 1e-15, False), (0.0, 1.0, -3.0, 2.0, 1e6, False, 1e-15, True), (0.0, 1.0, 0.0, 1.0, 1e6, False, 1e-15, True),
         (0.0, 0.0, 2.0, -1.0, 1e6, False, 1e-15, True), (0.0, 0.0, 0.0, 1.0, 1e6, False, 1e-15, True),
         (1.0, -6.0, 11.0, -6.0, 1e6, False, 1e-6, False), (1.0, -6.0, 11.0, -6.0, 1e6, True, 1e-6, True), (1.0, -6.0, 11.0, -6.0, 1e6, True, 1e-3, False)]
    for bad in (float("nan"), float("inf")):
        c += [(bad, 1.0, 1.0, 1.0, 1e6, False, 1e-15, False), (1.0, bad, 1.0, 1.0, 1e6, False, 1e-15, False), (1.0, 1.0, 1.0, bad, 1e6, False, 1e-15, False)]
    rng = np.random.default_rng(7)
    for _ in range(2000):
        r = sorted(rng.uniform(-5, 5, 3))
        if min(r[1] - r[0], r[2] - r[1]) < 0.2 or min(abs(x - 1e-7) for x in r) < 0.05:
            continue
        a = float(rng.uniform(0.5, 2.0)) * (1 if rng.random() < 0.5 else -1)
        c.append((a, -a * sum(r), a * (r[0] * r[1] + r[0] * r[2] + r[1] * r[2]), -a * r[0] * r[1] * r[2], 1e6, False, 1e-15, None))
    return c


def test_guard_on_hand_made_polynomials_on_the_device(lab):
    """4. cubic_guarded by itself on the device: whatever it answers is the reference's solver's decision (and root, to CUB_TOL); what the
    CPU test requires refused is refused."""
    cpu = D.CPU.build()
    import ctypes as C
    cpu.lab_reference.restype = C.c_double
    cpu.lab_reference.argtypes = [C.c_double] * 4
    cases = _cases()
    arr = np.array([(t3, t2, t1, t0, m, m, m, m, mt, float(dec)) for (t3, t2, t1, t0, mt, dec, m, _) in cases])
    ok, t = D.device_guard(lab, arr)
    answered = 0
    for i, (t3, t2, t1, t0, mt, dec, m, want) in enumerate(cases):
        if want is not None:
            assert bool(ok[i]) == want, (cases[i], bool(ok[i]), t[i])
        if not ok[i]:
            continue
        answered += want is None
        ref = cpu.lab_reference(t3, t2, t1, t0)
        if dec:
            assert (EPS < t[i] < mt) == (EPS < ref < mt), (cases[i], t[i], ref)
        else:
            assert (EPS <= t[i] < mt) == (EPS <= ref < mt), (cases[i], t[i], ref)
            assert abs(t[i] - ref) <= CUB_TOL * max(1.0, abs(ref)), (cases[i], t[i], ref)
    assert answered > 1000


def test_device_special_functions_against_mpmath(pkg, oracle, lab):
    """5. The device's cbrt / acos / cos on every argument the scenes above pass to them (their dense paths under the device libm),
    against mpmath at 60 digits correctly rounded: within ULP_BOUND.  NaN arguments (acos just beyond +-1) give NaN."""
    args = {f: [] for f in D.FN}
    for key in REPO + [f"fuzz_{s}" for s in range(12)]:
        res = _run(pkg, oracle, lab, key)
        for f in D.FN:
            args[f].append(res["libm"].args(f))
    for f in D.FN:
        x = np.unique(np.concatenate(args[f]).view(np.uint64)).view(np.float64)
        y = D.device_libm(lab, f, x)
        err = D.ulp_error(f, x, y)
        worst = int(np.argmax(err))
        print(f"{f}: {len(x)} distinct arguments, worst {err[worst]:.3f} ulp at {x[worst]!r} (device {y[worst]!r})")
        assert err.max() <= ULP_BOUND[f], (f, x[worst], y[worst], err[worst])


# ---- the same lab in the RT_FLAG_FAST variant's flags (-ffp-contract=fast) ------------------------------------------------------------------
FAST_KEYS = ["clebsch", "dingdong", "many_cubic"]
FAST_DENSE_SAMPLE = 600   # refused records per scene whose contracted dense root is held to exact arithmetic (some 2 ms each on the host)


@pytest.mark.parametrize("key", FAST_KEYS)
def test_degree3_rays_on_the_device_in_the_fast_variants_flags(pkg, oracle, lab, key):
    """cubic_at, cubic_coefs, cubic_guarded and the dense fall-back as the compiler contracts them for the FAST kernels.  Where the guard
    answers, the strict run's assertions: no decision differs from the oracle's, accepted roots within CUB_TOL.  Where it refuses, the
    contracted dense root is held to exact arithmetic within B3 on decided pairs (tests/tools/fast_ref.py) -- the bit-for-bit comparison
    under the device's libm stays with the strict build.  The refused shares of both builds are printed side by side."""
    import fast_ref as F
    strict = _run(pkg, oracle, lab, key)
    osc, cam, _, _ = _scene(pkg, oracle, key)
    rays, where = D.enumerate_rays(osc, cam)
    out = D.device_rays(D.lib(pkg, "fast"), osc.coefs, rays)
    out_strict = D.device_rays(lab, osc.coefs, rays)
    t_ref, _, _ = D.oracle_rays(osc, rays)
    refused = out["refused"] != 0
    answered = ~refused
    decide = (rays["flags"] & D.LAB_DECIDE) != 0
    max_t = rays["max_t"]
    differ = int((out["t_dense"].view(np.uint64) != out_strict["t_dense"].view(np.uint64)).sum())
    assert differ > 0, "this build of the lab is not contracted: it says nothing about the FAST variant"
    assert np.array_equal(out["guard_ok"] != 0, answered)
    with np.errstate(invalid="ignore"):
        acc = np.where(decide, (out["t"] > EPS) & (out["t"] < max_t), (out["t"] >= EPS) & (out["t"] < max_t))
        acc_ref = np.where(decide, (t_ref > EPS) & (t_ref < max_t), (t_ref >= EPS) & (t_ref < max_t))
        decision_diff = answered & (acc != acc_ref)
        assert not decision_diff.any(), f"{key}: {int(decision_diff.sum())} decisions differ from the oracle's; first record {int(np.flatnonzero(decision_diff)[0])}"
        used = answered & ~decide & acc_ref
        rel = np.abs(out["t"][used] - t_ref[used]) / np.abs(t_ref[used])
        worst_rel = float(rel.max()) if rel.size else 0.0
        assert worst_rel <= CUB_TOL, f"{key}: an accepted root is {worst_rel:.3g} relative off the oracle's"
    # the contracted dense path where the guard refused, against exact arithmetic
    coefs = np.ascontiguousarray(osc.coefs, dtype=np.float64).reshape(-1, 20)
    idx = np.flatnonzero(refused)
    idx = idx[:: max(1, len(idx) // FAST_DENSE_SAMPLE)]
    judged, worst_rho = 0, 0.0
    import mpmath
    for k in np.unique(rays["obj"][idx]).tolist():
        sel = idx[rays["obj"][idx] == k]
        pr = F.pairs(coefs[k:k + 1], rays["o"][sel], rays["d"][sel])
        for j, i in enumerate(sel.tolist()):
            if not pr["ok"][j, 0]:
                continue
            te = F.exact_t(coefs[k], rays["o"][i], rays["d"][i])
            rho = float(abs(mpmath.mpf(float(out["t_dense"][i])) - te) / mpmath.mpf(float(pr["B"][j, 0])))
            judged, worst_rho = judged + 1, max(worst_rho, rho)
            assert rho <= 1.0, (f"{key}: record {i} (object {k}, o {rays['o'][i].tolist()}, d {rays['d'][i].tolist()}): contracted dense t {float(out['t_dense'][i])!r}, "
                                f"exact {mpmath.nstr(te, 25)}, B3 {pr['B'][j, 0]:.3e}, rho {rho:.3g}")
    assert np.array_equal(out["t"][refused].view(np.uint64), out["t_dense"][refused].view(np.uint64))
    print(f"{key}: tests {len(rays)}; refused strict {strict['refused']} ({100.0 * strict['refused'] / len(rays):.3f} %), FAST flags {int(refused.sum())} "
          f"({100.0 * refused.sum() / len(rays):.3f} %); dense roots that differ in bits between the builds {differ}; decision diffs 0, worst answered root "
          f"{worst_rel:.2e}; {judged} of {len(idx)} sampled refused records decided, worst rho {worst_rho:.3g}")
    assert judged > 0 or not len(idx)
