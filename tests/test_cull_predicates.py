"""The work-removal predicates of rt_wavefront_math.hpp, held one by one to the oracle on the CPU (tests/tools/cull_lab.py: the kernels'
own header compiled for the host).  Every test asserts ZERO unsound verdicts: a predicate that says "skip" while the oracle accepts some
ray of the set the predicate speaks about.  Two sources of input: every block, tile and chunk of real frames, and the grazing generator
(a sphere tangent to a ray of the set at relative clearances +-1e-1 ... +-1e-15).  The non-vacuity tests check the inputs on the
reference side alone, and that each culling predicate does cull where exact geometry (mpmath, 50 digits) puts the sphere beyond a
thousand times its documented margin.  Long runs: python tests/tools/cull_lab.py [n] [first_seed]."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cull_lab as L  # noqa: E402

N_GRAZE = 110000      # cases per family; the generators drop a few (singular cameras, directions with |d|^2 <= EPS): at least 1e5 verdicts must remain


@pytest.fixture(scope="module")
def frames():
    t = L.Tally()
    for name, s, cam, stride in L.frame_sources(n_fuzz=30):
        t.add(L.frame(s, cam, stride=stride))
    print("\nreal frames:\n" + t.table())
    return t


@pytest.fixture(scope="module")
def grazing():
    out = {}
    for name, fn in (("cone", lambda: L.graze_primary(N_GRAZE, 0, 0)), ("pyr", lambda: L.graze_primary(N_GRAZE, 0, 1)),
                     ("dir", lambda: L.graze_shadow(N_GRAZE, 0, False)), ("sph", lambda: L.graze_shadow(N_GRAZE, 0, True))):
        out[name] = fn()
    t = L.Tally()
    for r, _, _ in out.values():
        t.add(r)
    print("\ngrazing generator:\n" + t.table())
    return out, t


SOLVE = ("us_needs_solve", "needs_solve")
PRIMARY = ("sphere_in_cone", "sphere_in_pyramid")
SHADOW = ("sphere_relevant<false>", "sphere_relevant<true>", "crec_relevant", "crec_in_box_shadow")


def _sound(t, names):
    for p in names:
        assert t.unsound[p] == 0, (p, t.unsound[p], [list(r) for n, r in t.examples if n == p][:2])


def test_solve_skipping_on_real_rays(frames):
    """us_needs_solve false => the oracle's root passes neither t >= EPS nor t > EPS; needs_solve false => the oracle returns -1."""
    _sound(frames, SOLVE)
    assert frames.n["us_needs_solve"] >= 100000 and frames.n["needs_solve"] >= 100000
    assert frames.culled["us_needs_solve"] > 0 and frames.culled["needs_solve"] > 0


def test_solve_skipping_on_hand_made_coefficients():
    """t1, t0 tiny (denormals included) and huge (1e300), discriminants one ulp either side of 0, t2 either side of EPS."""
    us, gq = L.hand_made_solve_records()
    v_us, v_gq = L.evaluate("us", us), L.evaluate("gq", gq)
    t = us[:, 4]
    assert len(us) > 5000 and (v_us == 0).sum() > 1000 and (v_gq == 0).sum() > 1000
    # Named case, found here: t1 = +-1e300 with t2, t0 > 0.  t1 * t1 overflows, the reference's discriminant and root are +inf, which passes
    # "t >= EPS" alone -- but no acceptance rule: both also ask t < MAX_T (or max_t <= MAX_T).  The predicate's "both roots <= 0" is the exact
    # answer.  So the lower bound is asserted wherever the oracle's root is finite, and a non-finite root only where |t1| > 1e154.
    bad = (v_us == 0) & ((t >= L.EPS) | (t > L.EPS)) & np.isfinite(t)
    assert not bad.any(), us[bad][:3]
    over = (v_us == 0) & ~np.isfinite(t)
    assert (np.abs(us[over, 2]) > 1e154).all() and not ((t[over] >= L.EPS) & (t[over] < L.MAX_T)).any()
    bad = (v_gq == 0) & (gq[:, 3] != -1.0)
    assert not bad.any(), gq[bad][:3]
    # named cases: a double root (discriminant exactly 0) is solved; one ulp below, the oracle returns -1 and so may the predicate
    assert L.evaluate("us", np.array([[1.0, 4.0, -2.0, 1.0, 0.0]]))[0] == 1
    assert L.evaluate("gq", np.array([[1.0, -2.0, 1.0, 0.0]]))[0] == 1
    assert L.evaluate("gq", np.array([[1.0, -2.0, np.nextafter(1.0, 2.0), 0.0]]))[0] == 0
    # t2 at EPS takes the linear branch: |t1| decides
    assert L.evaluate("gq", np.array([[1e-7, 0.0, 1.0, 0.0]]))[0] == 0 and L.evaluate("gq", np.array([[1e-7, 1.0, 1.0, 0.0]]))[0] == 1
    assert L.evaluate("us", np.array([[0.0, 4e-7, 1e-7, 1.0, 0.0]]))[0] == 0 and L.evaluate("us", np.array([[0.0, 4e-7, 1.1e-7, 1.0, 0.0]]))[0] == 1


def test_primary_cone_and_tile_pyramid(frames, grazing):
    """sphere_in_cone false => no primary ray of the 8 x 8 block accepts the sphere; sphere_in_pyramid false => none of the 16 x 16 tile."""
    _, g = grazing
    _sound(frames, PRIMARY)
    _sound(g, PRIMARY)


def test_corner_claim(frames, grazing):
    """Over all 64 lanes of a block, image-edge blocks included: dot(axis, d) >= cos_t (1 - 1e-9), cos_t taken from lanes 0, 7, 56, 63."""
    _, g = grazing
    for t in (frames, g):
        assert t.c["corner_n"] >= 100000 and t.c["corner_bad"] == 0, t.c


def test_shadow_phase(frames, grazing):
    """A false verdict of sphere_relevant<false|true>, crec_relevant or crec_in_box_shadow => the sphere blocks no shadow ray of the chunk
    towards that light (ball and box formed as phase A', the lean block and rt_adaptive.hip form them)."""
    _, g = grazing
    _sound(frames, SHADOW)
    _sound(g, SHADOW)


def test_shadow_phase_equalities(frames, grazing):
    """crec_relevant(cull_record(e, ball)) == sphere_relevant<false>(e, ball, light); the two crec_in_box_shadow overloads agree; a
    non-finite radius is always "test it": zero differing verdicts each."""
    _, g = grazing
    for t in (frames, g):
        assert (t.crec_differs, t.box_overloads_differ, t.nonfinite_culled) == (0, 0, 0)
    # infinite and NaN radii by hand, on grazing records
    rec, _ = grazing[0]["dir"][0].get("sh")
    rec2, _ = grazing[0]["sph"][0].get("sh")
    for r, want in ((rec[:2000].copy(), 15), (rec2[:2000].copy(), 1)):
        for bad_r, inv in ((np.inf, 0.0), (np.nan, 0.0), (np.nan, np.nan)):
            r[:, 4], r[:, 5] = bad_r, inv
            v, _ = L.evaluate("sh", r)
            assert (v == want).all()
    for kind, col in (("cone", 3), ("pyr", 3)):
        r = grazing[0][kind][0].get(kind)[0][:2000].copy()
        for bad_r in (np.inf, np.nan):
            r[:, col], r[:, col + 1] = bad_r, 0.0
            assert (L.evaluate(kind, r) == 1).all()


def test_documented_margins_by_hand():
    """Hand-made records either side of the 1e-6 margin of cull_record / sphere_relevant and of the (1 + 1e-9) factor of crec_in_box_shadow."""
    for rec, mask, want, what in L.margin_pins():
        v, _ = L.evaluate("sh", rec)
        assert v[0] & mask == want, (what, int(v[0]))


def test_own_sphere_window(frames):
    """own_lo < us_t0(s, biased origin) < own_hi => the oracle's shadow test of that ray against s does not block (directional lights with
    |d|^2 > EPS in front of the surface)."""
    c = frames.c
    assert c["own_n"] >= 100000 and c["own_skip"] > c["own_n"] // 2 and c["own_bad"] == 0, c


def test_backface_skips(frames):
    """Where the kernels skip a light behind the surface (backface_exact; flag 8 with q < -1e-9 mag), accumulating the oracle's term changes no
    bit of the sum.  The term is +0 in every channel -- except under a negative (raw-descriptor) colour, where finite * 0 is -0, and
    x + -0 == x for every x the sum can hold; those are counted apart, and scenes with colours in [0, 1] must give none."""
    c = frames.c
    assert c["bf_n"] >= 100000 and c["bf_skip"] >= 10000 and c["bf_bad"] == 0, c
    t = L.Tally()
    for name, s, cam, stride in L.frame_sources(n_fuzz=4):
        if not name.startswith("raw descriptor"):
            t.add(L.frame(s, cam, stride=16))
    assert t.c["bf_skip"] > 1000 and t.c["bf_bad"] == 0 and t.c["bf_negzero"] == 0, t.c


def test_inputs_are_not_vacuous(frames, grazing):
    """On the reference side alone: each grazing set has at least a quarter "no ray accepts" and a quarter "some ray accepts", and every
    predicate is evaluated at least 1e5 times in each source."""
    out, g = grazing
    for name, kind in (("cone", "cone"), ("pyr", "pyr"), ("dir", "sh"), ("sph", "sh")):
        _, truth = out[name][0].get(kind)
        frac = float(truth.mean())
        assert len(truth) >= 100000 and 0.25 <= frac <= 0.75, (name, len(truth), frac)
    for p in PRIMARY + SHADOW:
        assert g.n[p] >= 100000, (p, g.n[p])
    for p in SOLVE + PRIMARY + SHADOW:
        assert frames.n[p] >= 100000, (p, frames.n[p])


@pytest.mark.parametrize("name,kind,xkind,bit", [("cone", "cone", "cone", 1), ("pyr", "pyr", "pyr", 1), ("dir", "sh", "sh_dir", 3), ("sph", "sh", "sh_sph", 1), ("dir", "sh", "sh_box", 12)])
def test_predicates_cull_beyond_a_thousand_margins(grazing, name, kind, xkind, bit):
    """A predicate that always answered "test it" would pass every test above.  Exact distance of the centre from the predicate's own bounding
    volume (widened cone, planes of the pyramid, ball-swept line / segment, the box's shadow along the light) with mpmath at 50 digits: wherever it exceeds r by more than 1e-3
    of the predicate's distance scale -- a thousand times the documented margin -- the predicate must cull."""
    rec = [grazing[0][name][0].get(kind)[0]]
    for fname, sc, cam, stride in L.frame_sources(n_fuzz=3):      # the grazing set hugs the boundary: real frames supply the far spheres
        if fname.startswith("large"):
            continue
        r = L.frame(sc, cam, stride=64).get(kind)[0]
        rec.append(r[r[:, 24] == (1.0 if name == "sph" else 0.0)] if kind == "sh" else r)
    rec = np.concatenate(rec)
    v = L.evaluate(kind, rec)
    v = v[0] if kind == "sh" else v
    kept, beyond = L.must_cull_failures(xkind, rec, (v & bit) == bit, sample=1500)
    print(f"\n{name}: {beyond} of the sample beyond the band, {kept} of them kept")
    assert beyond >= 100 and kept == 0, (beyond, kept)


def test_own_window_and_backface_thresholds_by_hand():
    """Hand-made hits at the ends of the two skips.  A sphere of radius r lit from straight above by a directional light: hits whose normal makes
    (float) dot(n, l) the smallest positive floats, zero and the first negative ones (backface_exact's compare), and -- through the lab's
    frame walk on a scene built around them -- the own-sphere window on tiny and huge spheres, where own_lo and own_hi lie closest to the true
    t0 = 0.02 r + 1e-4.  Point light: q either side of -1e-9 mag."""
    for r in (1e-3, 1.0, 50.0):      # t0 of a hit is 2e-2 r + 1e-4: inside (own_lo, own_hi) = (~1e-10 (r^2 + 1), (r + 1)^2) for each of these
        s = L.O.Scene(64, 48, 40.0, 0, (0.1, 0.2, 0.3))
        s.add_object(L.sphere((0.0, 0.0, 4.0 * r), r), (0.8, 0.7, 0.6), 0.0)
        L.add_light(s, "directional", (0.0, -1.0, 0.0), (1, 1, 1), 1.0)       # grazing along the sphere's equator: dot(n, l) changes sign there
        L.add_light(s, "directional", (0.0, 0.0, 1.0), (1, 1, 1), 1.0)        # from behind the camera: in front of every hit
        L.add_light(s, "spherical", (0.0, r, 4.0 * r), (1, 1, 1), 50.0)  # ON the surface's pole: q changes sign around it
        L.add_light(s, "spherical", (0.0, 0.0, 4.0 * r), (1, 1, 1), 50.0)  # at the centre: behind every hit
        c = L.frame(s, None, stride=16).counters()
        assert c["own_n"] > 0 and c["own_skip"] > 0 and c["own_bad"] == 0, (r, c)
        assert c["bf_skip"] > 0 and c["bf_bad"] == 0 and c["bf_negzero"] == 0, (r, c)


def test_grazing_scenes_are_decided_by_their_tangent_spheres():
    """The whole scenes tests/test_cull_predicates_gpu.py sends through the product kernels: with the oracle alone, in at least half of them a
    tangent sphere is the nearest hit or the sole blocker of some pixel (the others are dropped there), every kind is among the kept ones, and
    each has at least four cullable spheres and no other object (both instantiations render it)."""
    kept, n = L.graze_scenes()
    assert n >= 24 and 2 * len(kept) >= n, (len(kept), n)
    assert {s["kind"] for s in kept} == set(L.GRAZE_KINDS)
    assert all(len(s["spheres"]) >= s["n_base"] + 6 for s in kept)
