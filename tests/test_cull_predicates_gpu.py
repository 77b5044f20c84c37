"""Device leg of tests/test_cull_predicates.py: tests/tools/cull_device_lab.hip evaluates the records the host lab produced -- grazing cases,
records of real frames and the hand-made margin pins -- on the GPU, one record per lane, built with the strict kernels' flags.  Every
verdict must equal the host build's and every field of cull_record must be bit-equal: the device sqrt of sphere_in_cone and the absence of
contraction are what this checks.  The pins carry their expected verdicts, so a changed margin fails here as well."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

N = 100000     # grazing cases per family


@pytest.fixture(scope="module")
def records():
    import cull_lab as L
    rec = {k: [] for k in L.KINDS}
    for kind, r in (("cone", L.graze_primary(N, 0, 0)[0]), ("pyr", L.graze_primary(N, 0, 1)[0]), ("sh", L.graze_shadow(N, 0, False)[0]),
                    ("sh", L.graze_shadow(N, 0, True)[0])):
        rec[kind].append(r.get(kind)[0])
    for name, s, cam, stride in L.frame_sources(n_fuzz=6):
        r = L.frame(s, cam, stride=max(stride, 7))
        for k in L.KINDS:
            rec[k].append(r.get(k)[0][:60000])
    for seed in range(8):     # needs_solve sees general quadrics only: every ray of mixed-class frames
        rec["gq"].append(L.frame(L.mixed_scene(seed), None, stride=1).get("gq")[0])
    us, gq = L.hand_made_solve_records()
    rec["us"].append(us)
    rec["gq"].append(gq)
    rec["sh"].append(np.array([p[0] for p in L.margin_pins()]))
    return {k: np.concatenate(v) for k, v in rec.items()}


def test_device_verdicts_equal_the_host_build(pkg, records):
    import cull_device_lab as D
    import cull_lab as L
    dev = D.lib(pkg, "strict")
    for kind in L.KINDS:
        rec = records[kind]
        assert len(rec) >= 100000, (kind, len(rec))
        host = L.evaluate(kind, rec)
        got = D.evaluate(dev, kind, rec)
        if kind == "sh":
            (host, host_crec), (got, got_crec) = host, got
            same = host_crec.view(np.uint64) == got_crec.view(np.uint64)
            print(f"\ncull_record: {len(rec)} records, {int((~same).sum())} fields differ in their bits")
            assert same.all(), rec[np.flatnonzero(~same.all(axis=1))[:2]]
        n = int((host != got).sum())
        print(f"\n{kind}: {len(rec)} records, {n} device verdicts differ from the host build's")
        assert n == 0, rec[np.flatnonzero(host != got)[:2]]


def test_documented_margins_on_the_device(pkg):
    import cull_device_lab as D
    import cull_lab as L
    dev = D.lib(pkg, "strict")
    for rec, mask, want, what in L.margin_pins():
        v, _ = D.evaluate(dev, "sh", rec)
        assert v[0] & mask == want, (what, int(v[0]))


def test_fast_variant_differs_only_inside_the_band(pkg, records):
    """The same source built as the FAST variant is built (-DRT_FAST=1 -ffp-contract=fast): contraction may move a verdict, but only within
    the margin.  Prints the number of differing verdicts per kind; none may differ where the exact clearance (mpmath, cull_lab.exact_excess)
    is more than 1e-3 of the predicate's distance scale from zero -- a thousand documented margins."""
    import cull_device_lab as D
    import cull_lab as L
    dev = D.lib(pkg, "fast")
    for kind in L.KINDS:
        rec = records[kind]
        host = L.evaluate(kind, rec)
        got = D.evaluate(dev, kind, rec)
        if kind == "sh":
            host, got = host[0], got[0]
        diff = np.flatnonzero(host != got)
        print(f"\n{kind}: {len(rec)} records, {len(diff)} FAST verdicts differ from the strict host build's")
        if kind in ("us", "gq"):
            continue    # (no geometric clearance to speak of: reported only)
        for i in diff[:400]:
            bits = int(host[i] ^ got[i])
            kinds = [kind] if kind != "sh" else (["sh_sph"] if rec[i, 24] != 0 else ((["sh_dir"] if bits & 3 else []) + (["sh_box"] if bits & 12 else [])))
            for xk in kinds:
                x = L.exact_excess(xk, rec[i])
                assert x is not None and abs(x[0]) <= 1e-3 * x[1], (xk, list(rec[i]), x)


# ---- grazing scenes through the product kernels -------------------------------------------------------------------------------------
def _scene(pkg, spec):
    s = pkg.Scene.new(spec["w"], spec["h"], spec["fov"], 0, (0.1, 0.2, 0.3))
    for c, r, col in spec["spheres"]:
        s.add_object(pkg.surface_make("sphere", list(c), [r]), col, 0.0)
    for kind, v, col, intensity in spec["lights"]:
        s.add_light(kind, list(v), col, intensity)
    return s


@pytest.fixture(scope="module")
def graze_specs():
    import cull_lab as L
    kept, n = L.graze_scenes()
    assert 2 * len(kept) >= n and len(kept) >= 24
    return kept


@pytest.mark.parametrize("i", range(24))
def test_grazing_scene_through_every_kernel(pkg, oracle, graze_specs, monkeypatch, i):
    """A scene with a sphere set tangent to a block's cone, a tile's pyramid or a chunk's shadow volume (both light kinds; the chunks on the
    near sphere's silhouette span it and the far one): default == RT_FLAG_NOCULL == RT_FLAG_SIMPLE == oracle over three frames, forced lean ==
    RT_FLAG_NOLEAN, the G-buffer planes == gbuffer_ref, one adaptive-supersampling frame == its composition from the oracle's frames, and the
    shadow-phase culling really ran."""
    import gbuffer_ref
    from test_gpu_parity import _check_against_oracle, oracle_from, render_desc
    from test_ssaa_adaptive_fuzz_gpu import ada, adaptive, identical
    spec = graze_specs[i]
    sc = _scene(pkg, spec)
    got = _check_against_oracle(pkg, oracle, sc)
    monkeypatch.setenv("MI355RT_LEAN", "always")
    lean = render_desc(pkg, sc)
    assert np.array_equal(lean, render_desc(pkg, sc, flags=pkg.RT_FLAG_NOLEAN)), "lean and general instantiation disagree"
    assert np.array_equal(lean, got), "forced lean and the default schedule disagree"
    monkeypatch.delenv("MI355RT_LEAN")
    r = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_COUNT)
    r.update()
    d = r.counters_detail()
    r.cleanup_update()
    assert d["cull_by_kind"]["shadow_directional"] > 0 and d["cull_by_kind"]["primary"] > 0
    osc = oracle_from(pkg, oracle, sc)
    r = pkg.Renderer(sc, device=0)
    o, t, n, _ = r.gbuffer(None)
    r.cleanup_update()
    ref = gbuffer_ref.compose(osc, None)
    assert np.array_equal(o.cpu().numpy(), ref["object"])
    assert np.array_equal(t.cpu().numpy().view(np.uint64), ref["t"].view(np.uint64))
    assert np.array_equal(n.cpu().numpy().view(np.uint32), ref["normal"].view(np.uint32))
    if i % 4 == 0 or spec["kind"].startswith("shadow"):
        tau = 1.0 / 32.0
        p, s = osc.render(nthreads=4), osc.with_size(2 * osc.width, 2 * osc.height).render(nthreads=8)
        frame, _, _ = adaptive(pkg, sc, None, 2, tau)
        assert identical(frame, ada.compose(p, s, 2, tau)), "adaptive supersampling frame"
