"""The device work counters (RT_FLAG_COUNT: rt_get_counters / rt_get_counters_detail) of the plain path against the oracle's, on the
random and edge scenes the frames are held to.  bench.py's Mrays/s numerator and its flop accounting are computed from them, and
they come from instantiations of their own (COUNT = true) that the product build never runs.

1. Degree <= 2: primary_rays, shadow_rays, reflect_rays, tests and hits equal the oracle's counters (hits: its `normals`) as
   integers, after each of three frames of one context (index order, then launch-order lists, half tiles in the second), and the
   counting frame is the product frame bit for bit -- in every kernel variant, through camera cuts and random walks, and per band.
2. The detail block: identities between its words, relations to the oracle's counters, determinism, and that culling and the lean
   instantiation only remove executed work.
3. Degree 3: the same against the oracle under the device's cbrt / acos / cos (tests/tools/cubic_device_lab.py), and the solver
   branches.

Nothing in sections 1 and 2 has a tolerance.  The relations of section 2 are asserted as strongly as rt_wavefront.hip promises them;
check_detail's docstring names the lines."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_cubic_gpu import many_cubic_objects_and_mirrors
from test_gpu_parity import CUBIC, camera_cut_sequence, general_camera_case, oracle_from, random_cubic_scene, random_scene, random_walk
from test_ssaa_adaptive_fuzz_gpu import build as build_shared, identical

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cubic_device_lab as D  # noqa: E402  (the oracle under the device's cbrt / acos / cos)

pytestmark = pytest.mark.gpu

COUNTED = ("primary_rays", "shadow_rays", "reflect_rays", "tests", "hits")
WG = 256   # rt_wavefront.hip: __launch_bounds__(256); cnt.primary_traced() runs on every lane of a tracing workgroup (the lean path: on
           # every lane of each of its four waves), half tiles included -- both workgroups of a split tile form 256 rays


def _pkg():
    import __graft_entry__ as graft
    return graft.load_package()


def _oracle():
    import __graft_entry__ as graft
    return graft.load_oracle()


# ---- scenes ------------------------------------------------------------------------------------------------------------------
# ("random", seed, spheres, lights, plane, mirrors, w, h, pose) / ("mixed", seed, w, h) / ("fuzz", seed) / ("edge", name): the keys of
# test_ssaa_adaptive_fuzz_gpu.build; ("shear", seed): test_general_camera_matrices_on_sphere_fields' cases, frames capped at 200 x 150
RANDOM = [  # two thirds under a moved camera (pose >= 0), every sphere count with and without the plane / mirrors, 1 .. 9 lights
    ("random", 8101, 3, 1, True, False, 160, 120, -1), ("random", 8102, 3, 6, False, True, 120, 90, 1),
    ("random", 8103, 8, 2, False, False, 160, 120, 2), ("random", 8104, 8, 7, True, True, 200, 150, -1),
    ("random", 8105, 20, 3, True, True, 160, 120, 3), ("random", 8106, 20, 8, False, False, 177, 131, 4),
    ("random", 8107, 40, 4, False, True, 160, 120, -1), ("random", 8108, 40, 9, True, False, 144, 100, 5),
    ("random", 8109, 70, 5, True, True, 128, 96, 6), ("random", 8110, 70, 1, False, False, 160, 120, -1),
    ("random", 8111, 130, 2, False, True, 128, 96, 7), ("random", 8112, 130, 5, True, False, 96, 72, 8),
    ("random", 8113, 200, 3, True, True, 96, 72, -1), ("random", 8114, 200, 4, False, False, 128, 96, 9),
    ("random", 8115, 12, 5, False, False, 200, 150, 2),
    ("random", 8116, 70, 40, True, True, 96, 64, 1),   # 40 lights: two shadow words per hit
]
MIXED = [("mixed", seed, 128, 96) for seed in range(24)]
FUZZ = [("fuzz", seed) for seed in [158, 534] + list(range(2000, 2040))]
EDGE = [("edge", n) for n in ("no_objects", "no_lights", "camera_inside_sphere", "light_inside_sphere")]
SHEAR = [("shear", seed) for seed in range(6)]
MIRRORS = [("edge", f"two_mirrors_depth_{d}") for d in (0, 1, 5)]
SCENES = RANDOM + MIXED + FUZZ + EDGE + SHEAR + MIRRORS


def key_id(key):
    if key[0] == "random":
        _, seed, n, lights, plane, mirrors, w, h, p = key
        return f"random{seed}-n{n}-l{lights}" + ("-plane" if plane else "") + ("-mirrors" if mirrors else "") + (f"-pose{p}" if p >= 0 else "")
    return "-".join(str(v) for v in key[:2])


@functools.lru_cache(maxsize=None)
def build(key):
    """key -> (scene or rt_scene_desc, oracle scene, camera)"""
    if key[0] == "shear":
        pkg = _pkg()
        sc, cam = general_camera_case(pkg, key[1], max_w=200, max_h=150)
        return sc, oracle_from(pkg, _oracle(), sc), cam
    return build_shared(key)


def _oracle_counts(d):
    return dict(d, hits=d["normals"])


@functools.lru_cache(maxsize=None)
def oracle_counters(key):
    _, osc, cam = build(key)
    return _oracle_counts(osc.render(cam=cam, counters=True, nthreads=8)[1])


def meta(key):
    """What the relations of section 2 need to know about a scene: objects per kernel class, lights per kind."""
    _, osc, _ = build(key)
    return scene_meta(osc)


def scene_meta(osc):
    cls = {"unitsq": 0, "quadric": 0, "linear": 0, "cubic": 0}
    for c in np.asarray(osc.coefs, dtype=np.float64).reshape(-1, 20):
        if np.any(c[:10] != 0):
            cls["cubic"] += 1
        elif np.any(c[13:16] != 0) or not (np.all(c[10:13] == 1.0) or np.all(c[10:13] == 0.0)):
            cls["quadric"] += 1
        elif np.all(c[10:13] == 1.0):
            cls["unitsq"] += 1
        else:
            cls["linear"] += 1
    sph = [bool(v) for v in np.asarray(osc.light_is_spherical).reshape(-1)]
    return dict(classes=cls, n_objects=sum(cls.values()), n_lights=len(sph), n_point=sum(sph), max_reflections=int(osc.max_reflections),
                mirrors=bool(np.any(np.asarray(osc.reflection, dtype=np.float64) > 1e-7)))


# ---- rendering ---------------------------------------------------------------------------------------------------------------
F32, U8 = 0, 1


def frames(pkg, sc, cams, flags=0, fmt=F32, sparse=False, detail=True, **kw):
    """One context, one frame per camera: [(frame, counters, detail block or None)]; without RT_FLAG_COUNT the counters are None.
    sparse: rt_render_sparse into an RGBA8 message, rebuilt with rt_assemble_sparse."""
    counting = bool(flags & pkg.RT_FLAG_COUNT)
    r = pkg.Renderer(sc, device=0, flags=flags, fmt=U8 if sparse else fmt, **kw)
    out = []
    try:
        if sparse:
            import torch
            cap = max(1, ((r.width + 15) // 16) * ((r.local_rows + 15) // 16))
            msg = torch.zeros((1, pkg.Renderer.sparse_bytes(cap)), dtype=torch.uint8, device="cuda:0")
            full = torch.zeros((r.height, r.width, 4), dtype=torch.uint8, device="cuda:0")
        for cam in cams:
            if sparse:
                r.update_sparse(msg.data_ptr(), cap, cam)
                r.assemble_sparse(msg.data_ptr(), cap, full.data_ptr())
                torch.cuda.synchronize()
                img = full.cpu().numpy().copy()
            else:
                r.update(cam)
                img = r.download().copy()
            c = r.counters() if counting else None
            d = r.counters_detail() if counting and detail and not (flags & pkg.RT_FLAG_SIMPLE) else None
            out.append((img, c, d))
    finally:
        r.cleanup_update()
    return out


def same_counters(got, want):
    bad = {c: (got[c], want[c]) for c in COUNTED if got[c] != want[c]}
    return not bad, bad


def check_detail(d, o, m, nocull=False, plane_noscan=False):
    """The detail block `d` of one frame against the oracle's counters `o` of that frame (None: only the relations that need none) and
    the scene's meta data `m`.

    Exact identities (Cnt<true> in rt_wavefront.hip): exec() adds to tests_executed and to one class, solve() to solves and one class,
    cubic() to tests_executed, solves, the cubic class and one branch; cull() adds every kind but the records to cull_evals.
    * shadow_rays_traced <= shadow_rays: cnt.traced() is booked for `wanted` lanes only, each of which books cnt.add(1) ("if (valid)
      cnt.add(1)" / "if (wanted) cnt.traced()" in phase B, wanted implies valid).
    * hit_lights_shaded <= surface_colors: cnt.shaded() is booked per hit and light whose shadow test found no blocker, and a counting
      build tests every hit against every light as the reference does ("COUNT builds test them anyway", phase B), so each booking is
      one of the oracle's surface_color calls.  Equality is not promised: lanes whose directional light is behind the surface sit the
      shading out ("Such lanes sit the shadow test out AND the shading of this light") -- but only they do, and each of them is a shadow
      ray that is not traced, so hit_lights_shaded >= surface_colors - (shadow_rays - shadow_rays_traced).
    * hit_lights_shaded <= shadow_rays_traced holds for directional lights (shaded lanes are `wanted` ones).  A point light behind
      the surface is not traced but its +0 term is shaded ("lanes sit the TEST out only ... their term is then shaded as +0"), so with
      point lights the bound is shadow_rays_traced + hits * point lights.
    * primary_rays_formed: "every lane of a tracing workgroup forms a primary ray (lanes outside the image a clamped one)"."""
    ex, sv, cb, ck = d["executed_by_class"], d["solves_by_class"], d["cubic_branches"], d["cull_by_kind"]
    assert sum(ex.values()) == d["tests_executed"], d
    assert sum(sv.values()) + sum(cb.values()) == d["solves"], d
    assert sum(cb.values()) == ex["cubic"], d
    assert d["cull_evals"] == ck["tile"] + ck["primary"] + ck["shadow_directional"] + ck["shadow_point"], d
    assert d["shadow_rays_traced"] <= d["shadow_rays"], d
    assert d["hit_lights_shaded"] <= d["shadow_rays"], d
    assert d["hit_lights_shaded"] <= d["shadow_rays_traced"] + d["hits"] * m["n_point"], d
    assert d["cubic_refused"] <= ex["cubic"], d
    for k, n in m["classes"].items():
        if n == 0:
            assert ex[k] == 0 and (k == "cubic" or sv[k] == 0), (k, d)
    if nocull:   # fa.cull = 0 (rt_capi.cpp): no cone, no shadow-phase culling, no records (n_crec = 0), and -- fa.all_cullable = 0 -- no tile test
        assert not any(ck.values()), d
    assert d["primary_rays_formed"] % WG == 0, d
    if o is not None:   # relations to the oracle
        assert o["surface_colors"] - (d["shadow_rays"] - d["shadow_rays_traced"]) <= d["hit_lights_shaded"] <= o["surface_colors"], (d, o)
        if plane_noscan:
            assert d["primary_rays_formed"] >= o["primary_rays"], (d, o)
    assert d["tests_executed"] <= (d["primary_rays_formed"] + d["reflect_rays"] + d["shadow_rays_traced"]) * m["n_objects"], d
    assert d["tests_executed"] >= d["hits"], d


def check_scene(pkg, key, flags=0, fmt=F32, sparse=False, **checks):
    """Three counting frames of one context: counters == the oracle's after each, frame == the product frame, the detail block's
    relations.  Returns the frames."""
    sc, _, cam = build(key)
    want, m = oracle_counters(key), meta(key)
    (product, _, _), = frames(pkg, sc, [cam], flags, fmt, sparse)
    got = frames(pkg, sc, [cam] * 3, flags | pkg.RT_FLAG_COUNT, fmt, sparse)
    for i, (img, c, d) in enumerate(got):
        ok, bad = same_counters(c, want)
        assert ok, (key_id(key), flags, f"frame {i + 1}", bad)
        assert identical(img, product), (key_id(key), flags, f"frame {i + 1}")
        if d is not None:
            check_detail(d, want, m, nocull=bool(flags & pkg.RT_FLAG_NOCULL), **checks)
    return got


# ---- 1. + 2.: every scene under the default, RT_FLAG_NOCULL and RT_FLAG_SIMPLE ------------------------------------------------
@pytest.mark.parametrize("key", SCENES, ids=key_id)
def test_counters_equal_the_oracles(pkg, key):
    a = check_scene(pkg, key)
    b = check_scene(pkg, key, pkg.RT_FLAG_NOCULL)
    check_scene(pkg, key, pkg.RT_FLAG_SIMPLE)
    # culling only removes executed tests, class by class (nearest / shadow_blocker: popcount of the surviving spheres instead of all)
    for (_, _, da), (_, _, db) in zip(a, b):
        for k in da["executed_by_class"]:
            assert da["executed_by_class"][k] <= db["executed_by_class"][k], (k, da, db)


# ---- the other variants, each on at least eight scenes with a mirror scene and one of more than 64 objects among them ----------
def _is(key, **want):
    assert key[0] == "random"
    have = dict(n=key[2] + int(key[4]), plane=key[4], mirrors=key[5])
    return all(have[k] == v for k, v in want.items())


GENERAL = [RANDOM[1], RANDOM[3], RANDOM[4], RANDOM[5], RANDOM[8], RANDOM[10], RANDOM[11], RANDOM[13], RANDOM[15], MIXED[3], MIXED[11], FUZZ[7], SHEAR[0],
           MIRRORS[2]]
ALL_SPHERES = [k for k in RANDOM if not k[4]] + [SHEAR[2]]   # no plane: two of them with mirrors (there the general instantiation runs)
VARIANTS = {
    "nolean": ALL_SPHERES + [RANDOM[8]],
    "lean": ALL_SPHERES,
    "nosplit": GENERAL,
    "noscan": GENERAL,
    "static_order": GENERAL,
    "rgba8": GENERAL,
    "sparse": GENERAL,
}
for _name, _keys in VARIANTS.items():   # coverage cannot shrink silently
    _r = [k for k in _keys if k[0] == "random"]
    assert len(set(_keys)) >= 8, _name
    assert any(k[5] for k in _r), f"{_name}: no scene with mirrors"
    assert any(k[2] + int(k[4]) > 64 for k in _r), f"{_name}: no scene with more than 64 objects"
assert all(not k[4] for k in VARIANTS["lean"] if k[0] == "random")


@pytest.mark.parametrize("variant,key", [(v, k) for v, keys in VARIANTS.items() for k in keys], ids=lambda p: p if isinstance(p, str) else key_id(p))
def test_counters_equal_the_oracles_in_the_other_variants(pkg, monkeypatch, variant, key):
    if variant == "lean":
        # rt_create reads MI355RT_LEAN: frames this small would otherwise leave the lean instantiation after the first one
        monkeypatch.setenv("MI355RT_LEAN", "always")
        lean = check_scene(pkg, key)
        monkeypatch.delenv("MI355RT_LEAN")
        general = check_scene(pkg, key, pkg.RT_FLAG_NOLEAN)
        # the lean instantiation executes no more unit-sphere tests than the general one (its own-sphere rule, its 8 x 8 blocks' tighter balls)
        assert lean[0][2]["executed_by_class"]["unitsq"] <= general[0][2]["executed_by_class"]["unitsq"]
        # both book the lanes the product build traces and shades: the same hits face the same lights in either instantiation
        for (_, _, dl), (_, _, dg) in zip(lean, general):
            assert dl["shadow_rays_traced"] == dg["shadow_rays_traced"] and dl["hit_lights_shaded"] == dg["hit_lights_shaded"], (dl, dg)
        return
    flags = {"nolean": pkg.RT_FLAG_NOLEAN, "nosplit": pkg.RT_FLAG_NOSPLIT, "noscan": pkg.RT_FLAG_NOSCAN, "static_order": pkg.RT_FLAG_STATIC_ORDER}.get(variant, 0)
    plane = variant == "noscan" and meta(key)["classes"]["linear"] > 0
    check_scene(pkg, key, flags, fmt=U8 if variant == "rgba8" else F32, sparse=variant == "sparse", plane_noscan=plane)


# ---- camera sequences: the case that once booked rays twice ---------------------------------------------------------------------
SEQUENCE_VARIANTS = ["default", "nolean", "mirrors"]


def _sequence(pkg, sc, cams, flags):
    """One counting context through `cams`: after every frame the counters are the oracle's for that view."""
    osc = oracle_from(pkg, _oracle(), sc)
    m, want = scene_meta(osc), {}
    got = frames(pkg, sc, cams, flags | pkg.RT_FLAG_COUNT)
    for i, (cam, (_, c, d)) in enumerate(zip(cams, got)):
        k = cam.tobytes()
        if k not in want:
            want[k] = _oracle_counts(osc.render(cam=cam, counters=True, nthreads=8)[1])
        ok, bad = same_counters(c, want[k])
        assert ok, (f"frame {i}", bad)
        check_detail(d, want[k], m)
    return [want[cam.tobytes()] for cam in cams]


@pytest.mark.parametrize("variant", SEQUENCE_VARIANTS)
def test_counters_through_camera_cuts(pkg, variant):
    """The views of test_launch_order_feedback_survives_camera_cuts at 640 x 360: empty, full, partial, stale and truncated lists."""
    sc, seq, (away, front, side) = camera_cut_sequence(pkg, mirrors=variant == "mirrors")
    want = _sequence(pkg, sc, seq, pkg.RT_FLAG_NOLEAN if variant == "nolean" else 0)
    assert want[0]["hits"] == 0 and want[2]["hits"] > 0 and want[6]["hits"] > 0   # away is empty; front and side see the scene


@pytest.mark.parametrize("variant,seed", [("default", 2), ("default", 4), ("nolean", 2), ("nolean", 4), ("mirrors", 1), ("mirrors", 3)])
def test_counters_through_random_walks(pkg, variant, seed):
    """Walks of test_launch_order_feedback_random_walks (odd seeds have mirrors): drifts, jumps, frames that look away."""
    sc, cams = random_walk(pkg, seed)
    assert scene_meta(oracle_from(pkg, _oracle(), sc))["mirrors"] == (variant == "mirrors")
    want = _sequence(pkg, sc, cams, pkg.RT_FLAG_NOLEAN if variant == "nolean" else 0)
    assert sum(w["hits"] > 0 for w in want) >= 2, "the walk never saw the scene"


# ---- bands -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,band,world", [(37, 1, 2), (50, 3, 4), (64, 5, 3), (100, 33, 2), (16, 8, 5)])
def test_counters_of_banded_frames(pkg, h, band, world):
    """Five of test_row_band_ownership_variants' cases: each rank's counters are the oracle's for its rows, and they add up to the frame's."""
    sc = random_scene(pkg, 99, 14, 5, w=150, h=h, mirrors=True)
    osc = oracle_from(pkg, _oracle(), sc)
    full = _oracle_counts(osc.render(counters=True, nthreads=8)[1])
    total = {c: 0 for c in COUNTED}
    for rank in range(world):
        r = pkg.Renderer(sc, device=0, rank=rank, world=world, band_rows=band, flags=pkg.RT_FLAG_COUNT)
        try:
            rows = r.row_map()
            assert np.array_equal(rows, pkg.band_rows_of_rank(h, band, world, rank))
            for frame in range(3):
                r.update()
                got = r.counters()
                want = _oracle_counts(osc.render(rows=rows, counters=True, nthreads=8)[1]) if len(rows) else {c: 0 for c in COUNTED}
                ok, bad = same_counters(got, want)
                assert ok, (rank, frame, bad)
        finally:
            r.cleanup_update()
        for c in COUNTED:
            total[c] += got[c]
    assert total == {c: full[c] for c in COUNTED}


# ---- determinism of the detail block ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [RANDOM[4], RANDOM[9], RANDOM[12], MIXED[5], MIXED[17], FUZZ[10], SHEAR[3], MIRRORS[2]], ids=key_id)
def test_detail_block_is_deterministic(pkg, key):
    """No launch-order feedback and no half tiles: three frames of one camera give the same detail block word for word, and so does a
    second context; with the feedback on, two fresh contexts still agree on their first frame."""
    sc, _, cam = build(key)
    fixed = pkg.RT_FLAG_COUNT | pkg.RT_FLAG_STATIC_ORDER | pkg.RT_FLAG_NOSPLIT
    a = frames(pkg, sc, [cam] * 3, fixed)
    assert a[0][2] == a[1][2] == a[2][2], key_id(key)
    assert frames(pkg, sc, [cam], fixed)[0][2] == a[0][2]
    assert frames(pkg, sc, [cam], pkg.RT_FLAG_COUNT)[0][2] == frames(pkg, sc, [cam], pkg.RT_FLAG_COUNT)[0][2]


def test_identities_hold_in_the_fma_contracted_build(pkg):
    """RT_FLAG_FAST rounds differently, so its counters are not the oracle's; the identities between the words do not care."""
    for key in (RANDOM[4], RANDOM[10], MIXED[3], MIRRORS[2]):
        sc, _, cam = build(key)
        m = meta(key)
        for _, c, d in frames(pkg, sc, [cam] * 3, pkg.RT_FLAG_COUNT | pkg.RT_FLAG_FAST):
            assert sum(d["executed_by_class"].values()) == d["tests_executed"]
            assert sum(d["solves_by_class"].values()) + sum(d["cubic_branches"].values()) == d["solves"]
            ck = d["cull_by_kind"]
            assert d["cull_evals"] == ck["tile"] + ck["primary"] + ck["shadow_directional"] + ck["shadow_point"]
            assert d["shadow_rays_traced"] <= d["shadow_rays"] and d["hit_lights_shaded"] <= d["shadow_rays_traced"] + d["hits"] * m["n_point"]
            assert d["primary_rays_formed"] % WG == 0 and d["tests_executed"] >= d["hits"]


# ---- 3. degree 3 -------------------------------------------------------------------------------------------------------------
CUBIC_SCENES = [("file", n) for n in CUBIC] + [("random_cubic", s) for s in range(6)] + [("many", 0)]
# scenes on which the five counters equal the device-libm oracle's on the MI355X (DESIGN.md 5.7 has the figures of the others)
CUBIC_EXACT = set(CUBIC_SCENES)


def cubic_scene(pkg, key):
    if key[0] == "file":
        return pkg.Scene.load_from_file(scene_path(key[1])).set_size(240, 180), None
    if key[0] == "random_cubic":
        return random_cubic_scene(pkg, key[1])
    return many_cubic_objects_and_mirrors(pkg), None


def cubic_bound(plain, dev, m):
    """What a last-ulp change of cbrt / acos / cos moves the oracle's own counters by on this scene (plain against device libm), times
    two -- and at least what one flipped pixel moves them by per bounce: n_objects * (1 + n_lights) tests, n_lights shadow rays, one hit,
    one reflected ray.  Primary rays do not depend on the solver."""
    bounces = 1 + (m["max_reflections"] if m["mirrors"] else 0)
    floor = dict(primary_rays=0, shadow_rays=m["n_lights"] * bounces, reflect_rays=bounces, tests=m["n_objects"] * (1 + m["n_lights"]) * bounces, hits=bounces)
    return {c: max(2 * abs(plain[c] - dev[c]), floor[c]) if c != "primary_rays" else 0 for c in COUNTED}


@pytest.mark.parametrize("key", CUBIC_SCENES, ids=lambda k: f"{k[0]}-{k[1]}")
def test_degree_three_counters(pkg, key):
    """Counting frame == product frame; wavefront, NOCULL and simple kernels agree on the five counters (they share the device functions);
    the identities; the counters against the oracle under the device's cbrt / acos / cos; the solver branches.

    cubic_branches: nearest books every test (cnt.cubic(br)), shadow_blocker only what the product build executes
    (cnt.cubic(br, prod)), so on scenes whose every object is of degree 3 the total is at least (primary_rays + reflect_rays) * n_cubic
    and every branch is at most the oracle's (cardano <-> br_cardano, trig <-> br_trig, quad <-> br_quad_hit + br_quad_miss,
    linear <-> br_linear + br_none)."""
    sc, cam = cubic_scene(pkg, key)
    osc = oracle_from(pkg, _oracle(), sc)
    m = scene_meta(osc)
    (product, _, _), = frames(pkg, sc, [cam])
    got = frames(pkg, sc, [cam] * 3, pkg.RT_FLAG_COUNT)
    plain = _oracle_counts(osc.render(cam=cam, counters=True, nthreads=8)[1])
    (_, dev), _, _ = D.render_device_libm(D.lib(pkg), osc, cam=cam, counters=True, nthreads=8)
    dev = _oracle_counts(dev)
    bound = cubic_bound(plain, dev, m)
    print(f"\ndegree-3 counters {key}: plain oracle {[plain[c] for c in COUNTED]} device-libm oracle {[dev[c] for c in COUNTED]} "
          f"device {[got[0][1][c] for c in COUNTED]} bound {[bound[c] for c in COUNTED]}")
    for i, (img, c, d) in enumerate(got):
        assert identical(img, product), f"frame {i + 1}"
        assert {k: c[k] for k in COUNTED} == {k: got[0][1][k] for k in COUNTED}, f"frame {i + 1}"
        check_detail(d, dev if key in CUBIC_EXACT else None, m)   # (a scene held to a bound has no oracle figure to relate to)
    c = got[0][1]
    for fl in (pkg.RT_FLAG_NOCULL, pkg.RT_FLAG_SIMPLE):
        (img, other, _), = frames(pkg, sc, [cam], fl | pkg.RT_FLAG_COUNT)
        assert identical(img, product)
        assert same_counters(other, c)[0], (fl, same_counters(other, c)[1])
    if key in CUBIC_EXACT:
        ok, bad = same_counters(c, dev)
        assert ok, bad
    else:
        for k in COUNTED:
            assert abs(c[k] - dev[k]) <= bound[k], (k, c[k], dev[k], bound[k])
    if m["classes"]["cubic"] == m["n_objects"]:
        cb = got[0][2]["cubic_branches"]
        want = dict(cardano=dev["br_cardano"], trig=dev["br_trig"], quad=dev["br_quad_hit"] + dev["br_quad_miss"], linear=dev["br_linear"] + dev["br_none"])
        assert sum(cb.values()) >= (c["primary_rays"] + c["reflect_rays"]) * m["classes"]["cubic"], (cb, c)
        if key in CUBIC_EXACT:
            for k in cb:
                assert cb[k] <= want[k], (k, cb, want)

