"""Culled bounce rays on the GPU (RT_FLAG_STREAM_CULL_BOUNCE; csrc/rt_stream_cull_bounce.hip).  The frame is
RT_FLAG_STREAM's frame by definition: every strict frame of degree <= 2 here is compared bit for bit with the CPU oracle, with the
RT_FLAG_STREAM | RT_FLAG_STREAM_CULL context and with the plain RT_FLAG_STREAM context, in both formats.  The host-side conditions (the
predicate against the oracle, the statistics scene's L >= D / 4) are in tests/test_stream_cull_bounce_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import bounce_cull_lab as B  # noqa: E402
import cull_lab as L  # noqa: E402
import raw_desc_scenes as R  # noqa: E402
import ssaa_ref  # noqa: E402
import stream_cull_lab as SC  # noqa: E402
import stream_scenes as S  # noqa: E402
from test_stream_cull_gpu import SWAPPED, check, frame, held_to_the_lab  # noqa: E402
from test_stream_cull_host import raw_scene_with_unbounded_spheres  # noqa: E402
from test_stream_gpu import MOVED  # noqa: E402

pytestmark = pytest.mark.gpu

F32, U8 = 0, 1


@pytest.fixture(autouse=True)
def the_feature(pkg):
    assert pkg.RT_FLAG_STREAM_CULL_BOUNCE == 1048576


def three(pkg):
    return pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_BOUNCE


def bframe(pkg, sc, cam=None, expect=True, **kw):
    r = pkg.Renderer(sc, device=0, **kw)
    try:
        assert r.stream_cull_bounce == expect, (r.stream_cull_bounce, r.stream_cull, r.streamed)
        r.update(cam)
        return r.download()
    finally:
        r.cleanup_update()


def check3(pkg, sc, want, what, cam=None, flags=None, expect=True, expect_cull=True, **kw):
    """Flagged == oracle == RT_FLAG_STREAM without either culling flag (test_stream_cull_gpu.check: both formats), and flagged ==
    the same context without the new flag (both formats)."""
    flags = three(pkg) if flags is None else flags
    bounce = pkg.RT_FLAG_STREAM_CULL_BOUNCE
    check(pkg, sc, want, what, cam=cam, flags=flags, plain_flags=flags & ~(pkg.RT_FLAG_STREAM_CULL | bounce), expect_cull=expect_cull, **kw)
    for fmt in (pkg.RT_FMT_RGBA32F, pkg.RT_FMT_RGBA8):
        got = bframe(pkg, sc, cam, expect, flags=flags, fmt=fmt, **kw)
        assert R.same(got, frame(pkg, sc, cam, expect_cull, flags=flags & ~bounce, fmt=fmt, **kw)), (what, fmt)


def expected(osc_arrays, max_refl):
    """(stream cull, stream cull bounce) of a streamed context from the scene image and the rule of include/mi355rt.h."""
    w = SC.image(osc_arrays)[2]
    mirror = bool((np.asarray(osc_arrays["reflection"], np.float32).astype(np.float64) > 1e-7).any())
    return bool(w["cull"]), bool(w["cull"]) and mirror and max_refl >= 1 and (w["n_us"] + 63) // 64 >= 2


def mirrored(osc, pad=70, seed=0, depth=2):
    """The oracle scene with every second object that reflects nothing given the ratio 0.5 (odd ratios stay), a far cluster of `pad` small
    spheres of which every third reflects -- so that the unit-sphere table has a second chunk -- and at least `depth` reflections."""
    t = S.O.Scene(osc.width, osc.height, osc.fov_deg, max(int(osc.max_reflections), depth), np.array(osc.bg_color, dtype=np.float32))
    t.vertical_fov = osc.vertical_fov
    for i, o in enumerate(osc.objects):
        ratio = o.reflection_ratio
        t.add_object(list(o.c), list(o.color), 0.5 if (ratio == 0.0 and i % 2 == 0) else ratio)
    rng = np.random.default_rng(900 + seed)
    far = np.array([14.0, 9.0, 30.0]) * rng.choice([-1.0, 1.0], 3) * np.array([1.0, 1.0, rng.uniform(0.8, 1.2)])
    far[2] = abs(far[2])
    for k in range(pad):
        t.add_object(R.sphere(tuple(far + rng.normal(scale=1.5, size=3)), 0.3), (0.5, 0.6, 0.7), 0.4 if k % 3 == 0 else 0.0)
    for l in osc.lights:
        t.lights.append(R.stored_light(l.is_spherical, list(l.p), list(l.color)))
    return t


def check_oracle_scene(pkg, osc, what, cam=None):
    cull, bounce = expected(SC.arrays_of_oracle(osc), int(osc.max_reflections))
    check3(pkg, R.desc(pkg, osc), osc.render(cam=cam, nthreads=8), what, cam=cam, expect=bounce, expect_cull=cull)
    return bounce


# ---- frames bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 128, 129, 193])
def test_sphere_counts(pkg, n):
    """65: the second chunk holds one entry; 128 / 129 / 193: a full last chunk, one entry behind it, four chunks."""
    sc = S.field(pkg, n, S.FIELD_SEED, mirrors=True, depth=2)
    check3(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), (n, "depth 2"))
    sc = S.field(pkg, n, S.FIELD_SEED, w=37, h=21, mirrors=True, depth=1)
    check3(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), (n, "37 x 21"))


def test_more_than_64_chunks(pkg):
    sc = S.field(pkg, 4100, 3, mirrors=True, depth=2)
    check3(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), "4100 spheres", flags=pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_BOUNCE)


def test_large_mixed_scene(pkg):
    """Mirrors that are ellipsoids and planes, bouncing onto spheres (degree <= 2: held to the oracle; degree-3 mirrors:
    test_cubic_mirrors_with_a_field)."""
    sc = S.mixed_large(pkg, 2000, S.MIXED_SEED, depth=2)
    check3(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), "large mixed", flags=pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_BOUNCE)


def cubic_mirror_and_field(pkg, name, w, h, with_quadric):
    """A shipped degree-3 scene whose surface is made a mirror (ratio 0.5), enlarged by the mirrored 65-sphere field (two chunks) -- and,
    with_quadric, by one reflecting ellipsoid with cross terms, so that the kernel for general quadrics AND degree 3 runs.  Two bounces."""
    a = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h).arrays()
    f = S.field(pkg, 65, S.FIELD_SEED, w=w, h=h, mirrors=True, depth=2).arrays()
    coefs, refl, alb = [a["coefs"], f["coefs"]], [np.full(len(a["reflection"]), 0.5, np.float32), f["reflection"]], [a["albedo"], f["albedo"]]
    if with_quadric:
        coefs.append(S.ellipsoid(np.array([3.0, 2.0, 18.0]), np.array([1.5, 0.8, 1.1]), np.array([0.3, -0.2, 0.1]))[None, :])
        refl.append(np.array([0.3], np.float32))
        alb.append(np.array([[0.9, 0.6, 0.3]], np.float32))
    coefs = np.concatenate(coefs)
    assert (coefs[:len(a["coefs"]), :10] != 0).any()      # (a degree-3 object)
    return pkg.desc_from_arrays(w, h, a["vertical_fov"], a["bg_color"], 2, coefs, np.concatenate(refl).astype(np.float32), np.concatenate(alb).astype(np.float32),
                                a["light_is_spherical"], a["light_p"], a["light_color"])


@pytest.mark.parametrize("with_quadric", [False, True], ids=["cubic", "cubic+quadric"])
@pytest.mark.parametrize("name", ["clebsch", "cayley"])
def test_cubic_mirrors_with_a_field(pkg, name, with_quadric):
    """The HAS_CUBIC instantiations, <0, 1> and <1, 1>, strict and fast: a degree-3 mirror bouncing onto spheres.  Degree 3 is held to the
    library's own frames: the flagged frame equals the RT_FLAG_STREAM | RT_FLAG_STREAM_CULL frame and the plain RT_FLAG_STREAM frame bit
    for bit in both formats, the FAST frame its unflagged twins; the mirror changes the frame and some bounce chunk is left unstaged."""
    w, h = 48, 36
    d = cubic_mirror_and_field(pkg, name, w, h, with_quadric)
    f = pkg
    for fmt in (f.RT_FMT_RGBA32F, f.RT_FMT_RGBA8):
        got = bframe(pkg, d, flags=three(pkg), fmt=fmt)
        assert R.same(got, frame(pkg, d, None, True, flags=f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_CULL, fmt=fmt)), (name, fmt)
        assert R.same(got, frame(pkg, d, None, False, flags=f.RT_FLAG_STREAM, fmt=fmt)), (name, fmt)
    fast = bframe(pkg, d, flags=three(pkg) | f.RT_FLAG_FAST)
    assert R.same(fast, frame(pkg, d, None, True, flags=f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_CULL | f.RT_FLAG_FAST))
    assert R.same(fast, frame(pkg, d, None, False, flags=f.RT_FLAG_STREAM | f.RT_FLAG_FAST))


@pytest.mark.parametrize("with_quadric", [False, True], ids=["cubic", "cubic+quadric"])
def test_cubic_mirror_bounces_are_culled(pkg, monkeypatch, with_quadric):
    """... and the bounce queries of that frame are real work: the degree-3 mirror is seen, its lanes bounce, chunks are left unstaged."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    d = cubic_mirror_and_field(pkg, "clebsch", 48, 36, with_quadric)
    r = pkg.Renderer(d, device=0, flags=three(pkg))
    try:
        assert r.stream_cull_bounce
        r.update()
        w = r.stream_cull_bounce_stats()
        g = r.gbuffer()[0].cpu().numpy()
        print("bounce work words", w, "pixels of the degree-3 mirror", int((g == 0).sum()))
        assert (g == 0).sum() > 50      # the cubic (object 0) fills part of the frame, and every one of its pixels bounces
        assert w[0] > 0 and w[1] < w[0] and 0 < w[3] < w[2]
    finally:
        r.cleanup_update()


def thin_cone_scene(pkg, w=63, h=47):
    """The unmirrored 129-sphere field and ONE mirror: a thin double cone (half-opening 2^-10) whose apex lies on the centre pixel's ray
    at t = 8 and whose axis crosses the image at a slope no other pixel centre lies on.  The centre ray meets the apex, where the gradient
    vanishes: its normal, hence its bounce ray, is NaN."""
    sc = S.field(pkg, 129, S.FIELD_SEED, w=w, h=h, mirrors=False, depth=2)
    ax = np.array([1.0, 0.37, 0.0])
    ax /= np.linalg.norm(ax)
    k = 1.0 + 2.0 ** -20
    q = np.zeros(20)
    q[10], q[11], q[12], q[13], q[18], q[19] = 1.0 - k * ax[0] ** 2, 1.0 - k * ax[1] ** 2, 1.0, -2.0 * k * ax[0] * ax[1], -16.0, 64.0
    sc.add_object(q, (0.8, 0.7, 0.6), 0.5)
    return sc


def test_a_bounce_ray_outside_the_tables_proof(pkg, monkeypatch):
    """A bouncing lane whose ray is NaN: it goes through the dense path over all objects, nothing is culled for it, and a bounce query
    whose only lane it is counts in word [4].  From the oracle's per-segment rays: which pixels bounce, and that the centre pixel's bounce
    ray is NaN.  The frame is the oracle's and the unflagged contexts' (check3)."""
    import paths_ref
    import rays_ref
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    w, h = 63, 47
    sc = thin_cone_scene(pkg, w, h)
    osc = S.oracle_of(pkg, sc)
    rays = np.ascontiguousarray(rays_ref.primary_rays(osc)).reshape(-1)
    seg = np.zeros((3, len(rays)), dtype=rays_ref.RAY_DTYPE)
    seg["o"] = 7.0      # (a sentinel: no bounce origin has x = 7 exactly)
    paths_ref.paths(osc, rays, seg_rays=seg)
    bouncing = np.flatnonzero(seg["o"][1, :, 0] != 7.0)
    centre = (h // 2) * w + w // 2
    assert centre in bouncing and np.isnan(seg["d"][1, centre]).all() and np.isnan(seg["o"][1, centre]).all()
    finite = [i for i in bouncing if i != centre]
    assert np.isfinite(seg["d"][1, finite]).all() and not (seg["o"][2, :, 0] != 7.0).any()
    blocks = {(i // w // 8, i % w // 8) for i in bouncing}
    alone = (centre // w // 8, centre % w // 8) not in {(i // w // 8, i % w // 8) for i in finite}
    assert alone      # the NaN lane is the only bouncing lane of its wave
    check3(pkg, sc, osc.render(nthreads=8), "thin cone")
    r = pkg.Renderer(sc, device=0, flags=three(pkg))
    try:
        r.update()
        got = r.stream_cull_bounce_stats()
        print("bounce work words", got, "bouncing pixels", bouncing)
        n_chunks = 3
        assert got[0] == len(blocks) * n_chunks and got[2] == len(finite) * n_chunks and got[4] == 1, got
    finally:
        r.cleanup_update()


@pytest.mark.parametrize("seed", range(8))
def test_raw_descriptor_scenes(pkg, seed):
    """Odd light vectors, non-finite colours and ratios, moved cameras (tests/tools/raw_desc_scenes.py), given mirrors and a second chunk."""
    osc, cam = R.scene(seed)
    osc.width, osc.height = min(osc.width, 64), min(osc.height, 48)
    check_oracle_scene(pkg, mirrored(osc, seed=seed), ("raw", seed), cam=cam)


NAMED = [n for n in sorted(R.NAMED) if R.NAMED[n][0] in ("mirror", "lean65") and R.NAMED[n][1] != "many"]


@pytest.mark.parametrize("part", range(4))
def test_named_raw_descriptor_scenes(pkg, part):
    """Every named oddity of the mirror class (NaN and negative ratios, non-finite albedos and colours, directions at EPS) and of the
    70-sphere class, with mirrors and a second chunk, in four parts.  (The forty-light layouts are left to tests/test_stream_cull_gpu.py:
    the lights do not enter a bounce query.)  Every one of them reaches a true decision."""
    assert any("refl_nan" in n for n in NAMED) and any("refl_neg" in n for n in NAMED) and len(NAMED) >= 40
    for name in NAMED[part::4]:
        osc, _, cams = R.named(name)
        osc.width, osc.height = min(osc.width, 64), min(osc.height, 48)
        assert check_oracle_scene(pkg, mirrored(osc), name, cam=cams[0]), name


def test_spheres_without_a_radius(pkg):
    a = raw_scene_with_unbounded_spheres()
    a["reflection"] = np.where(np.arange(len(a["reflection"])) % 3 == 0, 0.5, 0.0).astype(np.float32)
    d = pkg.desc_from_arrays(64, 48, np.radians(S.FOV), (0.05, 0.1, 0.2), 2, a["coefs"], a["reflection"], a["albedo"], a["light_is_spherical"], a["light_p"], a["light_color"])
    osc = S.O.Scene(64, 48, 0.0, 2, (0.05, 0.1, 0.2))
    osc.vertical_fov = float(np.radians(S.FOV))
    for i in range(len(a["reflection"])):
        osc.add_object(a["coefs"][i], a["albedo"][i], a["reflection"][i])
    for i in range(2):
        osc.lights.append(R.stored_light(a["light_is_spherical"][i], a["light_p"][i], a["light_color"][i]))
    check3(pkg, d, osc.render(nthreads=8), "unbounded tail")


@pytest.mark.parametrize("i", range(0, L.N_GRAZE_SCENES, 4))
def test_grazing_scenes_with_mirrors(pkg, i):
    """cull_lab's scenes with spheres tangent to a block's cone or a chunk's shadow volume, every second sphere a mirror, with a far cluster."""
    osc = L.spec_to_oracle(L.graze_scene_spec(i))
    assert check_oracle_scene(pkg, mirrored(osc, seed=i), ("graze", i))


def test_moved_camera(pkg):
    sc = S.field(pkg, 193, S.FIELD_SEED, mirrors=True, depth=2)
    for cam in (pkg.camera_matrix(*MOVED), pkg.camera_matrix((6.0, 2.0, 4.0), 120.0, -9.0)):
        check3(pkg, sc, S.oracle_of(pkg, sc).render(cam=cam, nthreads=8), "moved", cam=cam)


@pytest.mark.parametrize("fmt", [F32, U8], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("k", [2, 4])
def test_supersampling(pkg, k, fmt):
    w, h = 40, 30
    flag = pkg.RT_FLAG_SSAA2 if k == 2 else pkg.RT_FLAG_SSAA4
    sc = S.field(pkg, 129, S.FIELD_SEED, w=w, h=h, mirrors=True, depth=2)
    want = ssaa_ref.resolve(S.oracle_of(pkg, sc).with_size(k * w, k * h).render(nthreads=8), k)
    want = ssaa_ref.quantise(want) if fmt == U8 else want
    got = bframe(pkg, sc, flags=three(pkg) | flag, fmt=fmt)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert R.same(got, frame(pkg, sc, None, True, flags=(three(pkg) | flag) & ~pkg.RT_FLAG_STREAM_CULL_BOUNCE, fmt=fmt))


def test_rank_1_of_3_with_bands_of_8(pkg):
    sc = S.field(pkg, 193, S.FIELD_SEED, w=64, h=50, mirrors=True, depth=2)
    want = S.oracle_of(pkg, sc).render(nthreads=8)
    r = pkg.Renderer(sc, device=0, rank=1, world=3, band_rows=8, flags=three(pkg))
    try:
        assert r.stream_cull_bounce
        r.update()
        rows = r.row_map()
        assert 0 < len(rows) < 50 and R.same_as_oracle(r.download()[..., :3], want[rows])
    finally:
        r.cleanup_update()


def test_fast_variant_is_its_unflagged_twin(pkg):
    """RT_FLAG_FAST: bit for bit the FAST frame of the context without the flag, and of plain RT_FLAG_STREAM | RT_FLAG_FAST."""
    for sc in (S.field(pkg, 193, S.FIELD_SEED, mirrors=True, depth=2), S.mixed_large(pkg, 2000, S.MIXED_SEED, depth=2)):
        got = bframe(pkg, sc, flags=three(pkg) | pkg.RT_FLAG_FAST)
        assert R.same(got, frame(pkg, sc, None, True, flags=pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_FAST))
        assert R.same(got, frame(pkg, sc, None, False, flags=pkg.RT_FLAG_STREAM | pkg.RT_FLAG_FAST))


@pytest.mark.parametrize("transport", ["dense", "sparse"])
def test_multi_renderer(pkg, transport):
    extra = pkg.RT_MULTI_SPARSE if transport == "sparse" else 0
    sc = S.field(pkg, 193, S.FIELD_SEED, mirrors=True, depth=2)
    want = S.oracle_of(pkg, sc).render(nthreads=8)
    m = pkg.MultiRenderer(sc, [0, 0], band_rows=8, parts=2, flags=three(pkg) | extra)
    try:
        assert m.stream_cull_bounce is True
        for _ in range(2):
            m.update()
        assert R.same_as_oracle(m.download()[..., :3], want), transport
    finally:
        m.cleanup_update()
    m = pkg.MultiRenderer(sc, [0, 0], band_rows=8, parts=2, flags=(three(pkg) & ~pkg.RT_FLAG_STREAM_CULL) | extra)
    try:
        assert m.stream_cull_bounce is False
    finally:
        m.cleanup_update()


# ---- the decision -------------------------------------------------------------------------------------------------------------------------
def decision_cases(pkg):
    f = pkg
    mirrors = S.field(pkg, 129, S.FIELD_SEED, mirrors=True, depth=2)
    return [("without RT_FLAG_STREAM_CULL", mirrors, f.RT_FLAG_STREAM | f.RT_FLAG_STREAM_CULL_BOUNCE),
            ("with RT_FLAG_NOCULL", mirrors, three(pkg) | f.RT_FLAG_NOCULL),
            ("no mirror", S.field(pkg, 129, S.FIELD_SEED, mirrors=False, depth=2), three(pkg)),
            ("max_reflections = 0", S.field(pkg, 129, S.FIELD_SEED, mirrors=True, depth=0), three(pkg)),
            ("one chunk", S.field(pkg, 64, S.FIELD_SEED, mirrors=True, depth=2), three(pkg)),
            ("not streamed", mirrors, f.RT_FLAG_STREAM_CULL | f.RT_FLAG_STREAM_CULL_BOUNCE)]


@pytest.mark.parametrize("case", range(6))
def test_decision_false_is_the_context_without_the_flag(pkg, monkeypatch, case):
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    what, sc, flags = decision_cases(pkg)[case]
    r, p = pkg.Renderer(sc, device=0, flags=flags), pkg.Renderer(sc, device=0, flags=flags & ~pkg.RT_FLAG_STREAM_CULL_BOUNCE)
    try:
        assert r.stream_cull_bounce is False and p.stream_cull_bounce is False, what
        assert r.stream_cull == p.stream_cull and r.streamed == p.streamed, what
        with pytest.raises(pkg.RtError) as e:
            r.stream_cull_bounce_stats()
        assert e.value.code == -1 and "rt_debug_stream_cull_bounce" in e.value.message
        assert R.same(r.debug_scene_blob(), p.debug_scene_blob()) and R.same(r.stream_bounds(), p.stream_bounds()), what
        for _ in range(2):
            r.update()
            p.update()
        assert R.same(r.download(), p.download()), what
        if r.stream_cull:
            assert r.stream_cull_stats() == p.stream_cull_stats(), what
    finally:
        r.cleanup_update()
        p.cleanup_update()


def test_decision_true_otherwise(pkg):
    for sc, flags in ((S.field(pkg, 65, S.FIELD_SEED, mirrors=True, depth=1), three(pkg)),
                      (S.field(pkg, 129, S.FIELD_SEED, mirrors=True, depth=2), three(pkg) | pkg.RT_FLAG_FAST),
                      (S.field(pkg, 129, S.FIELD_SEED, mirrors=True, depth=2), three(pkg) | pkg.RT_FLAG_SSAA2),
                      (S.mixed_large(pkg, 2000, S.MIXED_SEED, depth=1), pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_BOUNCE)):
        r = pkg.Renderer(sc, device=0, flags=flags)
        try:
            assert r.stream_cull and r.stream_cull_bounce is True
        finally:
            r.cleanup_update()


def test_without_the_environment_switch_there_are_no_work_words(pkg, monkeypatch):
    monkeypatch.delenv("MI355RT_STREAM_CULL_STATS", raising=False)
    r = pkg.Renderer(S.field(pkg, 129, S.FIELD_SEED, mirrors=True, depth=2), device=0, flags=three(pkg))
    try:
        assert r.stream_cull_bounce
        r.update()
        with pytest.raises(pkg.RtError) as e:
            r.stream_cull_bounce_stats()
        assert e.value.code == -1 and "MI355RT_STREAM_CULL_STATS" in e.value.message
    finally:
        r.cleanup_update()


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------
def test_statistics(pkg, monkeypatch):
    """[0] == D exactly (blocks x segments >= 1 with a bouncing lane, x 5 chunks); [0] - [1] >= L; fewer pairs reach than were asked; every
    query had a lane that can be culled for; cumulative over two frames; rt_debug_stream_cull's words are those of the context without the
    flag after the same frames.  (The oracle gives D = 100, L = 57 for this scene; an MI355X gave the
    words [100, 42, 980, 336, 0, 0, 0, 0] per frame.)"""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    e = B.expectation()
    assert e["L"] >= e["D"] / 4
    sc = B.bounce_scene(pkg)
    r = pkg.Renderer(sc, device=0, flags=three(pkg))
    p = pkg.Renderer(sc, device=0, flags=three(pkg) & ~pkg.RT_FLAG_STREAM_CULL_BOUNCE)
    try:
        assert r.stream_cull_bounce and r.stream_cull_bounce_stats() == [0] * 8
        r.update()
        p.update()
        w = r.stream_cull_bounce_stats()
        print("bounce work words", w, "expected", e)
        assert w[0] == e["D"], (w, e)
        assert w[0] - w[1] >= e["L"], (w, e)
        assert w[2] == e["rays"] * e["n_chunks"] and w[3] < w[2], (w, e)
        assert w[4] == 0 and w[5:] == [0, 0, 0]
        assert R.same_as_oracle(r.download()[..., :3], S.oracle_of(pkg, sc).render(nthreads=8))
        r.update()
        p.update()
        assert r.stream_cull_bounce_stats() == [2 * x for x in w]   # cumulative
        assert r.stream_cull_stats() == p.stream_cull_stats() and r.stream_cull_stats()[0] > 0
    finally:
        r.cleanup_update()
        p.cleanup_update()


# ---- rt_set_scene -------------------------------------------------------------------------------------------------------------------------
def test_set_scene_clusters_exchange_places(pkg):
    sc, moved = B.bounce_scene(pkg), B.bounce_scene(pkg, SWAPPED)
    a, coefs = sc.arrays(), moved.arrays()["coefs"]
    want = S.oracle_of(pkg, moved).render(nthreads=8)
    r = pkg.Renderer(sc, device=0, flags=three(pkg))
    try:
        assert r.stream_cull_bounce
        r.update()
        before = r.download().copy()
        r.set_scene(coefs=coefs)
        r.update()
        after = r.download().copy()
        assert r.set_scene_status()["applied"] == 1 and r.stream_cull_bounce
        held_to_the_lab(pkg, r, coefs, a)
    finally:
        r.cleanup_update()
    assert not R.same(after, before) and R.same_as_oracle(after[..., :3], want)


def test_set_scene_and_frame_in_one_graph_replayed_twice(pkg):
    import torch
    sc = B.bounce_scene(pkg)
    a = sc.arrays()
    steps = [B.bounce_scene(pkg, SWAPPED).arrays()["coefs"], a["coefs"]]
    want = [S.oracle_of(pkg, B.bounce_scene(pkg, SWAPPED)).render(nthreads=8), S.oracle_of(pkg, sc).render(nthreads=8)]
    assert not R.same(want[0], want[1])
    r = pkg.Renderer(sc, device=0, flags=three(pkg))
    s = torch.cuda.Stream()
    try:
        assert r.stream_cull_bounce
        r.update(stream=s.cuda_stream, timed=False)
        with torch.cuda.stream(s):
            arr = torch.from_numpy(steps[0].copy()).to("cuda:0")
            buf = torch.empty((r.local_rows, r.width, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            r.set_scene_into(coefs=arr.data_ptr(), stream=s.cuda_stream)
            r.update(dev_fb=buf.data_ptr(), stream=s.cuda_stream, timed=False)
        for rep in range(2):
            with torch.cuda.stream(s):
                arr.copy_(torch.from_numpy(steps[rep].copy()))
                buf.view(torch.int32).fill_(0x7FC00000)
                g.replay()
            s.synchronize()
            got = buf.cpu().numpy()
            assert np.all(got[..., 3] == 1.0) and R.same_as_oracle(got[..., :3], want[rep]), rep
        assert r.set_scene_status()["applied"] == 2
        del g
    finally:
        torch.cuda.synchronize()
        r.cleanup_update()


# ---- unchanged neighbours -----------------------------------------------------------------------------------------------------------------
def test_queries_on_a_flagged_context_are_the_unflagged_contexts(pkg):
    sc = S.field(pkg, 193, S.FIELD_SEED, mirrors=True, depth=2)
    rng = np.random.default_rng(3)
    o = np.zeros((300, 3)) + rng.normal(scale=0.05, size=(300, 3))
    d = np.stack([rng.uniform(-0.6, 0.6, 300), rng.uniform(-0.45, 0.45, 300), np.ones(300)], axis=1)
    out = []
    for flags in (three(pkg) | pkg.RT_FLAG_STREAM_QUERIES, pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_QUERIES):
        r = pkg.Renderer(sc, device=0, flags=flags)
        try:
            assert r.stream_cull_bounce == bool(flags & pkg.RT_FLAG_STREAM_CULL_BOUNCE) and r.streamed_queries
            rec = {}
            r.update()
            rec["frame 0"] = r.download().copy()
            g = r.gbuffer()
            rec["object"], rec["t"], rec["normal"] = (x.cpu().numpy() for x in g[:3])
            rec["trace"] = r.trace(o, d)
            rec["shade"] = r.shade(o, d)
            rec["segments"], rec["last"], rec["ends"] = r.paths(o, d)
            r.update()
            rec["frame 1"] = r.download().copy()
            out.append(rec)
        finally:
            r.cleanup_update()
    assert (out[0]["object"] >= 0).any() and (out[0]["trace"]["object"] >= 0).any()
    for key in out[0]:
        a, b = np.ascontiguousarray(out[0][key]), np.ascontiguousarray(out[1][key])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), key
    assert R.same(out[0]["frame 0"], out[0]["frame 1"])


def test_streamed_adaptive_frame_on_a_flagged_context(pkg):
    sc = S.field(pkg, 193, S.FIELD_SEED, mirrors=True, depth=2)
    base = pkg.RT_FLAG_STREAM | pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA_ADAPTIVE | pkg.RT_FLAG_STREAM_ADAPTIVE
    got = []
    for flags in (base | pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_BOUNCE, base | pkg.RT_FLAG_STREAM_CULL, base):
        r = pkg.Renderer(sc, device=0, flags=flags)
        try:
            assert r.stream_cull_bounce == bool(flags & pkg.RT_FLAG_STREAM_CULL_BOUNCE) and r.streamed_adaptive
            r.update()
            got.append((r.download().copy(), r.refined))
        finally:
            r.cleanup_update()
    assert got[0][1] == got[1][1] == got[2][1] > 0 and R.same(got[0][0], got[1][0]) and R.same(got[0][0], got[2][0])


# ---- init_update() / update() -----------------------------------------------------------------------------------------------------------------
ADAPTER = r"""
import ctypes as C, os, re, subprocess, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "tools"))
import __graft_entry__ as g
import stream_scenes as S
pkg = g.load_package()
sc = S.field(pkg, 193, S.FIELD_SEED, mirrors=True, depth=2)
want = S.oracle_of(pkg, sc).render(nthreads=8)
a = sc.arrays()
upd = C.CDLL(pkg.UPDATE_LIB_PATH)
names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
update = getattr(upd, re.search(r"\b(_Z\d+updateRKN3glm3matI\S*)\b", names).group(1))
cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
update.argtypes, update.restype = [C.c_void_p], C.c_float
upd.mi355rt_update_download.argtypes = [C.c_void_p, C.c_size_t]
cam = np.ascontiguousarray(pkg.IDENTITY, dtype=np.float64)
init(7, sc._h)
ms = update(cam.ctypes.data)
out = np.zeros((a["height"], a["width"], 4), np.float32)
rc = upd.mi355rt_update_download(out.ctypes.data_as(C.c_void_p), out.nbytes)
cleanup()
print("frame", rc, ms > 0.0, bool(np.array_equal(out[..., :3].view(np.uint32), want.view(np.uint32))), bool(np.all(out[..., 3] == 1.0)))
"""


def adapter(**env):
    return subprocess.run([sys.executable, "-c", ADAPTER, ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))


def test_init_update_with_the_environment_switch():
    """The reference's back-end contract in a fresh process, on a mirrored field of four chunks: all three switches, the frame is the oracle's."""
    out = adapter(MI355RT_STREAM="1", MI355RT_STREAM_CULL="1", MI355RT_STREAM_CULL_BOUNCE="1")
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "frame 0 True True True", out.stdout
    out = adapter(MI355RT_STREAM="1", MI355RT_STREAM_CULL_BOUNCE="1")      # (the switch without MI355RT_STREAM_CULL: simply nothing)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "frame 0 True True True", out.stdout
    out = adapter(MI355RT_STREAM_CULL_BOUNCE="yes")
    assert out.returncode != 0 and "mi355rt: MI355RT_STREAM_CULL_BOUNCE: expected 0 or 1" in out.stderr, (out.stdout, out.stderr)
