"""Culled streamed frames on the GPU (RT_FLAG_STREAM_CULL; csrc/rt_stream_cull.hip).  The frame is RT_FLAG_STREAM's
frame by definition: every strict frame of degree <= 2 here is compared bit for bit with the CPU oracle (both formats) AND with the
context without the flag.  The host-side conditions (the scene image, the predicates about bounds, the statistics scene's L >= D / 4)
are in tests/test_stream_cull_host.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, compare, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cubic_device_lab as D  # noqa: E402
import cull_lab as L  # noqa: E402
import raw_desc_scenes as R  # noqa: E402
import ssaa_ref  # noqa: E402
import stream_cull_lab as SC  # noqa: E402
import stream_scenes as S  # noqa: E402
from test_raw_descriptor_gpu import rgba8_of  # noqa: E402
from test_stream_cull_host import raw_scene_with_unbounded_spheres  # noqa: E402
from test_stream_gpu import CUBIC, MOVED, QUADRIC, large_n, large_want, shade_of_primary, shipped, shipped_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

F32, U8 = 0, 1


@pytest.fixture(autouse=True)
def the_feature(pkg):
    assert pkg.RT_FLAG_STREAM_CULL == 524288


def both(pkg):
    return pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL


def frame(pkg, sc, cam=None, expect_cull=True, **kw):
    r = pkg.Renderer(sc, device=0, **kw)
    try:
        assert r.stream_cull == expect_cull, (r.stream_cull, r.streamed)
        assert (r.stream_bounds().size > 0) == expect_cull
        r.update(cam)
        return r.download()
    finally:
        r.cleanup_update()


def check(pkg, sc, want, what, cam=None, flags=None, plain_flags=None, expect_cull=True, **kw):
    """Flagged RGBA32F == oracle == unflagged; flagged RGBA8 == the oracle's quantisation == unflagged."""
    flags = both(pkg) if flags is None else flags
    plain_flags = (flags & ~pkg.RT_FLAG_STREAM_CULL) if plain_flags is None else plain_flags
    got = frame(pkg, sc, cam, expect_cull, flags=flags, **kw)
    assert np.all(got[..., 3] == 1.0) and R.same_as_oracle(got[..., :3], want), (what, R.n_diff(got[..., :3], want))
    assert R.same(got, frame(pkg, sc, cam, False, flags=plain_flags, **kw)), what
    got8 = frame(pkg, sc, cam, expect_cull, flags=flags, fmt=pkg.RT_FMT_RGBA8, **kw)
    q, ok = rgba8_of(want)
    assert got8.dtype == np.uint8 and not ((got8 != q)[..., :3] & ok).any() and np.all(got8[..., 3] == 255), what
    assert R.same(got8, frame(pkg, sc, cam, False, flags=plain_flags, fmt=pkg.RT_FMT_RGBA8, **kw)), what


# ---- sphere counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.COUNTS)
def test_sphere_counts(pkg, n):
    """1 .. 193 spheres: below four bounded spheres culling is off and so is the decision; from 65 on there are several chunks."""
    on = n >= 4
    for mirrors, depth in ((False, 0), (True, 2)):
        sc = S.field(pkg, n, S.FIELD_SEED, mirrors=mirrors, depth=depth)
        check(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), (n, mirrors, depth), expect_cull=on)
    sc = S.field(pkg, n, S.FIELD_SEED, w=37, h=21, mirrors=True, depth=1)
    check(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), (n, "37 x 21"), expect_cull=on)


def test_large_field_with_the_flag_alone_and_with_simple(pkg):
    """The first count beyond the LDS limit plus the large last sphere whose shadow falls on the field: streamed without being asked."""
    sc = S.field(pkg, large_n(), S.LARGE_SEED, big_last=True)
    check(pkg, sc, large_want(), "large field", flags=pkg.RT_FLAG_STREAM_CULL)
    got = frame(pkg, sc, flags=pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_SIMPLE)
    assert R.same_as_oracle(got[..., :3], large_want())


# ---- other scene kinds --------------------------------------------------------------------------------------------------------------------
def test_large_mixed_scene_with_mirrors(pkg):
    sc = S.mixed_large(pkg, 2000, S.MIXED_SEED)
    check(pkg, sc, S.oracle_of(pkg, sc).render(nthreads=8), "large mixed", flags=pkg.RT_FLAG_STREAM_CULL)


@pytest.mark.parametrize("seed", range(8))
def test_raw_descriptor_scenes(pkg, seed):
    """Odd light vectors, non-finite colours and ratios, moved cameras (tests/tools/raw_desc_scenes.py)."""
    osc, cam = R.scene(seed)
    osc.width, osc.height = min(osc.width, 80), min(osc.height, 60)
    d = R.desc(pkg, osc)
    _, _, w = SC.image(SC.arrays_of_oracle(osc))
    check(pkg, d, osc.render(cam=cam, nthreads=8), ("raw", seed), cam=cam, expect_cull=bool(w["cull"]))


def test_named_raw_descriptor_scenes(pkg):
    """Every named oddity of the sphere classes: |d|^2 at and below EPS, NaN / inf directions and colours, non-finite albedos."""
    names = [n for n in sorted(R.NAMED) if R.NAMED[n][0] in ("lean", "lean65", "mirror")]
    assert len(names) >= 8
    culled = 0
    for name in names[::max(1, len(names) // 16)]:
        osc, _, cams = R.named(name)
        osc.width, osc.height = min(osc.width, 64), min(osc.height, 48)
        _, _, w = SC.image(SC.arrays_of_oracle(osc))
        culled += w["cull"]
        check(pkg, R.desc(pkg, osc), osc.render(cam=cams[0], nthreads=8), name, cam=cams[0], expect_cull=bool(w["cull"]))
    assert culled >= 4


def test_spheres_without_a_radius(pkg):
    a = raw_scene_with_unbounded_spheres()
    d = pkg.desc_from_arrays(64, 48, np.radians(S.FOV), (0.05, 0.1, 0.2), 0, a["coefs"], a["reflection"], a["albedo"], a["light_is_spherical"], a["light_p"], a["light_color"])
    osc = S.O.Scene(64, 48, 0.0, 0, (0.05, 0.1, 0.2))
    osc.vertical_fov = float(np.radians(S.FOV))
    for i in range(len(a["reflection"])):
        osc.add_object(a["coefs"][i], a["albedo"][i], a["reflection"][i])
    for i in range(2):
        osc.lights.append(R.stored_light(a["light_is_spherical"][i], a["light_p"][i], a["light_color"][i]))
    check(pkg, d, osc.render(nthreads=8), "unbounded tail")
    r = pkg.Renderer(d, device=0, flags=both(pkg))
    try:
        b = r.stream_bounds().view(SC.US_DTYPE)
        assert len(b) == 3 and np.isfinite(b["r"][:2]).all() and np.isposinf(b["r"][2])
    finally:
        r.cleanup_update()


@pytest.mark.parametrize("i", range(0, L.N_GRAZE_SCENES, 2))
def test_grazing_scenes(pkg, i):
    """cull_lab's scenes with spheres tangent to a block's cone or a chunk's shadow volume -- and the same scene with a far cluster of 70
    spheres, so that the tangent spheres sit on the rim of a chunk of many members."""
    spec = L.graze_scene_spec(i)
    osc = L.spec_to_oracle(spec)
    check(pkg, R.desc(pkg, osc), osc.render(nthreads=8), ("graze", i))
    rng = np.random.default_rng(i)
    far = np.array([40.0, 30.0, 20.0]) * rng.choice([-1.0, 1.0], 3) * rng.uniform(0.5, 1.5)
    rim = dict(spec, spheres=spec["spheres"] + [(tuple(far + rng.normal(scale=1.0, size=3)), 0.3, (0.5, 0.5, 0.5)) for _ in range(70)])
    osc = L.spec_to_oracle(rim)
    check(pkg, R.desc(pkg, osc), osc.render(nthreads=8), ("graze, chunk rim", i))


# ---- shipped scenes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QUADRIC)
def test_shipped_quadric_scenes(pkg, name):
    sc = shipped(pkg, name, 96, 72, 4)
    on = bool(SC.image(sc.arrays())[2]["cull"])   # (culling is on from four bounded spheres: 20spheres)
    assert on == (name == "20spheres")
    for cam in (None, pkg.camera_matrix(*MOVED)):
        a = frame(pkg, sc, cam, expect_cull=on, flags=both(pkg))
        assert R.same(a, frame(pkg, sc, cam, False, flags=pkg.RT_FLAG_STREAM)), name


@pytest.mark.parametrize("name", CUBIC)
def test_shipped_cubic_scenes(pkg, oracle, name):
    """== rt_shade_rays(rt_primary_rays) bit for bit, == the unflagged frame, and within the cubic bar of tests/test_stream_gpu.py."""
    w, h = 80, 60
    sc = shipped(pkg, name, w, h, 4)
    r = pkg.Renderer(sc, device=0, flags=both(pkg))
    try:
        on = r.stream_cull
        r.update()
        got = r.download().copy()
        assert R.same(got, shade_of_primary(pkg, r))
    finally:
        r.cleanup_update()
    assert R.same(got, frame(pkg, sc, None, False, flags=pkg.RT_FLAG_STREAM))
    got = frame(pkg, shipped(pkg, name, w, h), None, on, flags=both(pkg))
    c = compare(got[..., :3], shipped_oracle(name, w, h))
    assert c["n_bad_pixels"] <= max(3, int(0.002 * w * h)), c
    c = D.compare_device_libm(pkg, got[..., :3], oracle.load_scene(scene_path(name)).with_size(w, h))
    assert c["n_bad_pixels"] == 0, c


# ---- context kinds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [F32, U8], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("k", [2, 4])
def test_supersampling(pkg, k, fmt):
    w, h = 40, 30
    flag = pkg.RT_FLAG_SSAA2 if k == 2 else pkg.RT_FLAG_SSAA4
    sc = S.field(pkg, 129, S.FIELD_SEED, w=w, h=h, mirrors=True, depth=1)
    want = ssaa_ref.resolve(S.oracle_of(pkg, sc).with_size(k * w, k * h).render(nthreads=8), k)   # (the same scene on the k-times finer grid)
    want = ssaa_ref.quantise(want) if fmt == U8 else want
    got = frame(pkg, sc, flags=both(pkg) | flag, fmt=fmt)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert R.same(got, frame(pkg, sc, None, False, flags=pkg.RT_FLAG_STREAM | flag, fmt=fmt))


def test_rank_1_of_3_with_bands_of_8(pkg):
    sc = S.field(pkg, 193, S.FIELD_SEED, w=64, h=50, mirrors=True, depth=1)
    want = S.oracle_of(pkg, sc).render(nthreads=8)
    r = pkg.Renderer(sc, device=0, rank=1, world=3, band_rows=8, flags=both(pkg))
    try:
        assert r.stream_cull
        r.update()
        rows = r.row_map()
        assert 0 < len(rows) < 50 and R.same_as_oracle(r.download()[..., :3], want[rows])
    finally:
        r.cleanup_update()


def test_rotated_and_moved_camera(pkg):
    sc = S.field(pkg, large_n(), S.LARGE_SEED, big_last=True)
    for cam in (pkg.camera_matrix((0.5, 0.3, -1.0), 88.0, 2.0), pkg.camera_matrix((6.0, 2.0, 4.0), 120.0, -9.0)):
        check(pkg, sc, S.oracle_of(pkg, sc).render(cam=cam, nthreads=8), "moved", cam=cam, flags=pkg.RT_FLAG_STREAM_CULL)


def test_fast_variant_to_its_bar(pkg):
    """RT_FLAG_FAST: 1e-5 relative, at most max(2, 0.2 % of the pixels) beyond it -- and the unflagged FAST frame bit for bit (the same
    arithmetic per tested object)."""
    for sc, want in ((S.field(pkg, large_n(), S.LARGE_SEED, big_last=True), large_want()),
                     (shipped(pkg, "20spheres", 64, 48, 4), shipped_oracle("20spheres", 64, 48, 4))):
        got = frame(pkg, sc, flags=both(pkg) | pkg.RT_FLAG_FAST)
        c = compare(got[..., :3], want)
        assert c["n_bad_pixels"] <= max(2, int(0.002 * 64 * 48)), c
        assert R.same(got, frame(pkg, sc, None, False, flags=pkg.RT_FLAG_STREAM | pkg.RT_FLAG_FAST))


@pytest.mark.parametrize("transport", ["dense", "sparse"])
def test_multi_renderer(pkg, transport):
    extra = pkg.RT_MULTI_SPARSE if transport == "sparse" else 0
    m = pkg.MultiRenderer(S.field(pkg, large_n(), S.LARGE_SEED, big_last=True), [0, 0], band_rows=8, parts=2, flags=pkg.RT_FLAG_STREAM_CULL | extra)
    try:
        for _ in range(2):
            m.update()
        assert R.same_as_oracle(m.download()[..., :3], large_want()), transport
    finally:
        m.cleanup_update()


# ---- the decision -------------------------------------------------------------------------------------------------------------------------
def test_decision_false_is_the_context_without_the_flag(pkg, monkeypatch):
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    sc = S.field(pkg, 129, S.FIELD_SEED, mirrors=True, depth=1)
    for flags, plain in ((both(pkg) | pkg.RT_FLAG_NOCULL, pkg.RT_FLAG_STREAM | pkg.RT_FLAG_NOCULL), (pkg.RT_FLAG_STREAM_CULL, 0)):
        r, p = pkg.Renderer(sc, device=0, flags=flags), pkg.Renderer(sc, device=0, flags=plain)
        try:
            assert r.stream_cull is False and r.stream_bounds().size == 0 and r.streamed == p.streamed == bool(flags & pkg.RT_FLAG_STREAM)
            with pytest.raises(pkg.RtError) as e:
                r.stream_cull_stats()
            assert e.value.code == -1 and "rt_debug_stream_cull" in e.value.message
            assert R.same(r.debug_scene_blob(), p.debug_scene_blob())
            for _ in range(2):
                r.update()
                p.update()
            assert R.same(r.download(), p.download())
        finally:
            r.cleanup_update()
            p.cleanup_update()


def test_without_the_environment_switch_there_are_no_work_words(pkg, monkeypatch):
    monkeypatch.delenv("MI355RT_STREAM_CULL_STATS", raising=False)
    r = pkg.Renderer(S.field(pkg, 129, S.FIELD_SEED), device=0, flags=both(pkg))
    try:
        assert r.stream_cull
        r.update()
        with pytest.raises(pkg.RtError) as e:
            r.stream_cull_stats()
        assert e.value.code == -1
    finally:
        r.cleanup_update()


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expectation():
    import __graft_entry__ as graft
    pkg = graft.load_package()
    return SC.stats_expectation(pkg, SC.cluster_scene(pkg))


def test_statistics(pkg, monkeypatch):
    """Word [2] == D exactly (blocks with a hit x lights x chunks: one segment, both lights culled for, five chunks in one group);
    [2] - [3] >= L; fewer primary chunks staged than decided; fewer entries swept than decided; nothing ran unculled."""
    monkeypatch.setenv("MI355RT_STREAM_CULL_STATS", "1")
    e = expectation()
    assert e["L"] >= e["D"] / 4
    sc = SC.cluster_scene(pkg)
    r = pkg.Renderer(sc, device=0, flags=both(pkg))
    try:
        assert r.stream_cull_stats() == [0] * 8
        r.update()
        w = r.stream_cull_stats()
        print("work words", w, "expected", e)
        assert w[0] == 48 * e["n_chunks"] and w[1] < w[0]
        assert w[2] == e["D"] and w[2] - w[3] >= e["L"]
        assert w[5] < w[4] <= 64 * w[3] and w[6] == 0 and w[7] == 0
        assert R.same_as_oracle(r.download()[..., :3], S.oracle_of(pkg, sc).render(nthreads=8))
        r.update()
        assert r.stream_cull_stats() == [2 * x for x in w]   # cumulative
    finally:
        r.cleanup_update()


# ---- rt_set_scene -------------------------------------------------------------------------------------------------------------------------
SWAPPED = (SC.CLUSTERS[1][0], SC.CLUSTERS[0][0], (3.0, -6.0, 23.0))


def held_to_the_lab(pkg, r, coefs, a):
    """The device's blob and bounds == what the host packs for the new scene under the context's order."""
    got = r.debug_scene_blob()
    t = got[r_off(a):r_off(a) + 64 * len(a["reflection"])].view(SC.US_DTYPE)
    blob, bounds, w = SC.image(dict(a, coefs=coefs), slot_orig=t["orig"])
    assert w["n_us"] == len(a["reflection"])
    assert R.same(got[:blob.size], blob) and R.same(r.stream_bounds(), bounds)


def r_off(a):
    return SC.image(a)[2]["off_us"]


def test_set_scene_clusters_exchange_places(pkg):
    sc, moved = SC.cluster_scene(pkg), SC.cluster_scene(pkg, SWAPPED)
    a, coefs = sc.arrays(), moved.arrays()["coefs"]
    want = S.oracle_of(pkg, moved).render(nthreads=8)
    r = pkg.Renderer(sc, device=0, flags=both(pkg))
    try:
        r.update()
        before, old_bounds = r.download().copy(), r.stream_bounds().copy()
        held_to_the_lab(pkg, r, a["coefs"], a)
        r.set_scene(coefs=coefs)
        r.update()
        after = r.download().copy()
        assert r.set_scene_status()["applied"] == 1
        assert not R.same(r.stream_bounds(), old_bounds)
        held_to_the_lab(pkg, r, coefs, a)
    finally:
        r.cleanup_update()
    assert not R.same(after, before) and R.same_as_oracle(after[..., :3], want)
    assert R.same(after, frame(pkg, moved, flags=both(pkg)))


def test_set_scene_and_frame_in_one_graph_replayed_twice(pkg):
    import torch
    sc = SC.cluster_scene(pkg)
    a = sc.arrays()
    steps = [SC.cluster_scene(pkg, SWAPPED).arrays()["coefs"], a["coefs"]]
    want = [frame(pkg, SC.cluster_scene(pkg, SWAPPED), flags=both(pkg)), frame(pkg, sc, flags=both(pkg))]
    assert not R.same(want[0], want[1])
    r = pkg.Renderer(sc, device=0, flags=both(pkg))
    s = torch.cuda.Stream()
    try:
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
            assert R.same(buf.cpu().numpy(), want[rep]), rep
            held_to_the_lab(pkg, r, steps[rep], a)
        assert r.set_scene_status()["applied"] == 2
        del g
    finally:
        torch.cuda.synchronize()
        r.cleanup_update()


# ---- the other readers of the reordered table -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("queries", ["staged", "streamed"])
def test_queries_on_a_flagged_context_are_the_unflagged_contexts(pkg, queries):
    """rt_render_gbuffer, rt_trace_rays, rt_shade_rays and rt_trace_paths between frames: their records are the unflagged context's bit for
    bit (the nearest-hit rule does not depend on the table's order), and the frames stay what they are."""
    sc = S.field(pkg, 193, S.FIELD_SEED, mirrors=True, depth=2)
    extra = pkg.RT_FLAG_STREAM_QUERIES if queries == "streamed" else 0
    rng = np.random.default_rng(3)
    o = np.zeros((300, 3)) + rng.normal(scale=0.05, size=(300, 3))
    d = np.stack([rng.uniform(-0.6, 0.6, 300), rng.uniform(-0.45, 0.45, 300), np.ones(300)], axis=1)
    out = []
    for flags in (both(pkg) | extra, pkg.RT_FLAG_STREAM | extra):
        r = pkg.Renderer(sc, device=0, flags=flags)
        try:
            assert r.stream_cull == bool(flags & pkg.RT_FLAG_STREAM_CULL) and r.streamed_queries == (queries == "streamed")
            rec = {}
            r.update()
            rec["frame 0"] = r.download().copy()
            g = r.gbuffer()
            rec["object"], rec["t"], rec["normal"] = (x.cpu().numpy() for x in g[:3])
            r.update()
            rec["frame 1"] = r.download().copy()
            rec["trace"] = r.trace(o, d)
            rec["shade"] = r.shade(o, d)
            seg, last, ends = r.paths(o, d)
            rec["segments"], rec["last"], rec["ends"] = seg, last, ends
            r.update()
            rec["frame 2"] = r.download().copy()
            out.append(rec)
        finally:
            r.cleanup_update()
    assert (out[0]["object"] >= 0).any() and (out[0]["trace"]["object"] >= 0).any()
    for key in out[0]:
        a, b = np.ascontiguousarray(out[0][key]), np.ascontiguousarray(out[1][key])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), key
    assert R.same(out[0]["frame 0"], out[0]["frame 2"])


def test_streamed_adaptive_frame_on_a_flagged_context(pkg):
    sc = S.field(pkg, 193, S.FIELD_SEED, mirrors=True, depth=1)
    base = pkg.RT_FLAG_STREAM | pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA_ADAPTIVE | pkg.RT_FLAG_STREAM_ADAPTIVE
    got = []
    for flags in (base | pkg.RT_FLAG_STREAM_CULL, base):
        r = pkg.Renderer(sc, device=0, flags=flags)
        try:
            assert r.stream_cull == bool(flags & pkg.RT_FLAG_STREAM_CULL) and r.streamed_adaptive
            r.update()
            got.append((r.download().copy(), r.refined))
        finally:
            r.cleanup_update()
    assert got[0][1] == got[1][1] > 0 and R.same(got[0][0], got[1][0])


# ---- init_update() / update() -----------------------------------------------------------------------------------------------------------------
def test_init_update_with_the_environment_switch():
    from test_stream_gpu import adapter
    out = adapter("field", MI355RT_STREAM_CULL="1")
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "frame 0 True True True", out.stdout
    out = adapter(scene_path("20spheres"), MI355RT_STREAM="1", MI355RT_STREAM_CULL="1")
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "frame 0 True True True", out.stdout
    out = adapter(scene_path("quadratic"), MI355RT_STREAM_CULL="yes")
    assert out.returncode != 0 and "mi355rt: MI355RT_STREAM_CULL: expected 0 or 1" in out.stderr, (out.stdout, out.stderr)
