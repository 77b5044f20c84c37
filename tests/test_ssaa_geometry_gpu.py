"""Geometric edges for adaptive supersampling (RT_FLAG_SSAA_GEOMETRY) on the GPU.

Strict contexts, degree <= 2: every frame == ssaa_geometry_ref.compose of the oracle's P (W x H), S (kW x kH), object ids and
normals (tests/tools/gbuffer_ref.py), bit for bit, for k in {2, 4}, tau in {-1, 0, 1/32, +inf}, min_cos in {-inf, 0.5, 0.999} and
both formats (RGBA8: the reference's quantisation of the composed frame, exactly); rt_get_ssaa_refined == the mask's popcount;
the work counters == the oracle's composition with the new mask.  Ranks, the multi layer, alternating streams, a captured graph,
update().  FAST contexts and degree 3: ids and normals from Renderer.gbuffer() of a k = 1 sibling (the same kernel), P from its
render; the refined SET must be geo_mask | refine_mask of those exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, compare, scene_path
from test_gpu_parity import oracle_from, random_cubic_scene
from test_ssaa_adaptive_fuzz_gpu import (COUNT_KEY, COUNTED, _oracle_counts, _sum, build, identical, mismatch, oracle_frame, rows_counts,
                                         sample_counts)
from test_ssaa_adaptive_gpu import EXE, F32, POSES, U8, ada_flags, kflag, scene
from test_ssaa_geometry_host import lightless_scene

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gbuffer_ref  # noqa: E402
import ssaa_adaptive_ref as ada  # noqa: E402
import ssaa_geometry_ref as geo  # noqa: E402
import ssaa_ref  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
TAUS = (-1.0, 0.0, 1.0 / 32.0, INF)
COSES = (-INF, 0.5, 0.999)
_G = {}


def gflags(pkg, k, extra=0):
    return ada_flags(pkg, k, pkg.RT_FLAG_SSAA_GEOMETRY | extra)


def _oracle():
    import __graft_entry__ as graft
    return graft.load_oracle()


def _pkg():
    import __graft_entry__ as graft
    return graft.load_package()


def build_any(key):
    """The adaptive fuzz test's scenes by key, plus ("shipped", name, w, h) and ("lightless",)."""
    pkg, oracle = _pkg(), _oracle()
    if key[0] == "shipped":
        sc = scene(pkg, key[1], key[2], key[3], 4)
        return sc, oracle.load_scene(scene_path(key[1])).with_size(key[2], key[3], 4), None
    if key[0] == "lightless":
        sc = lightless_scene(pkg, 56, 40)
        return sc, oracle_from(pkg, oracle, sc), None
    return build(key)


def frames(key, k):
    """(P, S, obj, N) of the oracle for scene `key`."""
    if (key, k) not in _G:
        _, osc, cam = build_any(key)
        if key not in _G:
            g = gbuffer_ref.compose(osc, cam)
            _G[key] = (osc.render(cam=cam, nthreads=8), g["object"], g["normal"])
        s = osc.with_size(k * osc.width, k * osc.height).render(cam=cam, nthreads=8)
        _G[(key, k)] = s
    p, obj, nrm = _G[key]
    return p, _G[(key, k)], obj, nrm


def want_frame(p, s, k, tau, obj, nrm, c, fmt):
    out = geo.compose(p, s, k, tau, obj, nrm, c)
    return ssaa_ref.quantise(out) if fmt == U8 else out


def full_mask(p, tau, obj, nrm, c):
    return ada.refine_mask(p, tau) | geo.geo_mask(obj, nrm, c)


def check_scene(pkg, key, ks=(2, 4), fmts=(F32, U8), taus=TAUS, coses=COSES, extra=0):
    """One context per (k, format); every (tau, min_cos) is a further frame of it."""
    sc, _, cam = build_any(key)
    for k in ks:
        p, s, obj, nrm = frames(key, k)
        for fmt in fmts:
            r = pkg.Renderer(sc, device=0, flags=gflags(pkg, k, extra), fmt=fmt)
            try:
                for tau in taus:
                    for c in coses:
                        r.set_ssaa_threshold(tau)
                        r.set_ssaa_geometry(c)
                        r.update(cam)
                        got, n = r.download(), r.refined
                        want = want_frame(p, s, k, tau, obj, nrm, c, fmt)
                        assert identical(got, want), (key, k, fmt, tau, c, mismatch(got, want))
                        assert n == int(full_mask(p, tau, obj, nrm, c).sum()), (key, k, fmt, tau, c, n)
            finally:
                r.cleanup_update()


# 1. strict, degree <= 2, against the oracle
@pytest.mark.parametrize("name", ["quadratic", "20spheres", "reflection_test"])
def test_shipped_scenes(pkg, name):
    check_scene(pkg, ("shipped", name, 64, 48))


def test_lightless_scene(pkg):
    """No lights, black background: the colour term refines nothing at any tau >= 0, the geometric one exactly the silhouettes."""
    key = ("lightless",)
    p, _, obj, nrm = frames(key, 2)
    assert not ada.refine_mask(p, 0.0).any() and geo.geo_mask(obj, nrm, -INF).any()
    check_scene(pkg, key)


RANDOM = [("random", 9701, 12, 4, True, True, 64, 48, 1), ("random", 9702, 65, 3, False, False, 48, 36, 4), ("random", 9703, 130, 2, True, True, 40, 30, 6)]


@pytest.mark.parametrize("key", RANDOM, ids=[f"n{k[2]}" for k in RANDOM])
def test_random_sphere_fields(pkg, key):
    i = RANDOM.index(key)
    check_scene(pkg, key, ks=((2, 4)[i % 2],), fmts=((F32, U8)[i // 2 % 2],))
    check_scene(pkg, key, ks=((4, 2)[i % 2],), fmts=(F32,), taus=(1.0 / 32.0,), coses=(0.999,))


@pytest.mark.parametrize("seed", [0, 3, 5])
def test_mixed_class_scenes(pkg, seed):
    check_scene(pkg, ("mixed", seed, 64, 48), ks=(2 if seed % 2 else 4,), fmts=(U8 if seed == 5 else F32,))


@pytest.mark.parametrize("seed", [158, 2007, 2021, 2045])
def test_fuzz_scenes(pkg, seed):
    """The fuzzer's scenes: random sizes from 1 x 1 up, random (also sheared) camera matrices."""
    check_scene(pkg, ("fuzz", seed), ks=(4 if seed % 3 == 0 else 2,), fmts=(F32,))


@pytest.mark.parametrize("name", ["no_objects", "no_lights", "1x1", "3x1", "1x5", "camera_inside_sphere", "nested_spheres", "quadrics_and_planes_moved",
                                  "two_mirrors_depth_1"])
def test_edge_scenes(pkg, name):
    check_scene(pkg, ("edge", name), ks=(4,), fmts=(F32,), taus=(-1.0, 1.0 / 32.0, INF))
    check_scene(pkg, ("edge", name), ks=(2,), fmts=(U8,), taus=(0.0,), coses=(-INF, 0.999))


# 2. three frames with a camera cut, alternating streams, a captured graph of three frames with differing cameras
def _cam_frames(key, cams, k):
    _, osc, _ = build_any(key)
    out = []
    for cam in cams:
        g = gbuffer_ref.compose(osc, cam)
        out.append((osc.render(cam=cam, nthreads=8), osc.with_size(k * osc.width, k * osc.height).render(cam=cam, nthreads=8), g["object"], g["normal"]))
    return out


def test_camera_cut_streams_and_graph(pkg):
    import torch
    key, k, tau, c = ("shipped", "20spheres", 64, 48), 4, 1.0 / 32.0, 0.999
    sc, _, _ = build_any(key)
    cams = [pkg.camera_matrix(*p) for p in POSES + [((0.5, 0.0, 1.0), 95.0, 3.0)]]
    ref = _cam_frames(key, cams, k)
    wants = [want_frame(p, s, k, tau, o, n, c, F32) for p, s, o, n in ref]
    masks = [int(full_mask(p, tau, o, n, c).sum()) for p, s, o, n in ref]
    r = pkg.Renderer(sc, device=0, flags=gflags(pkg, k), ssaa_threshold=tau, ssaa_min_cos=c)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for j, i in enumerate((0, 0, 1, 2, 0)):                     # two frames of one pose, a cut, another, back: on alternating streams
        r.update(cams[i], stream=streams[j % 2].cuda_stream)
        assert identical(r.download(), wants[i]) and r.refined == masks[i], i
    r.cleanup_update()
    r = pkg.Renderer(sc, device=0, flags=gflags(pkg, k), ssaa_threshold=tau, ssaa_min_cos=c)
    bufs = [torch.zeros((48, 64, 4), dtype=torch.float32, device="cuda:0") for _ in cams]
    s = streams[0]
    r.update(cams[0], stream=s.cuda_stream, timed=False)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for cam, buf in zip(cams, bufs):
            r.update(cam, dev_fb=buf.data_ptr(), stream=s.cuda_stream, timed=False)
    r.set_ssaa_geometry(-INF)    # (the graph keeps the values it was captured with)
    r.set_ssaa_threshold(-1.0)
    g.replay()
    torch.cuda.synchronize()
    for i, buf in enumerate(bufs):
        assert identical(buf.cpu().numpy(), wants[i]), i
    del g
    r.cleanup_update()


# 3. counters: the oracle's P, plus the k^2 samples of every refined pixel of the NEW mask; the G pass books nothing
def test_counters_against_the_oracle(pkg):
    sc, _, cam = build(COUNT_KEY)
    p, pc = oracle_frame(COUNT_KEY, 1, True)
    _, _, obj, nrm = frames(COUNT_KEY, 2)
    for k, tau, c in ((2, 1.0 / 32.0, -INF), (4, INF, 0.999), (2, -1.0, 0.5)):
        r = pkg.Renderer(sc, device=0, flags=gflags(pkg, k, pkg.RT_FLAG_COUNT), ssaa_threshold=tau, ssaa_min_cos=c)
        r.update(cam)
        n, got = r.refined, r.counters()
        r.cleanup_update()
        mask = full_mask(p, tau, obj, nrm, c)
        assert n == int(mask.sum())
        want = _sum(_oracle_counts(pc), sample_counts(COUNT_KEY, k, mask))
        assert {x: got[x] for x in COUNTED} == want, (k, tau, c, {x: (got[x], want[x]) for x in COUNTED if got[x] != want[x]})
        assert got["primary_rays"] == p.shape[0] * p.shape[1] + k * k * n


def test_counters_of_a_banded_frame(pkg):
    world, band, k, tau, c = 3, 4, 2, INF, -INF
    sc, _, cam = build(COUNT_KEY)
    p, _, obj, nrm = frames(COUNT_KEY, k)
    h = p.shape[0]
    mask = full_mask(p, tau, obj, nrm, c)
    for rank in range(world):
        rows = pkg.band_rows_of_rank(h, band, world, rank)
        halo = []
        for b0 in range(0, len(rows), band):
            g0, g1 = int(rows[b0]), int(rows[min(b0 + band, len(rows)) - 1])
            halo += [g for g in (g0 - 1, g1 + 1) if 0 <= g < h]
        lm = np.zeros_like(mask)
        lm[rows] = mask[rows]
        r = pkg.Renderer(sc, device=0, rank=rank, world=world, band_rows=band, flags=gflags(pkg, k, pkg.RT_FLAG_COUNT), ssaa_threshold=tau, ssaa_min_cos=c)
        r.update(cam)
        n, got = r.refined, r.counters()
        r.cleanup_update()
        assert n == int(lm.sum()), rank
        want = _sum(rows_counts(COUNT_KEY, rows), rows_counts(COUNT_KEY, halo), sample_counts(COUNT_KEY, k, lm))
        assert {x: got[x] for x in COUNTED} == want, (rank, {x: (got[x], want[x]) for x in COUNTED if got[x] != want[x]})


# 4. ranks: the rows assembled by rt_row_map == the single-context frame (itself == the oracle's composition)
def band_edge_scene(pkg, w=48, h=40):
    """A plane whose horizon is the boundary between image rows 19 and 20 -- along a band edge for bands of 1 and 5 rows, inside a
    band of 8 -- in front of nothing, no lights, black background; and a sphere cut by it."""
    s = pkg.Scene.new(w, h, 50.0, 1, (0.0, 0.0, 0.0))
    s.add_object(pkg.surface_make("plane", [0, -1, 0], [0, 1, 0]), (0.5, 0.5, 0.5))
    s.add_object(pkg.surface_make("sphere", [1.0, 0.5, 8], [1.5]), (0.5, 0.5, 0.5))
    return s


@pytest.mark.parametrize("band", [1, 5, 8])
@pytest.mark.parametrize("world", [2, 3])
def test_ranks(pkg, world, band):
    oracle = _oracle()
    k, fmt = (2, 4)[(world + band) % 2], (F32, U8)[band % 2]
    for sc, cam, tau, c in ((band_edge_scene(pkg), pkg.camera_matrix((0.0, 0.3, 0.0), 90.0, 0.0), INF, -INF),
                            (band_edge_scene(pkg), None, INF, 0.999),
                            (scene(pkg, "reflection_test", 50, 43, 4), None, 1.0 / 32.0, 0.999)):
        osc = oracle_from(pkg, oracle, sc)
        g = gbuffer_ref.compose(osc, cam)
        p, s = osc.render(cam=cam, nthreads=8), osc.with_size(k * osc.width, k * osc.height).render(cam=cam, nthreads=8)
        want = want_frame(p, s, k, tau, g["object"], g["normal"], c, fmt)
        mask = full_mask(p, tau, g["object"], g["normal"], c)
        assert mask.any() and not mask.all()
        h = osc.height
        single = pkg.Renderer(sc, device=0, flags=gflags(pkg, k), fmt=fmt, ssaa_threshold=tau, ssaa_min_cos=c)
        single.update(cam)
        whole = single.download()
        single.cleanup_update()
        assert identical(whole, want), mismatch(whole, want)
        full = np.zeros_like(whole)
        seen = np.zeros(h, dtype=bool)
        for rank in range(world):
            r = pkg.Renderer(sc, device=0, rank=rank, world=world, band_rows=band, flags=gflags(pkg, k), fmt=fmt, ssaa_threshold=tau, ssaa_min_cos=c)
            r.update(cam)
            rows = r.row_map()
            got = r.download()
            assert r.refined == int(mask[rows].sum()), (rank, r.refined)
            r.cleanup_update()
            full[rows] = got
            seen[rows] = True
        assert seen.all() and identical(full, whole), (world, band, mismatch(full, whole))


def test_band_edge_scene_has_a_silhouette_along_band_edges(pkg):
    """What test_ranks relies on: at the identity camera the plane's horizon lies between rows 19 and 20 (bands of 1 and 5 rows end
    there), and the colour term sees none of it."""
    sc = band_edge_scene(pkg)
    osc = oracle_from(pkg, _oracle(), sc)
    g = gbuffer_ref.compose(osc)
    obj = g["object"]
    assert (obj[19, :5] == 0).all() and (obj[20, :5] == -1).all()
    assert not ada.refine_mask(osc.render(nthreads=8), 0.0).any()
    m = geo.geo_mask(obj, g["normal"], -INF)
    assert m[19, :5].all() and m[20, :5].all() and not m[17, :5].any() and not m[22, :5].any()


@pytest.mark.parametrize("transport", ["classic", "sparse"])
def test_multi_layer(pkg, transport):
    w, h, k, tau, c = 64, 48, 2, 1.0 / 32.0, 0.999
    extra = {"classic": 0, "sparse": pkg.RT_MULTI_SPARSE}[transport]
    key = ("shipped", "reflection_test", w, h)
    sc, _, _ = build_any(key)
    p, s, obj, nrm = frames(key, k)
    m = pkg.MultiRenderer(sc, [0, 0], band_rows=8, parts=2, flags=gflags(pkg, k) | extra)
    try:
        m.set_ssaa_threshold(tau)
        for cc in (-INF, c):
            m.set_ssaa_geometry(cc)
            for _ in range(2):
                m.update()
            got, want = m.download(), want_frame(p, s, k, tau, obj, nrm, cc, F32)
            assert identical(got, want), (transport, cc, mismatch(got, want))
        with pytest.raises(pkg.RtError):
            m.set_ssaa_geometry(float("nan"))
    finally:
        m.cleanup_update()
    plain = pkg.MultiRenderer(sc, [0, 0], band_rows=8, parts=2, flags=ada_flags(pkg, k))
    try:
        with pytest.raises(pkg.RtError, match="RT_FLAG_SSAA_GEOMETRY"):
            plain.set_ssaa_geometry(0.5)
    finally:
        plain.cleanup_update()


def test_setter_on_live_contexts(pkg):
    sc = scene(pkg, "20spheres", 32, 24)
    r = pkg.Renderer(sc, device=0, flags=gflags(pkg, 2))
    with pytest.raises(pkg.RtError):
        r.set_ssaa_geometry(float("nan"))
    r.set_ssaa_geometry(INF)
    r.set_ssaa_threshold(INF)
    r.update()
    hit = int((gbuffer_ref.compose(oracle_from(pkg, _oracle(), sc))["object"] >= 0).sum())
    assert r.refined >= hit > 0            # (min_cos = +inf: every pixel with an object next to one of the same object)
    r.cleanup_update()
    r = pkg.Renderer(sc, device=0, flags=ada_flags(pkg, 2))
    with pytest.raises(pkg.RtError, match="RT_FLAG_SSAA_GEOMETRY"):
        r.set_ssaa_geometry(0.5)
    r.cleanup_update()
    for extra in (0, pkg.RT_FLAG_SSAA_GEOMETRY):   # the G-buffer entry points keep refusing supersampling contexts
        r = pkg.Renderer(sc, device=0, flags=ada_flags(pkg, 2, extra))
        with pytest.raises(pkg.RtError):
            r.gbuffer()
        with pytest.raises(pkg.RtError):
            r.pick([(1, 1)])
        r.cleanup_update()


# 5. the same machine code: FAST contexts, and degree 3 in strict ones, against Renderer.gbuffer() of a k = 1 sibling
def _sibling(pkg, sc, cam, flags):
    r = pkg.Renderer(sc, device=0, flags=flags)
    try:
        r.update(cam)
        p = r.download()
        po, _, pn, _ = r.gbuffer(cam, t=False)
        return p, po.cpu().numpy(), pn.cpu().numpy()
    finally:
        r.cleanup_update()


def check_refined_set(pkg, sc, cam, k, flags, taus=(1.0 / 32.0, INF), coses=COSES):
    """-> [(tau, c, mask, frame)]: the refined set == geo_mask | refine_mask of the sibling's planes and frame, unrefined pixels == P."""
    p, obj, nrm = _sibling(pkg, sc, cam, flags)
    out = []
    r = pkg.Renderer(sc, device=0, flags=gflags(pkg, k, flags))
    try:
        for tau in taus:
            for c in coses:
                r.set_ssaa_threshold(tau)
                r.set_ssaa_geometry(c)
                r.update(cam)
                got, n = r.download(), r.refined
                mask = full_mask(p, tau, obj, nrm, c)
                assert n == int(mask.sum()), (k, tau, c, n, int(mask.sum()))
                with np.errstate(invalid="ignore"):
                    differs = (got.view(np.uint32) != p.view(np.uint32)).any(axis=-1)
                assert not (differs & ~mask).any(), (k, tau, c, int((differs & ~mask).sum()))   # unrefined pixels are P, bit for bit
                out.append((tau, c, mask, got))
    finally:
        r.cleanup_update()
    return out


@pytest.mark.parametrize("name", ["20spheres", "reflection_test", "quadratic", "clebsch"])
def test_fast_contexts_refine_the_set_of_their_own_gbuffer(pkg, name):
    w, h = 160, 120
    sc = scene(pkg, name, w, h, 4)
    for k, cam in ((2, None), (4, pkg.camera_matrix(*POSES[1]))):
        res = check_refined_set(pkg, sc, cam, k, pkg.RT_FLAG_FAST)
        full = pkg.Renderer(sc, device=0, flags=kflag(pkg, k) | pkg.RT_FLAG_FAST)
        full.update(cam)
        s = full.download()
        full.cleanup_update()
        for tau, c, mask, got in res:
            assert identical(got[mask], s[mask]), (name, k, tau, c)   # refined pixels: the FAST build's own supersampled frame
        assert any(m.any() and not m.all() for _, _, m, _ in res)


@pytest.mark.parametrize("seed", range(4))
def test_degree_three_in_strict_contexts(pkg, seed):
    """The random degree-3 scenes and cameras of the adaptive fuzz test.  Refined pixels: bit-equal to the library's own
    supersampled frame, and against the oracle's resolve conftest.compare's bar with at most max(2, 0.04 % of the pixels) beyond."""
    w, h, k = 96, 72, 2 if seed % 2 else 4
    sc, cam = random_cubic_scene(pkg, seed, w, h)
    res = check_refined_set(pkg, sc, cam, k, 0, taus=(1.0 / 32.0,), coses=(-INF, 0.999))
    full = pkg.Renderer(sc, device=0, flags=kflag(pkg, k))
    full.update(cam)
    own = full.download()
    full.cleanup_update()
    osc = oracle_from(pkg, _oracle(), sc)
    want = ssaa_ref.resolve(osc.with_size(k * w, k * h).render(cam=cam, nthreads=8), k)
    for tau, c, mask, got in res:
        assert identical(got[mask], own[mask]), (seed, tau, c)
        cmp = compare(got[mask][:, :3], want[mask][:, :3])
        print(f"degree 3 seed {seed} k {k} c {c}: refined {int(mask.sum())}, beyond the bar {cmp['n_bad_pixels']} (cap {max(2, int(0.0004 * w * h))})")
        assert cmp["n_bad_pixels"] <= max(2, int(0.0004 * w * h)), (seed, c, cmp)


# 6. update() through the reference's back-end contract
def test_update_driver(pkg, tmp_path):
    w, h, k = 64, 48, 4
    out = str(tmp_path / "f.f32")
    key = ("shipped", "20spheres", w, h)
    p, s, obj, nrm = frames(key, k)
    for val, c in (("", -INF), ("0.999", 0.999)):
        env = dict(os.environ, MI355RT_SSAA="4", MI355RT_SSAA_ADAPTIVE="", MI355RT_SSAA_GEOMETRY=val)
        q = subprocess.run([EXE, scene_path("20spheres"), str(w), str(h), "4", out, "--frames", "2"], capture_output=True, text=True, env=env, timeout=600)
        assert q.returncode == 0, q.stderr[-2000:]
        got = np.fromfile(out, dtype=np.float32).reshape(h, w, 4)
        want = want_frame(p, s, k, 1.0 / 32.0, obj, nrm, c, F32)
        assert identical(got, want), (val, mismatch(got, want))


# 7. one classifier body (rt_adaptive.hip: classify_body): the neighbour-row rule of the geometric classifier is the plain one's
ONE_W, ONE_H = 37, 23
ONE_LAYOUTS = [(1, 0, 8)] + [(3, rank, band) for band in (1, 5) for rank in range(3)]   # band 1: both neighbour rows of every row are halo slots; band 5: the last band is partial


def one_object_scene(pkg):
    """The camera inside a single sphere, lit through its wall by two lights outside it (from inside, a light inside faces no
    normal): every primary ray hits object 0, so with min_cos = -inf the geometric term can refine nothing, and the colours vary smoothly."""
    s = pkg.Scene.new(ONE_W, ONE_H, 60.0, 0, (0.1, 0.1, 0.1))
    s.add_object(pkg.surface_make("sphere", [0, 0, 0], [50.0]), (0.9, 0.8, 0.7))
    s.add_light("spherical", [30, 40, 120], (1, 1, 1), 60000.0)
    s.add_light("spherical", [-60, -20, 90], (1.0, 0.6, 0.3), 40000.0)
    return s


def test_both_classifiers_follow_one_neighbour_row_rule(pkg):
    """A context with RT_FLAG_SSAA_GEOMETRY and min_cos = -inf on a frame whose every pixel shows object 0 must return the frame, and
    the refined count, of the same context without the flag, bit for bit: for tau = -1 (everything refines), +inf (nothing does) and a
    tau taken from the plain frame at which some pixels do; as the only rank and as every rank of 3 with bands of 1 and 5 rows."""
    sc = one_object_scene(pkg)
    plain = pkg.Renderer(sc, device=0)
    try:
        plain.update()
        p = plain.download()
        po, _, _, _ = plain.gbuffer(t=False, normal=False)
        assert po.shape == (ONE_H, ONE_W) and bool((po == 0).all())   # rt_render_gbuffer: object 0 in every pixel
    finally:
        plain.cleanup_update()
    counts = {e: int(ada.refine_mask(p, 2.0 ** -e).sum()) for e in range(1, 25)}
    mid = 2.0 ** -min(counts, key=lambda e: abs(counts[e] - ONE_W * ONE_H // 2))
    assert 0 < int(ada.refine_mask(p, mid).sum()) < ONE_W * ONE_H, counts
    for fmt in (F32, U8):
        for world, rank, band in ONE_LAYOUTS:
            pair = [pkg.Renderer(sc, device=0, rank=rank, world=world, band_rows=band, flags=flags, fmt=fmt, **kw)
                    for flags, kw in ((ada_flags(pkg, 2), {}), (gflags(pkg, 2), {"ssaa_min_cos": -INF}))]
            try:
                assert pair[0].local_rows == pair[1].local_rows > 0
                for tau in (-1.0, INF, mid):
                    got = []
                    for r in pair:
                        r.set_ssaa_threshold(tau)
                        r.update()
                        got.append((r.download(), r.refined))
                    (a, na), (b, nb) = got
                    print(f"fmt {fmt} world {world} rank {rank} band {band} tau {tau}: refined {na} / {nb} of {a.shape[0] * ONE_W}, differing pixels {mismatch(b, a)}")
                    assert identical(b, a) and nb == na, (fmt, world, rank, band, tau, na, nb, mismatch(b, a))
                    assert na == {-1.0: a.shape[0] * ONE_W, INF: 0}.get(tau, na)
                    if world == 1 and tau == mid:
                        assert 0 < na < ONE_W * ONE_H, na
            finally:
                for r in pair:
                    r.cleanup_update()
