"""RT_FLAG_FAST held to exact arithmetic, ray by ray and pixel by pixel ("The FAST build against exact arithmetic").

Every context of the first half is RT_FLAG_FAST, on surfaces of degree <= 2; the second half holds the strict AND the FAST build on
degree-3 scenes, where the strict build is otherwise held only to the oracle's own formulas.  Truth, the bound B and the "decided" classification are tests/tools/fast_ref.py's, validated
without a GPU by tests/test_fast_ref_host.py on the same scenes and rays.  On every decided ray a query's `object` is the exact winner,
|t - t_exact| <= B, `point` is o + t d to 2u per term, the normal is the exact normal at that point to half a float32 ulp plus the
gradient's own bound, and a blocked flag is the exact one; a frame's pixels beyond the project's bar (conftest.compare: 1e-5 relative)
must all be pixels whose path is not decided.  Undecided rays are not judged; their share is capped (1 % of a query set, 0.2 % of a
frame).  Each assertion's message carries the worst rho = |t - t_exact| / B, the excluded count, and for a failure the ray, the object,
the device's value, the exact value and B."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, compare

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import fast_ref as F  # noqa: E402
import rays_ref  # noqa: E402
import stream_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("staged", "streamed")
FRAME_KINDS = ("default", "NOLEAN", "SIMPLE", "STREAM")


@functools.lru_cache(maxsize=None)
def case(name):
    """(product scene, oracle scene, the 2 048 query rays, their per-ray t_max)."""
    import __graft_entry__ as graft
    pkg = graft.load_package()
    sc = F.scene(pkg, name)
    osc = S.oracle_of(pkg, sc)
    rays = F.query_rays(osc, F.RAY_SEED)
    return sc, osc, rays, F.query_t_max(osc, rays, F.TMAX_SEED)


@functools.lru_cache(maxsize=None)
def frame_truth(name):
    """(the strict oracle's 96 x 72 frame, which pixels' paths are decided)."""
    osc = case(name)[1]
    decided = F.decided_paths(osc, rays_ref.primary_rays(osc), pixel_dirs=True).reshape(F.H, F.W)
    return osc.render(nthreads=8), decided


def context(pkg, name, mode, extra=0):
    flags = pkg.RT_FLAG_FAST | extra | ((pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_QUERIES) if mode == "streamed" else 0)
    r = pkg.Renderer(case(name)[0], device=0, flags=flags)
    assert r.streamed_queries == (mode == "streamed")
    return r


def to_device(rays):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float64).reshape(-1, 6)).to("cuda:0")


def passes(rep, cap=F.QUERY_CAP):
    print(rep)
    assert rep.passed(cap), str(rep)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", F.SCENES)
def test_trace_rays(pkg, name, mode):
    import torch
    _, osc, rays, _ = case(name)
    r = context(pkg, name, mode)
    out = torch.full((len(rays), 6), float("nan"), dtype=torch.float64, device="cuda:0")
    d_rays = to_device(rays)
    torch.cuda.synchronize()
    r.trace_into(d_rays.data_ptr(), len(rays), out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(-1).view(rays_ref.HIT_DTYPE)
    r.cleanup_update()
    passes(F.check_closest(osc, rays, got, f"rt_trace_rays, {name}, {mode}"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", F.SCENES)
def test_occluded_rays(pkg, name, mode):
    _, osc, rays, t_max = case(name)
    r = context(pkg, name, mode)
    plain = r.occluded(rays["o"], rays["d"])[0].cpu().numpy()
    limited = r.occluded(rays["o"], rays["d"], t_max)[0].cpu().numpy()
    r.cleanup_update()
    assert set(np.unique(plain).tolist()) <= {0, 1} and set(np.unique(limited).tolist()) <= {0, 1}
    passes(F.check_occluded(osc, rays, None, plain, f"rt_occluded_rays, t_max NULL, {name}, {mode}"))
    passes(F.check_occluded(osc, rays, t_max, limited, f"rt_occluded_rays, per-ray t_max, {name}, {mode}"))
    assert 0 < limited.sum() < plain.sum() < len(rays)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", F.SCENES)
def test_gbuffer_and_pick(pkg, name, mode):
    """rt_render_gbuffer's planes and rt_pick's records of every pixel, on the rays the same context's rt_primary_rays returns, with
    the direction term in B: a frame kernel may form the direction a few units in the last place away from those."""
    _, osc, _, _ = case(name)
    r = context(pkg, name, mode)
    rays = r.primary_rays()[0].cpu().numpy().reshape(-1, 6).copy().view(rays_ref.RAY_DTYPE).reshape(-1)
    o, t, nrm, _ = r.gbuffer()
    planes = dict(object=o.cpu().numpy().reshape(-1), t=t.cpu().numpy().reshape(-1), normal=nrm.cpu().numpy().reshape(-1, 4))
    xy = np.stack([np.tile(np.arange(F.W), F.H), np.repeat(np.arange(F.H), F.W)], axis=1)
    picked = r.pick(xy)
    r.cleanup_update()
    assert len(rays) == F.W * F.H
    want = rays_ref.primary_rays(osc)
    # (the reference's direction takes some 16 roundings of values below 1.2 -- camera_x / camera_y, the matrix row, the difference, the
    # normalisation -- so a strict and a contracted evaluation are each within 20u of the exact direction)
    print(f"{name}, {mode}: rt_primary_rays' directions differ from the strict oracle's by at most {np.abs(rays['d'] - want['d']).max() / F.U:.1f} u")
    assert np.array_equal(rays["o"], want["o"]) and np.abs(rays["d"] - want["d"]).max() <= 40 * F.U
    passes(F.check_closest(osc, rays, planes, f"rt_render_gbuffer, {name}, {mode}", pixel_dirs=True), F.FRAME_CAP)
    passes(F.check_closest(osc, rays, picked, f"rt_pick, {name}, {mode}", pixel_dirs=True), F.FRAME_CAP)
    assert (planes["normal"][:, 3] == 0).all() and (planes["object"] >= 0).sum() > len(rays) // 10


def bad_pixels(got, want, rtol=1e-5, atol=1e-7):
    """The pixels conftest.compare counts as bad (the same rule, as a mask)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    diff = np.abs(got - want)
    rel = diff / np.maximum(np.maximum(np.abs(got), np.abs(want)), 1e-300)
    return ((rel > rtol) & (diff > atol)).any(axis=-1)


def check_colours(got, name, what):
    """conftest.compare against the strict oracle's frame as it is; the bad pixels are a subset of the undecided ones and within the
    FAST frames' allowance of max(2, 0.2 % of the pixels)."""
    want, decided = frame_truth(name)
    c = compare(got, want)
    bad = bad_pixels(got, want)
    assert int(bad.sum()) == c["n_bad_pixels"]
    excluded = int((~decided).sum())
    print(f"{what}: {c}, {excluded} of {decided.size} pixels excluded")
    assert excluded <= F.FRAME_CAP * decided.size, (what, excluded)
    judged = np.argwhere(bad & decided)
    assert not len(judged), (f"{what}: {len(judged)} pixels with a decided path are beyond the bar ({excluded} excluded); first (y, x) = {judged[0].tolist()}: "
                             f"got {got[tuple(judged[0])].tolist()}, oracle {want[tuple(judged[0])].tolist()}; {c}")
    assert c["n_bad_pixels"] <= max(2, int(0.002 * decided.size)), (what, c)


@pytest.mark.parametrize("kind", FRAME_KINDS)
@pytest.mark.parametrize("name", F.SCENES)
def test_frames(pkg, name, kind):
    extra = dict(default=0, NOLEAN=pkg.RT_FLAG_NOLEAN, SIMPLE=pkg.RT_FLAG_SIMPLE, STREAM=pkg.RT_FLAG_STREAM)[kind]
    r = pkg.Renderer(case(name)[0], device=0, flags=pkg.RT_FLAG_FAST | extra)
    assert r.streamed == (kind == "STREAM")
    r.update()
    got = r.download()[..., :3].copy()
    r.cleanup_update()
    check_colours(got, name, f"rt_render, {kind}, {name}")
    want = frame_truth(name)[0]
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 50   # (a frame with something in it)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", F.SCENES)
def test_shade_rays(pkg, name, mode):
    """rt_shade_rays on the context's own primary rays: the frame's colours, held as the frames are."""
    r = context(pkg, name, mode)
    rays = r.primary_rays()[0].cpu().numpy().reshape(-1, 6)
    got = r.shade(rays[:, :3], rays[:, 3:])
    r.cleanup_update()
    assert got.shape == (F.W * F.H, 4) and (got[:, 3] == 1.0).all()
    check_colours(got[:, :3].reshape(F.H, F.W, 3), name, f"rt_shade_rays, {mode}, {name}")


# ---- degree 3: the strict and the FAST build, staged and streamed ---------------------------------------------------------------------------
# (tests/tools/fast_ref.py, "DEGREE 3"; the sets, the bars and the wrong kernels they reject are held in tests/test_fast_ref_host.py.)
# A kernel's degree-3 t is held to B3 + CUB_TOL |t_exact|: cubic_guarded answers only within CUB_TOL of the reference's result, and a
# kernel does not say which of its answers the guard gave.
BUILDS = ("strict", "FAST")
CUBIC_FRAME_KINDS = ("default", "SIMPLE", "STREAM")


@functools.lru_cache(maxsize=None)
def cubic_case(name, frame=False):
    """(product scene, oracle scene, the 1 024 query rays, their per-ray t_max); frame: the frames' field, without query rays."""
    import __graft_entry__ as graft
    import raw_desc_scenes as R
    pkg = graft.load_package()
    osc = F.cubic_scene(name, frame=frame)
    if frame:
        return R.desc(pkg, osc), osc, None, None
    rays = F.cubic_query_rays(osc, name)
    return R.desc(pkg, osc), osc, rays, F.query_t_max(osc, rays, F.TMAX_SEED)


@functools.lru_cache(maxsize=None)
def cubic_frame_truth(name):
    """(the strict oracle's 32 x 24 frame at depth 2, which pixels' paths are decided)."""
    osc = cubic_case(name, True)[1]
    decided = F.decided_paths(osc, rays_ref.primary_rays(osc), pixel_dirs=True).reshape(osc.height, osc.width)
    return osc.render(nthreads=8), decided


def cubic_context(pkg, name, build, mode, frame=False, extra=0):
    flags = (pkg.RT_FLAG_FAST if build == "FAST" else 0) | extra | ((pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_QUERIES) if mode == "streamed" else 0)
    r = pkg.Renderer(cubic_case(name, frame)[0], device=0, flags=flags)
    if mode is not None:
        assert r.streamed_queries == (mode == "streamed")
    return r


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", F.CUBIC_SCENES)
def test_degree3_trace_rays(pkg, name, build, mode):
    import torch
    _, osc, rays, _ = cubic_case(name)
    r = cubic_context(pkg, name, build, mode)
    out = torch.full((len(rays), 6), float("nan"), dtype=torch.float64, device="cuda:0")
    d_rays = to_device(rays)
    torch.cuda.synchronize()
    r.trace_into(d_rays.data_ptr(), len(rays), out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(-1).view(rays_ref.HIT_DTYPE)
    r.cleanup_update()
    passes(F.check_closest(osc, rays, got, f"rt_trace_rays, {name}, {build}, {mode}", guarded=True))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", [n for n in F.CUBIC_SCENES if n != "bent65"])
def test_degree3_occluded_rays(pkg, name, build, mode):
    _, osc, rays, t_max = cubic_case(name)
    r = cubic_context(pkg, name, build, mode)
    plain = r.occluded(rays["o"], rays["d"])[0].cpu().numpy()
    limited = r.occluded(rays["o"], rays["d"], t_max)[0].cpu().numpy()
    r.cleanup_update()
    assert set(np.unique(plain).tolist()) <= {0, 1} and set(np.unique(limited).tolist()) <= {0, 1}
    passes(F.check_occluded(osc, rays, None, plain, f"rt_occluded_rays, t_max NULL, {name}, {build}, {mode}"))
    passes(F.check_occluded(osc, rays, t_max, limited, f"rt_occluded_rays, per-ray t_max, {name}, {build}, {mode}"))
    assert 0 < limited.sum() < plain.sum() <= len(rays)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", [n for n in F.CUBIC_SCENES if n != "clebsch"])
def test_degree3_gbuffer_and_pick(pkg, name, build, mode):
    """The planes and the picks of every pixel are equal, and both are held to truth on the context's own primary rays."""
    _, osc, _, _ = cubic_case(name)
    r = cubic_context(pkg, name, build, mode)
    rays = r.primary_rays()[0].cpu().numpy().reshape(-1, 6).copy().view(rays_ref.RAY_DTYPE).reshape(-1)
    o, t, nrm, _ = r.gbuffer()
    planes = dict(object=o.cpu().numpy().reshape(-1), t=t.cpu().numpy().reshape(-1), normal=nrm.cpu().numpy().reshape(-1, 4))
    xy = np.stack([np.tile(np.arange(osc.width), osc.height), np.repeat(np.arange(osc.height), osc.width)], axis=1)
    picked = r.pick(xy)
    r.cleanup_update()
    want = rays_ref.primary_rays(osc)
    assert len(rays) == osc.width * osc.height and np.array_equal(rays["o"], want["o"]) and np.abs(rays["d"] - want["d"]).max() <= 40 * F.U
    assert np.array_equal(planes["object"], np.asarray(picked["object"]).reshape(-1))
    assert np.array_equal(planes["t"].view(np.uint64), np.ascontiguousarray(picked["t"], dtype=np.float64).reshape(-1).view(np.uint64))
    assert np.array_equal(planes["normal"][:, :3], np.asarray(picked["normal"]).reshape(len(rays), -1)[:, :3])
    passes(F.check_closest(osc, rays, planes, f"rt_render_gbuffer, {name}, {build}, {mode}", pixel_dirs=True, guarded=True), F.FRAME_CAP)
    passes(F.check_closest(osc, rays, picked, f"rt_pick, {name}, {build}, {mode}", pixel_dirs=True, guarded=True), F.FRAME_CAP)
    coefs = np.asarray(osc.coefs).reshape(-1, 20)
    assert coefs[planes["object"][planes["object"] >= 0], :10].any(axis=1).sum() > len(rays) // 10     # degree-3 hits


def check_cubic_colours(got, name, what):
    """Every pixel beyond conftest.compare's bar against the strict oracle's frame is a pixel whose path is not decided."""
    want, decided = cubic_frame_truth(name)
    c = compare(got, want)
    bad = bad_pixels(got, want)
    assert int(bad.sum()) == c["n_bad_pixels"]
    excluded = int((~decided).sum())
    print(f"{what}: {c}, {excluded} of {decided.size} pixels excluded")
    assert excluded <= F.FRAME_CAP * decided.size, (what, excluded)
    judged = np.argwhere(bad & decided)
    assert not len(judged), (f"{what}: {len(judged)} pixels with a decided path are beyond the bar ({excluded} excluded); first (y, x) = {judged[0].tolist()}: "
                             f"got {got[tuple(judged[0])].tolist()}, oracle {want[tuple(judged[0])].tolist()}; {c}")


@pytest.mark.parametrize("kind", CUBIC_FRAME_KINDS)
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", F.CUBIC_FRAME_SCENES)
def test_degree3_frames(pkg, name, build, kind):
    extra = dict(default=0, SIMPLE=pkg.RT_FLAG_SIMPLE, STREAM=pkg.RT_FLAG_STREAM)[kind]
    r = cubic_context(pkg, name, build, None, frame=True, extra=extra)
    assert r.streamed == (kind == "STREAM")
    r.update()
    got = r.download()[..., :3].copy()
    r.cleanup_update()
    check_cubic_colours(got, name, f"rt_render, {kind}, {build}, {name}")
    want = cubic_frame_truth(name)[0]
    assert got.shape == (24, 32, 3) and len(np.unique(want.reshape(-1, 3), axis=0)) > 50   # (a frame with something in it)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", F.CUBIC_FRAME_SCENES)
def test_degree3_shade_rays(pkg, name, build, mode):
    r = cubic_context(pkg, name, build, mode, frame=True)
    rays = r.primary_rays()[0].cpu().numpy().reshape(-1, 6)
    got = r.shade(rays[:, :3], rays[:, 3:])
    r.cleanup_update()
    assert got.shape == (32 * 24, 4) and (got[:, 3] == 1.0).all()
    check_cubic_colours(got[:, :3].reshape(24, 32, 3), name, f"rt_shade_rays, {build}, {mode}, {name}")
