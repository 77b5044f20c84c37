"""Edge-adaptive supersampling (RT_FLAG_SSAA_ADAPTIVE) on the GPU.  Every frame is compared bit for bit with the numpy composition
(tests/tools/ssaa_adaptive_ref.py) of a W x H plain frame and a kW x kH sample frame: the oracle's for surfaces of degree <= 2, the
library's own k = 1 renders for degree-3 surfaces; and with single-context frames for bands, sparse messages, the multi layer,
update() and graph capture."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ssaa_adaptive_ref as ada  # noqa: E402
import ssaa_ref  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tests", "host_driver", "update_driver")
F32, U8 = 0, 1
QUADRIC = ["quadratic", "20spheres", "reflection_test"]
CUBIC = ["clebsch", "cubic", "cayley", "dingdong", "monkey_saddle"]
POSES = [((0.0, 0.0, 0.0), 90.0, 0.0), ((1.5, 0.5, -2.0), 80.0, -6.0)]
TAU = 1.0 / 32.0


def kflag(pkg, k):
    return {2: pkg.RT_FLAG_SSAA2, 4: pkg.RT_FLAG_SSAA4}[k]


def scene(pkg, name, w, h, max_refl=None):
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
    if max_refl is not None:
        sc.set_max_reflections(max_refl)
    return sc


def render(pkg, name, w, h, flags=0, fmt=F32, max_refl=None, cam=None, frames=1, refined=False, **kw):
    r = pkg.Renderer(scene(pkg, name, w, h, max_refl), device=0, flags=flags, fmt=fmt, **kw)
    try:
        for _ in range(frames):
            ms = r.update(cam)
        assert ms > 0.0
        out = r.download()
        return (out, r.refined) if refined else out
    finally:
        r.cleanup_update()


@functools.lru_cache(maxsize=None)
def oracle_frame(name, w, h, max_refl):
    import __graft_entry__ as graft
    return graft.load_oracle().load_scene(scene_path(name)).with_size(w, h, max_refl).render(nthreads=8)


def expect(p, s, k, tau, fmt):
    out = ada.compose(p, s, k, tau)
    return ssaa_ref.quantise(out) if fmt == U8 else out


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def ada_flags(pkg, k, extra=0):
    return kflag(pkg, k) | pkg.RT_FLAG_SSAA_ADAPTIVE | extra


# 1. quadric scenes against the oracle
@pytest.mark.parametrize("fmt", [F32, U8], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name", QUADRIC)
def test_quadric_scenes_against_the_oracle(pkg, name, k, fmt):
    w, h = 160, 120
    p = oracle_frame(name, w, h, 4)
    s = oracle_frame(name, k * w, k * h, 4)
    for tau in (TAU, 0.2):
        got, n = render(pkg, name, w, h, flags=ada_flags(pkg, k), fmt=fmt, max_refl=4, refined=True, ssaa_threshold=tau)
        want = expect(p, s, k, tau, fmt)
        assert same(got, want), (name, k, fmt, tau, int((got != want).any(axis=-1).sum()))
        assert n == int(ada.refine_mask(p, tau).sum()), (n, tau)


# 2. degree-3 scenes against the library's own k = 1 renders
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name", CUBIC)
def test_cubic_scenes_against_own_renders(pkg, name, k):
    w, h = 120, 90
    p, s = render(pkg, name, w, h), render(pkg, name, k * w, k * h)
    for fmt in (F32, U8):
        for tau in (TAU, 0.1):
            got = render(pkg, name, w, h, flags=ada_flags(pkg, k), fmt=fmt, ssaa_threshold=tau)
            assert same(got, expect(p, s, k, tau, fmt)), (name, k, fmt, tau)


# 3. the two limits: tau < 0 is the full supersampled frame (every pixel through the ray-list kernel), +inf the k = 1 frame
@pytest.mark.parametrize("name", QUADRIC + CUBIC)
def test_limits(pkg, name):
    w, h = 96, 72
    for k in (2, 4):
        full = render(pkg, name, w, h, flags=kflag(pkg, k), max_refl=4)
        got, n = render(pkg, name, w, h, flags=ada_flags(pkg, k), max_refl=4, refined=True, ssaa_threshold=-1.0)
        assert same(got, full) and n == w * h, (name, k)
    plain = render(pkg, name, w, h, max_refl=4)
    got, n = render(pkg, name, w, h, flags=ada_flags(pkg, 2), max_refl=4, refined=True, ssaa_threshold=float("inf"))
    assert same(got, plain) and n == 0, name


# 4. odd sizes and thin images
@pytest.mark.parametrize("w,h", [(37, 23), (1, 40), (40, 1), (1, 1), (17, 3)])
def test_odd_sizes(pkg, w, h):
    for k in (2, 4):
        p, s = oracle_frame("reflection_test", w, h, 4), oracle_frame("reflection_test", k * w, k * h, 4)
        for fmt in (F32, U8):
            got = render(pkg, "reflection_test", w, h, flags=ada_flags(pkg, k), fmt=fmt, max_refl=4, ssaa_threshold=0.01)
            assert same(got, expect(p, s, k, 0.01, fmt)), (w, h, k, fmt)


# 5. variants
@pytest.mark.parametrize("name", ["20spheres", "reflection_test", "clebsch"])
def test_variants(pkg, name):
    w, h = 200, 150
    base = render(pkg, name, w, h, flags=ada_flags(pkg, 2), frames=2)
    for extra in (pkg.RT_FLAG_SIMPLE, pkg.RT_FLAG_NOLEAN, pkg.RT_FLAG_NOCULL | pkg.RT_FLAG_STATIC_ORDER):
        assert same(render(pkg, name, w, h, flags=ada_flags(pkg, 2, extra), frames=2), base), (name, extra)
    fast = pkg.RT_FLAG_FAST
    for tau in (TAU, -1.0):
        got = render(pkg, name, w, h, flags=ada_flags(pkg, 2, fast), frames=2, ssaa_threshold=tau)
        if tau < 0:
            assert same(got, render(pkg, name, w, h, flags=pkg.RT_FLAG_SSAA2 | fast)), name
        else:
            p = render(pkg, name, w, h, flags=fast)
            s = render(pkg, name, 2 * w, 2 * h, flags=fast)
            assert same(got, expect(p, s, 2, tau, F32)), name


# 6. bands (of 5 and of 1 rows) and reassembly: every rank's rows equal the single-context frame's (needs the halo rows)
@pytest.mark.parametrize("band", [5, 1])
@pytest.mark.parametrize("fmt", [F32, U8], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("k", [2, 4])
def test_bands_and_rt_assemble(pkg, k, fmt, band):
    import torch
    w, h, world = 150, 107, 3
    sc = scene(pkg, "reflection_test", w, h, 4)
    want = render(pkg, "reflection_test", w, h, flags=ada_flags(pkg, k), fmt=fmt, max_refl=4)
    rs = [pkg.Renderer(sc, device=0, rank=r, world=world, band_rows=band, flags=ada_flags(pkg, k), fmt=fmt) for r in range(world)]
    mlr = pkg.max_local_rows(h, band, world)
    dt = torch.uint8 if fmt == U8 else torch.float32
    gathered = torch.zeros((world, mlr, w, 4), dtype=dt, device="cuda:0")
    for r, ren in enumerate(rs):
        rows = pkg.band_rows_of_rank(h, band, world, r)
        ren.update()
        local = ren.download()
        assert same(local, want[rows]), (r, int((local != want[rows]).any(axis=-1).sum()))
        gathered[r, :len(rows)] = torch.from_numpy(local).to("cuda:0")
    full = torch.zeros((h, w, 4), dtype=dt, device="cuda:0")
    rs[0].assemble(gathered.data_ptr(), full.data_ptr())
    torch.cuda.synchronize()
    assert same(full.cpu().numpy(), want)
    buf = torch.zeros((rs[1].local_rows, w, 4), dtype=dt, device="cuda:0")
    rs[1].update(dev_fb=buf.data_ptr())
    torch.cuda.synchronize()
    assert same(buf.cpu().numpy(), want[pkg.band_rows_of_rank(h, band, world, 1)])
    for ren in rs:
        ren.cleanup_update()


# 7. sparse messages
def _tiles_of(words, cap, pixel_words):
    off = (4 + cap + 3) & ~3
    tw = 256 * pixel_words
    return {int(words[4 + j]): words[off + j * tw: off + (j + 1) * tw].tobytes() for j in range(min(int(words[0]), cap))}


@pytest.mark.parametrize("fmt", [F32, U8], ids=["rgba32f", "rgba8"])
def test_sparse_transport(pkg, fmt):
    import torch
    w, h, world, band = 200, 150, 2, 8
    sc = scene(pkg, "20spheres", w, h)
    pw = 1 if fmt == U8 else 4
    fl = ada_flags(pkg, 2)
    rs = [pkg.Renderer(sc, device=0, rank=r, world=world, band_rows=band, flags=fl, fmt=fmt) for r in range(world)]
    cap = max(((w + 15) // 16) * ((ren.local_rows + 15) // 16) for ren in rs)
    nbytes = rs[0].sparse_msg_bytes(cap)
    stamps = torch.zeros(rs[0].sparse_stamp_bytes(), dtype=torch.uint8, device="cuda:0")
    inc = torch.zeros((h, w, 4), dtype=torch.uint8 if fmt == U8 else torch.float32, device="cuda:0")
    for tag, (pos, yaw, pitch) in enumerate(POSES):
        cam = pkg.camera_matrix(pos, yaw, pitch)
        want = render(pkg, "20spheres", w, h, flags=fl, fmt=fmt, cam=cam)
        direct = torch.full((world, nbytes), 0xCD, dtype=torch.uint8, device="cuda:0")
        packed = torch.full((world, nbytes), 0xAB, dtype=torch.uint8, device="cuda:0")
        for r, ren in enumerate(rs):
            ren.update_sparse(direct[r].data_ptr(), cap, cam=cam)
            ren.update(cam)
            ren.pack_sparse(packed[r].data_ptr(), cap)
        torch.cuda.synchronize()
        d, p = direct.cpu().numpy().view(np.uint32), packed.cpu().numpy().view(np.uint32)
        for r in range(world):
            assert not d[r, 1] and np.array_equal(d[r, :4], p[r, :4])
            assert _tiles_of(d[r], cap, pw) == _tiles_of(p[r], cap, pw)
        full = torch.zeros_like(inc)
        rs[0].assemble_sparse(direct.data_ptr(), cap, full.data_ptr())
        rs[0].assemble_sparse_incremental(direct.data_ptr(), cap, inc.data_ptr(), stamps.data_ptr(), tag)
        torch.cuda.synchronize()
        assert same(full.cpu().numpy(), want), pos
        assert same(inc.cpu().numpy(), want), ("incremental", pos)
    for ren in rs:
        ren.cleanup_update()


# 8. the multi-GPU layer, one device repeated, and its threshold setter
@pytest.mark.parametrize("transport", ["classic", "bandwise", "sparse"])
def test_multi_layer(pkg, transport):
    w, h = 200, 150
    extra = {"classic": 0, "bandwise": pkg.RT_MULTI_BANDWISE, "sparse": pkg.RT_MULTI_SPARSE}[transport]
    sc = scene(pkg, "reflection_test", w, h, 4)
    m = pkg.MultiRenderer(sc, [0, 0], band_rows=8, parts=4, flags=ada_flags(pkg, 2) | extra)
    try:
        for tau in (TAU, 0.15):
            if tau != TAU:
                m.set_ssaa_threshold(tau)
            for pos, yaw, pitch in POSES:
                cam = pkg.camera_matrix(pos, yaw, pitch)
                want = render(pkg, "reflection_test", w, h, flags=ada_flags(pkg, 2), max_refl=4, cam=cam, ssaa_threshold=tau)
                for _ in range(2):
                    m.update(cam)
                assert same(m.download(), want), (transport, pos, tau)
        with pytest.raises(pkg.RtError):
            m.set_ssaa_threshold(float("nan"))
    finally:
        m.cleanup_update()


# 9. update() through the reference's back-end contract
@pytest.mark.parametrize("devices", [None, "0,0"], ids=["single", "multi"])
def test_update_driver(pkg, tmp_path, devices):
    w, h = 192, 144
    out = str(tmp_path / "f.f32")
    for val, tau in (("", TAU), ("0.1", 0.1)):
        env = dict(os.environ, MI355RT_SSAA="2", MI355RT_SSAA_ADAPTIVE=val)
        if devices:
            env.update(MI355RT_DEVICES=devices, MI355RT_PARTS="2", MI355RT_BAND_ROWS="8")
        p = subprocess.run([EXE, scene_path("reflection_test"), str(w), str(h), "4", out, "--frames", "2"], capture_output=True, text=True, env=env,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        got = np.fromfile(out, dtype=np.float32).reshape(h, w, 4)
        assert same(got, render(pkg, "reflection_test", w, h, flags=ada_flags(pkg, 2), max_refl=4, ssaa_threshold=tau)), val


# 10. the threshold between frames, refusals on a live context
def test_threshold_between_frames(pkg):
    w, h = 160, 120
    r = pkg.Renderer(scene(pkg, "20spheres", w, h), device=0, flags=ada_flags(pkg, 4))
    with pytest.raises(pkg.RtError):
        r.set_ssaa_threshold(float("nan"))
    r.update()
    a = r.download()
    r.set_ssaa_threshold(-1.0)
    assert same(r.download(), a)                       # (applies from the next frame on)
    r.update()
    assert same(r.download(), render(pkg, "20spheres", w, h, flags=kflag(pkg, 4))) and r.refined == w * h
    r.set_ssaa_threshold(TAU)
    r.update()
    assert same(r.download(), a)
    r.cleanup_update()
    plain = pkg.Renderer(scene(pkg, "20spheres", w, h), device=0, flags=pkg.RT_FLAG_SSAA2)
    with pytest.raises(pkg.RtError):
        plain.set_ssaa_threshold(0.1)
    with pytest.raises(pkg.RtError):
        plain.refined
    plain.cleanup_update()


# 11. stream capture: three frames with different cameras
def test_stream_capture_of_three_frames(pkg):
    import torch
    w, h = 200, 150
    sc = scene(pkg, "20spheres", w, h)
    cams = [pkg.camera_matrix(*p) for p in POSES + [((0.5, 0.0, 1.0), 95.0, 3.0)]]
    r = pkg.Renderer(sc, device=0, flags=ada_flags(pkg, 4))
    bufs = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in cams]
    s = torch.cuda.Stream()
    r.update(cams[0], stream=s.cuda_stream, timed=False)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for cam, buf in zip(cams, bufs):
            r.update(cam, dev_fb=buf.data_ptr(), stream=s.cuda_stream, timed=False)
    r.set_ssaa_threshold(-1.0)   # (the graph keeps the tau it was captured with)
    g.replay()
    torch.cuda.synchronize()
    for cam, buf in zip(cams, bufs):
        assert same(buf.cpu().numpy(), render(pkg, "20spheres", w, h, flags=ada_flags(pkg, 4), cam=cam))
    del g
    r.cleanup_update()


# 12. counters: one ray per pixel, the halo rows, k^2 per refined pixel
@pytest.mark.parametrize("extra", [0, 4], ids=["wavefront", "simple"])
@pytest.mark.parametrize("k", [2, 4])
def test_counters(pkg, k, extra):
    w, h = 120, 90
    r = pkg.Renderer(scene(pkg, "20spheres", w, h), device=0, flags=ada_flags(pkg, k, pkg.RT_FLAG_COUNT | extra))
    r.update()
    assert r.counters()["primary_rays"] == w * h + k * k * r.refined
    r.cleanup_update()
    world, band = 3, 4
    for rank in range(world):
        rr = pkg.Renderer(scene(pkg, "20spheres", w, h), device=0, rank=rank, world=world, band_rows=band, flags=ada_flags(pkg, k, pkg.RT_FLAG_COUNT | extra))
        rr.update()
        rows = pkg.band_rows_of_rank(h, band, world, rank)
        own = set(int(v) for v in rows)
        halo = 0
        for b0 in range(0, len(rows), band):
            g0, g1 = int(rows[b0]), int(rows[min(b0 + band, len(rows)) - 1])
            halo += (g0 - 1 >= 0 and g0 - 1 not in own) + (g1 + 1 < h and g1 + 1 not in own)
        assert rr.counters()["primary_rays"] == w * len(rows) + w * halo + k * k * rr.refined, rank
        rr.cleanup_update()


# 13. full size, several poses, against the library's own k = 1 renders at both sizes
def test_full_size_1080p(pkg):
    w, h = 1920, 1080
    r = pkg.Renderer(scene(pkg, "20spheres", w, h), device=0, flags=ada_flags(pkg, 2))
    for pos, yaw, pitch in POSES + [((0.5, 0.0, 1.0), 95.0, 3.0)]:
        cam = pkg.camera_matrix(pos, yaw, pitch)
        for _ in range(2):
            r.update(cam)
        got = r.download()
        p = render(pkg, "20spheres", w, h, cam=cam)
        s = render(pkg, "20spheres", 2 * w, 2 * h, cam=cam)
        assert same(got, ada.compose(p, s, 2, TAU)), pos
        assert r.refined == int(ada.refine_mask(p, TAU).sum())
    r.cleanup_update()
