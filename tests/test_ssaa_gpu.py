"""Supersampling (RT_FLAG_SSAA2 / RT_FLAG_SSAA4) on the GPU.  Every frame is compared bit for bit: with the numpy resolve
(tests/tools/ssaa_ref.py) of the oracle's samples at k times the size for surfaces of degree <= 2, of the same library's own k = 1
render at that size for degree-3 surfaces (both sides are the device's samples, so no libm allowance), and with the single-context
supersampled frame for bands, sparse messages, the multi-GPU layer, update() and graph capture."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ssaa_ref  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tests", "host_driver", "update_driver")
F32, U8 = 0, 1
QUADRIC = ["quadratic", "20spheres", "reflection_test"]
CUBIC = ["clebsch", "cubic", "cayley", "dingdong", "monkey_saddle"]
POSES = [((0.0, 0.0, 0.0), 90.0, 0.0), ((1.5, 0.5, -2.0), 80.0, -6.0)]


def kflag(pkg, k):
    return {1: 0, 2: pkg.RT_FLAG_SSAA2, 4: pkg.RT_FLAG_SSAA4}[k]


def scene(pkg, name, w, h, max_refl=None):
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
    if max_refl is not None:
        sc.set_max_reflections(max_refl)
    return sc


def render(pkg, name, w, h, flags=0, fmt=F32, max_refl=None, cam=None, frames=1, **kw):
    r = pkg.Renderer(scene(pkg, name, w, h, max_refl), device=0, flags=flags, fmt=fmt, **kw)
    try:
        for _ in range(frames):
            ms = r.update(cam)
        assert ms > 0.0
        return r.download()
    finally:
        r.cleanup_update()


@functools.lru_cache(maxsize=None)
def oracle_samples(name, w, h, max_refl):
    import __graft_entry__ as graft
    return graft.load_oracle().load_scene(scene_path(name)).with_size(w, h, max_refl).render(nthreads=8)


def expect(samples, k, fmt):
    out = ssaa_ref.resolve(samples, k)
    return ssaa_ref.quantise(out) if fmt == U8 else out


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


# 1. quadric scenes against the oracle's samples
@pytest.mark.parametrize("fmt", [F32, U8], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name", QUADRIC)
def test_quadric_scenes_against_the_oracle(pkg, name, k, fmt):
    w, h = 160, 120
    r = pkg.Renderer(scene(pkg, name, w, h, 4), device=0, flags=kflag(pkg, k), fmt=fmt)
    assert r.samples == k and (r.width, r.height, r.local_rows) == (w, h, h)
    r.update()
    got = r.download()
    r.cleanup_update()
    want = expect(oracle_samples(name, k * w, k * h, 4), k, fmt)
    assert same(got, want), (name, k, fmt, int((got != want).any(axis=-1).sum()))


# 2. degree-3 scenes against the library's own samples
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name", CUBIC)
def test_cubic_scenes_against_own_samples(pkg, name, k):
    w, h = 160, 120
    samples = render(pkg, name, k * w, k * h)
    for fmt in (F32, U8):
        got = render(pkg, name, w, h, flags=kflag(pkg, k), fmt=fmt)
        assert same(got, expect(samples, k, fmt)), (name, k, fmt)


# 3. full size, several frames on one context
def test_full_size_1080p_rows_against_the_oracle(pkg, oracle):
    w, h = 1920, 1080
    sc = scene(pkg, "20spheres", w, h)
    r = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_SSAA2)
    osc = oracle.load_scene(scene_path("20spheres")).with_size(2 * w, 2 * h)
    rng = np.random.default_rng(1080)
    rows = np.sort(rng.choice(h, size=16, replace=False))
    rows[0], rows[-1] = 0, h - 1
    for pos, yaw, pitch in POSES + POSES[:1]:
        cam = pkg.camera_matrix(pos, yaw, pitch)
        for _ in range(3):   # (launch-order lists and the schedule switch see earlier frames)
            r.update(cam)
        got = r.download()
        assert got.shape == (h, w, 4)
        samples = osc.render(cam=cam, rows=np.stack([2 * rows, 2 * rows + 1], axis=1).reshape(-1), nthreads=8)
        assert same(got[rows], ssaa_ref.resolve(samples, 2)), (pos, yaw, pitch)
    r.cleanup_update()


# 4. variants
@pytest.mark.parametrize("name", ["20spheres", "reflection_test", "clebsch"])
def test_variants(pkg, name):
    w, h = 200, 150
    base = render(pkg, name, w, h, flags=pkg.RT_FLAG_SSAA2, frames=2)
    for extra in (pkg.RT_FLAG_SIMPLE, pkg.RT_FLAG_NOLEAN, pkg.RT_FLAG_NOCULL | pkg.RT_FLAG_STATIC_ORDER):
        assert same(render(pkg, name, w, h, flags=pkg.RT_FLAG_SSAA2 | extra, frames=2), base), (name, extra)
    fast_samples = render(pkg, name, 2 * w, 2 * h, flags=pkg.RT_FLAG_FAST)
    for fmt in (F32, U8):
        got = render(pkg, name, w, h, flags=pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_FAST, fmt=fmt, frames=2)
        assert same(got, expect(fast_samples, 2, fmt)), (name, fmt)


# 5. bands and reassembly
@pytest.mark.parametrize("fmt", [F32, U8], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("k", [2, 4])
def test_bands_and_rt_assemble(pkg, k, fmt):
    import torch
    w, h, world, band = 150, 107, 3, 5
    sc = scene(pkg, "reflection_test", w, h, 4)
    want = render(pkg, "reflection_test", w, h, flags=kflag(pkg, k), fmt=fmt, max_refl=4)
    rs = [pkg.Renderer(sc, device=0, rank=r, world=world, band_rows=band, flags=kflag(pkg, k), fmt=fmt) for r in range(world)]
    mlr = pkg.max_local_rows(h, band, world)
    dt = torch.uint8 if fmt == U8 else torch.float32
    gathered = torch.zeros((world, mlr, w, 4), dtype=dt, device="cuda:0")
    for r, ren in enumerate(rs):
        rows = pkg.band_rows_of_rank(h, band, world, r)
        assert ren.local_rows == len(rows) and ren.max_local_rows == mlr
        assert np.array_equal(ren.row_map(), rows)
        assert ren.pixel_bytes == (4 if fmt == U8 else 16)
        ren.update()
        local = ren.download()
        assert local.shape == (len(rows), w, 4)
        assert same(local, want[rows])
        gathered[r, :len(rows)] = torch.from_numpy(local).to("cuda:0")
    full = torch.zeros((h, w, 4), dtype=dt, device="cuda:0")
    rs[0].assemble(gathered.data_ptr(), full.data_ptr())
    torch.cuda.synchronize()
    assert same(full.cpu().numpy(), want)
    # a rank rendering straight into a caller's buffer (dev_fb) gives the same rows
    buf = torch.zeros((rs[1].local_rows, w, 4), dtype=dt, device="cuda:0")
    rs[1].update(dev_fb=buf.data_ptr())
    torch.cuda.synchronize()
    assert same(buf.cpu().numpy(), want[pkg.band_rows_of_rank(h, band, world, 1)])
    for ren in rs:
        ren.cleanup_update()


# 6. sparse messages
def _tiles_of(words, cap, pixel_words):
    off = (4 + cap + 3) & ~3
    tw = 256 * pixel_words
    return {int(words[4 + j]): words[off + j * tw: off + (j + 1) * tw].tobytes() for j in range(min(int(words[0]), cap))}


@pytest.mark.parametrize("fmt", [F32, U8], ids=["rgba32f", "rgba8"])
def test_sparse_transport(pkg, fmt):
    import torch
    w, h, world, band = 200, 150, 2, 8
    sc = scene(pkg, "20spheres", w, h)
    bg = pkg.bg_rgba8(sc.arrays()["bg_color"]) if fmt == U8 else pkg.bg_rgba32f(sc.arrays()["bg_color"])
    pw = 1 if fmt == U8 else 4
    rs = [pkg.Renderer(sc, device=0, rank=r, world=world, band_rows=band, flags=pkg.RT_FLAG_SSAA2, fmt=fmt) for r in range(world)]
    cap = max(((w + 15) // 16) * ((ren.local_rows + 15) // 16) for ren in rs)
    nbytes = rs[0].sparse_msg_bytes(cap)
    stamps = torch.zeros(rs[0].sparse_stamp_bytes(), dtype=torch.uint8, device="cuda:0")
    assert stamps.numel() == 4 * world * cap
    inc = torch.zeros((h, w, 4), dtype=torch.uint8 if fmt == U8 else torch.float32, device="cuda:0")
    for tag, (pos, yaw, pitch) in enumerate(POSES):
        cam = pkg.camera_matrix(pos, yaw, pitch)
        want = render(pkg, "20spheres", w, h, flags=pkg.RT_FLAG_SSAA2, fmt=fmt, cam=cam)
        direct = torch.full((world, nbytes), 0xCD, dtype=torch.uint8, device="cuda:0")
        packed = torch.full((world, nbytes), 0xAB, dtype=torch.uint8, device="cuda:0")
        for r, ren in enumerate(rs):
            ren.update_sparse(direct[r].data_ptr(), cap, cam=cam)
            ren.update(cam)
            ren.pack_sparse(packed[r].data_ptr(), cap)
        torch.cuda.synchronize()
        d, p = direct.cpu().numpy().view(np.uint32), packed.cpu().numpy().view(np.uint32)
        for r, ren in enumerate(rs):
            assert not d[r, 1] and np.array_equal(d[r, :4], p[r, :4]), (r, d[r, :4], p[r, :4])
            assert _tiles_of(d[r], cap, pw) == _tiles_of(p[r], cap, pw)   # (slot order is free)
            mirror = pkg.pack_sparse_numpy(want[pkg.band_rows_of_rank(h, band, world, r)], ren.local_rows, bg, cap)
            assert int(d[r, 0]) == int(mirror[0]) and _tiles_of(d[r], cap, pw) == _tiles_of(mirror, cap, pw)
            # the tiles that travel are the OUTPUT tiles that are not pure background
            local = np.ascontiguousarray(want[pkg.band_rows_of_rank(h, band, world, r)]).view(np.uint32).reshape(ren.local_rows, w, pw)
            n = sum(bool(np.any(local[ty:ty + 16, tx:tx + 16] != np.asarray(bg, np.uint32).reshape(pw)))
                    for ty in range(0, ren.local_rows, 16) for tx in range(0, w, 16))
            assert int(d[r, 0]) == n
        full = torch.zeros_like(inc)
        rs[0].assemble_sparse(direct.data_ptr(), cap, full.data_ptr())
        rs[0].assemble_sparse_incremental(direct.data_ptr(), cap, inc.data_ptr(), stamps.data_ptr(), tag)
        torch.cuda.synchronize()
        assert same(full.cpu().numpy(), want), pos
        assert same(inc.cpu().numpy(), want), ("incremental", pos)
    for ren in rs:
        ren.cleanup_update()


# 7. the multi-GPU layer, one device repeated
@pytest.mark.parametrize("transport", ["classic", "bandwise", "sparse"])
def test_multi_layer(pkg, transport):
    w, h = 200, 150
    extra = {"classic": 0, "bandwise": pkg.RT_MULTI_BANDWISE, "sparse": pkg.RT_MULTI_SPARSE}[transport]
    sc = scene(pkg, "reflection_test", w, h, 4)
    m = pkg.MultiRenderer(sc, [0, 0], band_rows=8, parts=4, flags=pkg.RT_FLAG_SSAA2 | extra)
    try:
        assert m.n_contexts == 8
        for pos, yaw, pitch in POSES:
            cam = pkg.camera_matrix(pos, yaw, pitch)
            want = render(pkg, "reflection_test", w, h, flags=pkg.RT_FLAG_SSAA2, max_refl=4, cam=cam)
            for _ in range(2):
                m.update(cam)
            assert same(m.download(), want), (transport, pos)
            sent, dense = m.last_transfer()
            assert dense == w * h * 16 and sent > 0   # (the output frame's bytes, not the samples')
    finally:
        m.cleanup_update()


# 8. update() through the reference's back-end contract
@pytest.mark.parametrize("devices", [None, "0,0"], ids=["single", "multi"])
def test_update_driver(pkg, tmp_path, devices):
    w, h = 192, 144
    out = str(tmp_path / "f.f32")
    env = dict(os.environ, MI355RT_SSAA="2")
    if devices:
        env.update(MI355RT_DEVICES=devices, MI355RT_PARTS="2", MI355RT_BAND_ROWS="8")
    p = subprocess.run([EXE, scene_path("reflection_test"), str(w), str(h), "4", out, "--frames", "2"], capture_output=True, text=True, env=env,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    got = np.fromfile(out, dtype=np.float32).reshape(h, w, 4)
    assert same(got, render(pkg, "reflection_test", w, h, flags=pkg.RT_FLAG_SSAA2, max_refl=4))


# 9. counters and timing
@pytest.mark.parametrize("extra", [0, 4], ids=["wavefront", "simple"])
@pytest.mark.parametrize("k", [2, 4])
def test_counters_count_every_sample(pkg, k, extra):
    w, h = 120, 90
    r = pkg.Renderer(scene(pkg, "20spheres", w, h), device=0, flags=kflag(pkg, k) | pkg.RT_FLAG_COUNT | extra)
    ms = r.update()
    assert ms > 0.0
    c = r.counters()
    assert c["primary_rays"] == k * k * w * h
    r.cleanup_update()
    c1 = pkg.Renderer(scene(pkg, "20spheres", k * w, k * h), device=0, flags=pkg.RT_FLAG_COUNT | extra)
    c1.update()
    c1c = c1.counters()
    for key in ("primary_rays", "shadow_rays", "reflect_rays", "tests", "hits"):   # the same rays as a k = 1 frame of the sample grid
        assert c1c[key] == c[key], key
    c1.cleanup_update()


# 10. stream capture
def test_stream_capture_of_three_frames(pkg):
    import torch
    w, h = 200, 150
    sc = scene(pkg, "20spheres", w, h)
    cams = [pkg.camera_matrix(*p) for p in POSES + [((0.5, 0.0, 1.0), 95.0, 3.0)]]
    r = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_SSAA2)
    bufs = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in cams]
    s = torch.cuda.Stream()
    r.update(cams[0], stream=s.cuda_stream, timed=False)   # (first call on this stream before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for cam, buf in zip(cams, bufs):
            r.update(cam, dev_fb=buf.data_ptr(), stream=s.cuda_stream, timed=False)
    g.replay()
    torch.cuda.synchronize()
    for cam, buf in zip(cams, bufs):
        assert same(buf.cpu().numpy(), render(pkg, "20spheres", w, h, flags=pkg.RT_FLAG_SSAA2, cam=cam))
    del g
    r.cleanup_update()
