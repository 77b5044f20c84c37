"""Sparse transport of RGBA32F frames on the GPU: rt_render_sparse / rt_pack_sparse / rt_assemble_sparse[_incremental] with 16-byte
pixels, RT_MULTI_SPARSE in the one-process multi-GPU layer, and update() with MI355RT_MULTI_SPARSE.  Every frame must equal the
single-context rt_render frame (same flags) bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path
import test_gpu_parity as gp

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tests", "host_driver", "update_driver")
F32 = 0


def _tiles_of(words, cap, pixel_words):
    """id -> tile bytes of one message (slot order is free)."""
    off = (4 + cap + 3) & ~3
    tw = 256 * pixel_words
    return {int(words[4 + j]): words[off + j * tw: off + (j + 1) * tw].tobytes() for j in range(min(int(words[0]), cap))}


RANK_CASES = [(200, 250, 3, 8, "20spheres"), (333, 97, 2, 16, "20spheres"), (256, 160, 4, 5, "reflection_test"), (96, 72, 2, 8, "cayley"),
              (64, 48, 1, 16, "quadratic")]


@pytest.mark.parametrize("flags", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("w,h,world,band,name", RANK_CASES)
def test_rank_level_rgba32f_transport(pkg, w, h, world, band, name, flags):
    """rt_render_sparse -> rt_assemble_sparse and rt_render -> rt_pack_sparse -> rt_assemble_sparse, three frames in a row (launch-order
    feedback active): the rebuilt frame equals the dense RGBA32F frame; packed messages hold the numpy mirror's id -> tile pairs; a
    capacity that is too small only raises `overflow` and leaves the bytes after the message alone."""
    import torch
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(w, h)
    ref = pkg.Renderer(sc, device=0, flags=flags, fmt=F32)
    ref.update()
    want = ref.download()
    rs = [pkg.Renderer(sc, device=0, rank=r, world=world, band_rows=band, flags=flags, fmt=F32) for r in range(world)]
    bg = pkg.bg_rgba32f(sc.arrays()["bg_color"])
    n_tiles = max(((w + 15) // 16) * ((ren.local_rows + 15) // 16) for ren in rs)
    nbytes = rs[0].sparse_msg_bytes(n_tiles)
    assert nbytes == 16 * ((4 + n_tiles + 3) // 4) + 4096 * n_tiles
    for frame in range(3):
        # (a) one kernel writes the message
        msgs = torch.full((world, nbytes), 0xCD, dtype=torch.uint8, device="cuda:0")
        for r, ren in enumerate(rs):
            ren.update_sparse(msgs[r].data_ptr(), n_tiles)
        out = torch.full((h, w, 4), 7.0e30, dtype=torch.float32, device="cuda:0")
        rs[0].assemble_sparse(msgs.data_ptr(), n_tiles, out.data_ptr())
        torch.cuda.synchronize()
        assert not msgs.cpu().numpy().view(np.uint32)[:, 1].any()
        assert np.array_equal(out.cpu().numpy(), want), ("render_sparse", frame)
        # (b) render + pack
        msgs.fill_(0xAB)
        for r, ren in enumerate(rs):
            ren.update()
            ren.pack_sparse(msgs[r].data_ptr(), n_tiles)
        out.fill_(3.0)
        rs[0].assemble_sparse(msgs.data_ptr(), n_tiles, out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), ("pack", frame)
        words = msgs.cpu().numpy().view(np.uint32)
        for r, ren in enumerate(rs):
            mirror = pkg.pack_sparse_numpy(ren.download(), ren.local_rows, bg, n_tiles)
            assert words[r][0] == mirror[0] and words[r][1] == 0
            assert _tiles_of(words[r], n_tiles, 4) == _tiles_of(mirror, n_tiles, 4)
        assert np.array_equal(pkg.assemble_sparse_numpy(words, w, h, band, world, bg, n_tiles), want)
    # too small: overflow only, nothing written past the message (a canary region after it)
    small = max(1, n_tiles // 7)
    sb = rs[0].sparse_msg_bytes(small)
    for how in ("render_sparse", "pack"):
        buf = torch.full((world, sb + 8192), 0x5C, dtype=torch.uint8, device="cuda:0")
        for r, ren in enumerate(rs):
            if how == "render_sparse":
                ren.update_sparse(buf[r].data_ptr(), small)
            else:
                ren.update()
                ren.pack_sparse(buf[r].data_ptr(), small)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.all(host[:, sb:] == 0x5C), how
        hdr = host[:, :16].copy().view(np.uint32)
        assert np.array_equal(hdr[:, 1] != 0, hdr[:, 0] > small), how


def test_rgba8_sizes_unchanged(pkg):
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(64, 48)
    r8 = pkg.Renderer(sc, device=0, fmt=pkg.RT_FMT_RGBA8)
    for cap in (0, 1, 3, 4, 5, 16200):
        assert r8.sparse_msg_bytes(cap) == pkg.Renderer.sparse_bytes(cap)


def test_incremental_rgba32f_assembly_follows_a_moving_camera(pkg):
    """rt_assemble_sparse_incremental on RGBA32F: cuts where content appears, disappears entirely and comes back; every frame equals the
    dense frame."""
    import torch
    w, h, world, band = 400, 300, 3, 16
    sc = gp.random_scene(pkg, 777, 9, 4, w=w, h=h, with_plane=False)
    ref = pkg.Renderer(sc, device=0, fmt=F32)
    rs = [pkg.Renderer(sc, device=0, rank=r, world=world, band_rows=band, fmt=F32) for r in range(world)]
    cap = max(((w + 15) // 16) * ((ren.local_rows + 15) // 16) for ren in rs)
    nbytes = rs[0].sparse_msg_bytes(cap)
    msgs = torch.zeros((world, nbytes), dtype=torch.uint8, device="cuda:0")
    full = torch.full((h, w, 4), 3.0, dtype=torch.float32, device="cuda:0")
    stamps = torch.full((rs[0].sparse_stamp_bytes(),), 0x5A, dtype=torch.uint8, device="cuda:0")
    cams = [pkg.camera_matrix((0.0, 0.0, 0.0), 90.0, 0.0), pkg.camera_matrix((2.0, 0.5, 1.0), 80.0, 3.0), pkg.camera_matrix((0.0, 0.0, 0.0), -90.0, 0.0),
            pkg.camera_matrix((0.0, 0.0, 0.0), -90.0, 0.0), pkg.camera_matrix((-3.0, 1.0, 4.0), 100.0, -5.0), pkg.camera_matrix((0.0, 0.0, 0.0), 90.0, 0.0)]
    saw_content = 0
    for k, cam in enumerate(cams):
        for r, ren in enumerate(rs):
            if k % 2:
                ren.update_sparse(msgs[r].data_ptr(), cap, cam)
            else:
                ren.update(cam)
                ren.pack_sparse(msgs[r].data_ptr(), cap)
        rs[0].assemble_sparse_incremental(msgs.data_ptr(), cap, full.data_ptr(), stamps.data_ptr(), k)
        ref.update(cam)
        torch.cuda.synchronize()
        assert np.array_equal(full.cpu().numpy(), ref.download()), f"frame {k}"
        saw_content += int(msgs.cpu().numpy().view(np.uint32)[:, 0].sum() > 0)
    assert 3 <= saw_content < len(cams)


def _expected_sent(pkg, want, bg, h, w, band, world, pixel_words, msg_bytes_of):
    """Σ over contexts of header + id array + count x tile bytes, the counts taken from the single-context frame."""
    mx = pkg.max_local_rows(h, band, world)
    cap = ((w + 15) // 16) * ((mx + 15) // 16)
    head = msg_bytes_of(cap) - cap * 1024 * pixel_words
    total = 0
    for q in range(world):
        rows = pkg.band_rows_of_rank(h, band, world, q)
        count = int(pkg.pack_sparse_numpy(want[rows], len(rows), bg, cap)[0]) if len(rows) else 0
        total += head + count * 1024 * pixel_words
    return total


MULTI_CASES = [([0, 0, 0], 1, 8, (400, 277)), ([0, 0], 2, 16, (400, 277)), ([0], 3, 16, (400, 277)), ([0, 0], 4, 4, (129, 31))]
CAMS = [((0.0, 0.0, 0.0), 90.0, 0.0), ((0.0, 0.0, 0.0), -90.0, 0.0), ((0.5, 0.2, -1.0), 94.0, 1.0)]   # the middle one sees nothing


@pytest.mark.parametrize("fmt", [0, 1], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("devices,parts,band,size", MULTI_CASES)
def test_multi_sparse_matches_single_context(pkg, devices, parts, band, size, fmt):
    """RT_MULTI_SPARSE: three frames (one without any content) alternately into the object's own buffer (incremental assembly) and a
    caller's buffer (fill + scatter); each equals the single-context frame, and last_transfer() counts header + ids + count x tile per
    context, less than the dense transport on 20spheres where the bands are at least a tile high."""
    import torch
    w, h = size
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(w, h)
    ref = pkg.Renderer(sc, device=0, fmt=fmt)
    m = pkg.MultiRenderer(sc, devices, band_rows=band, parts=parts, fmt=fmt, flags=pkg.RT_MULTI_SPARSE)
    world = len(devices) * parts
    assert m.n_contexts == world
    assert m.transport == ("device copies" if len(devices) > 1 else "in place")
    bg = pkg.bg_rgba8(sc.arrays()["bg_color"]) if fmt else pkg.bg_rgba32f(sc.arrays()["bg_color"])
    pw = 1 if fmt else 4
    px_bytes = 4 * pw
    caller = torch.full((h, w, px_bytes), 0x77, dtype=torch.uint8, device="cuda:0")
    for rnd in range(2):   # own, caller, own / caller, own, caller
        for k, pose in enumerate(CAMS):
            cam = pkg.camera_matrix(*pose)
            ref.update(cam)
            want = ref.download()
            to_caller = (k + rnd) % 2 == 1
            m.update(cam, full_ptr=caller.data_ptr() if to_caller else None, timed=(k != 1))
            got = m.download()
            assert np.array_equal(got, want), (rnd, k, to_caller)
            if to_caller:
                torch.cuda.synchronize()
                assert np.array_equal(caller.cpu().numpy().view(want.dtype).reshape(want.shape), want)
            sent, dense = m.last_transfer()
            assert dense == w * h * px_bytes
            exp = _expected_sent(pkg, want, bg, h, w, band, world, pw, lambda c: pkg.lib().rt_sparse_msg_bytes(fmt, c))
            assert sent == exp, (rnd, k, sent, exp)
            if band >= 16:   # (4-row bands: each context's tiles are 3/4 padding rows, so its message can exceed its rows)
                assert sent < dense
    m.cleanup_update()


def test_multi_sparse_orders_writes_after_the_callers_work(pkg):
    """Two enqueue-only RT_MULTI_SPARSE frames into a caller's buffer with a device copy of that buffer enqueued on rt_multi_stream() in
    between: the copy holds frame 1 exactly (frame 2's fill + scatter wait for it)."""
    import torch
    w, h = 400, 277
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(w, h)
    ref = pkg.Renderer(sc, device=0, fmt=F32)
    m = pkg.MultiRenderer(sc, [0, 0], band_rows=8, parts=2, fmt=F32, flags=pkg.RT_MULTI_SPARSE)
    cam1, cam2 = pkg.camera_matrix((0.0, 0.0, 0.0), 90.0, 0.0), pkg.camera_matrix((1.0, 0.5, -2.0), 97.0, 2.0)
    ref.update(cam1)
    want1 = ref.download()
    ref.update(cam2)
    want2 = ref.download()
    assert not np.array_equal(want1, want2)
    a = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    b = torch.zeros_like(a)
    s = torch.cuda.ExternalStream(pkg.multi_lib().rt_multi_stream(m._h), device="cuda:0")
    for _ in range(2):
        m.update(cam1, full_ptr=a.data_ptr(), timed=False)
        with torch.cuda.stream(s):
            b.copy_(a)
        m.update(cam2, full_ptr=a.data_ptr(), timed=False)
        m.wait()
        torch.cuda.synchronize()
        assert np.array_equal(b.cpu().numpy(), want1)
        assert np.array_equal(a.cpu().numpy(), want2)


def test_multi_sparse_refusals(pkg):
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(64, 48)
    with pytest.raises(pkg.RtError) as e:
        pkg.MultiRenderer(sc, [0, 0], flags=pkg.RT_MULTI_SPARSE | pkg.RT_MULTI_BANDWISE)
    assert e.value.code == -1 and "RT_MULTI_BANDWISE" in e.value.message and "RT_MULTI_SPARSE" in e.value.message
    with pytest.raises(pkg.RtError) as e:
        pkg.MultiRenderer(sc, [0, 0], flags=pkg.RT_MULTI_SPARSE | pkg.RT_FLAG_SIMPLE)
    assert e.value.code == -1 and "RT_FLAG_SIMPLE" in e.value.message
    # the dense transports report bytes_sent == bytes_dense
    m = pkg.MultiRenderer(sc, [0, 0], parts=2, fmt=F32)
    assert m.last_transfer() == (0, 0)
    m.update()
    assert m.last_transfer() == (64 * 48 * 16, 64 * 48 * 16)
    m.cleanup_update()


_SELF_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import __graft_entry__ as graft
pkg = graft.load_package()
w, h = 320, 203
sc = pkg.Scene.load_from_file(sys.argv[2]).set_size(w, h)
for fmt in (0, 1):
    ref = pkg.Renderer(sc, device=0, fmt=fmt)
    m = pkg.MultiRenderer(sc, [0], band_rows=16, parts=2, fmt=fmt, flags=pkg.RT_MULTI_SELF_EXCHANGE | pkg.RT_MULTI_SPARSE)
    assert m.transport == "rccl", m.transport
    for pose in (((0.0, 0.0, 0.0), 90.0, 0.0), ((0.0, 0.0, 0.0), -90.0, 0.0), ((0.5, 0.2, -1.0), 94.0, 1.0)):
        cam = pkg.camera_matrix(*pose)
        ref.update(cam)
        m.update(cam)
        assert np.array_equal(m.download(), ref.download()), (fmt, pose)
        sent, dense = m.last_transfer()
        assert 0 < sent < dense, (sent, dense)
    m.cleanup_update()
print("self-exchange sparse ok")
"""


def test_multi_sparse_rccl_self_exchange(pkg):
    """SELF_EXCHANGE | SPARSE: one RCCL rank sends its used message prefixes to itself (a child process of its own, like the other RCCL
    tests); both formats, three frames including one without content."""
    p = subprocess.run([sys.executable, "-c", _SELF_CHILD, ROOT, scene_path("20spheres")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "self-exchange sparse ok" in p.stdout


@pytest.mark.parametrize("extra", [{"MI355RT_DEVICES": "0,0"}, {"MI355RT_DEVICES": "0", "MI355RT_MULTI_SELF": "1"}], ids=["devices00", "self"])
@pytest.mark.parametrize("fmt", ["rgba32f", "rgba8"])
def test_update_driver_with_multi_sparse(pkg, tmp_path, extra, fmt):
    """update.h driver with MI355RT_MULTI_SPARSE=1 produces the single-GPU frame (the same driver without a device list)."""
    assert os.path.exists(EXE)
    w, h = 320, 203
    outs = {}
    for label, env_extra in (("single", {}), ("sparse", dict(extra, MI355RT_MULTI_SPARSE="1", MI355RT_PARTS="2"))):
        out = str(tmp_path / f"{label}.bin")
        env = {k: v for k, v in os.environ.items() if not k.startswith("MI355RT_")}
        env.update(env_extra, MI355RT_FORMAT=fmt)
        p = subprocess.run([EXE, scene_path("20spheres"), str(w), str(h), "-1", out, "--frames", "3"], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, (label, p.stderr[-2000:])
        outs[label] = open(out, "rb").read()
    assert len(outs["single"]) == w * h * (4 if fmt == "rgba8" else 16)
    assert outs["sparse"] == outs["single"]


def test_update_driver_refuses_sparse_with_bandwise(pkg, tmp_path):
    env = dict(os.environ, MI355RT_DEVICES="0,0", MI355RT_MULTI_SPARSE="1", MI355RT_MULTI_BANDWISE="1")
    p = subprocess.run([EXE, scene_path("20spheres"), "64", "48", "-1", str(tmp_path / "x.bin")], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode != 0
    assert "MI355RT_MULTI_SPARSE" in p.stderr and "MI355RT_MULTI_BANDWISE" in p.stderr
