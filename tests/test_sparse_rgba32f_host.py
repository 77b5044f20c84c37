"""Sparse transport of RGBA32F frames, host side: message sizes (rt_sparse_msg_bytes needs no context, so no GPU) and the
numpy mirrors of rt_pack_sparse / rt_assemble_sparse through a gloo gather, with the oracle standing in for the renderer.
The rebuilt float frame must equal the oracle's frame (alpha 1.0) bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_sharding import _free_port

CAPACITIES = (0, 1, 3, 4, 5, 16200)


def test_sparse_msg_bytes(pkg):
    L = pkg.lib()
    for cap in CAPACITIES:
        assert L.rt_sparse_msg_bytes(pkg.RT_FMT_RGBA8, cap) == L.rt_sparse_bytes(cap)
        f32 = L.rt_sparse_msg_bytes(pkg.RT_FMT_RGBA32F, cap)
        assert f32 == 16 * ((4 + cap + 3) // 4) + 4096 * cap
        assert f32 % 16 == 0 and L.rt_sparse_bytes(cap) % 16 == 0
        assert f32 == 4 * pkg.sparse_words(cap, 4) and L.rt_sparse_bytes(cap) == 4 * pkg.sparse_words(cap)
    for fmt in (2, 7, 0xFFFFFFFF):
        assert L.rt_sparse_msg_bytes(fmt, 4) == 0


def test_new_symbols_are_in_the_binding_lists(pkg):
    assert "rt_sparse_msg_bytes" in pkg.ABI_SYMBOLS and "rt_multi_last_transfer" in pkg.MULTI_ABI_SYMBOLS
    assert pkg.RT_MULTI_SPARSE == 0x40000
    hdr = open(f"{ROOT}/include/mi355rt.h").read()
    assert "#define RT_MULTI_SPARSE 0x40000u" in hdr and "#define RT_ABI_VERSION 3" in hdr
    C.CDLL(pkg.MULTI_LIB_PATH).rt_multi_last_transfer   # exported


def test_numpy_mirror_round_trip_rgba32f():
    """pack / assemble mirrors on a synthetic frame: background bit-equal to (bg, 1.0f) is dropped, anything else (a -0.0 in
    place of 0.0, a different alpha) is content; width not a multiple of 16, bands that cut through tiles."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("sharding_mirror", os.path.join(ROOT, "cuda-ray-tracer_amd", "sharding.py"))
    sh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sh)
    w, h, band, world = 37, 45, 5, 3
    bg_color = (0.0, 0.25, 0.5)
    bg = sh.bg_rgba32f(bg_color)
    full = np.empty((h, w, 4), np.float32)
    full[...] = np.array(bg_color + (1.0,), np.float32)
    full[3, 2] = (0.1, 0.2, 0.3, 1.0)
    full[40, 36, 0] = -0.0          # differs from the background only in its bits
    full[22, 17, 3] = 0.5           # alpha
    mx = sh.max_local_rows(h, band, world)
    cap = ((w + 15) // 16) * ((mx + 15) // 16)
    msgs = []
    for r in range(world):
        rows = sh.band_rows_of_rank(h, band, world, r)
        m = sh.pack_sparse_numpy(full[rows], len(rows), bg, cap)
        assert m.size == sh.sparse_words(cap, 4) and m[1] == 0
        msgs.append(m)
    assert sum(int(m[0]) for m in msgs) == 3
    got = sh.assemble_sparse_numpy(np.stack(msgs), w, h, band, world, bg, cap)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), full.view(np.uint32))
    # a too-small capacity only raises overflow
    rows = sh.band_rows_of_rank(h, band, world, 0)
    small = sh.pack_sparse_numpy(full[rows] + np.float32(1.0), len(rows), bg, 1)
    assert small[1] == 1 and small[0] > 1


def _sparse_f32_worker(rank, world, port, h, w, band, cap, out_path):
    import sys
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as graft
    pkg, O = graft.load_package(), graft.load_oracle()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    sc = O.load_scene(scene_path("20spheres")).with_size(w, h)
    rows = pkg.band_rows_of_rank(h, band, world, rank)
    img = sc.render(rows=rows) if len(rows) else np.zeros((0, w, 3), dtype=np.float32)
    rgba = np.concatenate([img.astype(np.float32), np.ones(img.shape[:2] + (1,), np.float32)], axis=-1)
    bg = pkg.bg_rgba32f(sc.bg_color)
    msg = torch.from_numpy(pkg.pack_sparse_numpy(rgba, len(rows), bg, cap).view(np.int32).copy())
    gathered = pkg.gather_to_root(msg, world, rank)
    if rank == 0:
        full = pkg.assemble_sparse_numpy(gathered.numpy().view(np.uint32), w, h, band, world, bg, cap)
        np.save(out_path, full)
        np.save(out_path + ".counts.npy", gathered.numpy().view(np.uint32)[:, 0])
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,h,band", [(2, 60, 8), (3, 50, 5)])
def test_gloo_sparse_gather_rebuilds_the_float_frame(oracle, tmp_path, world, h, band):
    """RGBA32F messages (16-byte pixels) through the gather: the rebuilt frame is the oracle's float frame with alpha 1.0, bit for
    bit; width 90 (not a multiple of 16) and band heights that cut through 16-row tiles."""
    import torch.multiprocessing as mp
    w = 90
    out = str(tmp_path / "full.npy")
    cap = ((w + 15) // 16) * ((h + 15) // 16)
    mp.spawn(_sparse_f32_worker, args=(world, _free_port(), h, w, band, cap, out), nprocs=world, join=True)
    want = oracle.load_scene(scene_path("20spheres")).with_size(w, h).render()
    got = np.load(out)
    assert got.dtype == np.float32
    assert np.array_equal(got[..., :3].view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert np.all(got[..., 3] == 1.0)
    counts = np.load(out + ".counts.npy")
    assert 0 < counts.sum() < world * cap   # some tiles travelled, not all
