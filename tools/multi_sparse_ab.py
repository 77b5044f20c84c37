#!/usr/bin/env python3
"""rt_render_multi on a one-GPU box (device list [0, 0, 0, 0] x 2 parts = 8 contexts, device copies instead of RCCL): the classic transport
(rows into rank-major slots, then rt_assemble), RT_MULTI_BANDWISE (one strided copy per context into the frame) and RT_MULTI_SPARSE
(render + pack per context, the host waits for the message headers, only the used prefixes travel, the root scatters the tiles),
alternated frame by frame in one process.  `ms` is rt_render_multi's own figure: device time on the root from the start of its render to
the complete frame.  last_transfer() gives the bytes each transport delivered to the root's reassembly.

On one GPU every "transfer" is an HBM copy, so this measures the sparse path's OVERHEADS (host header wait, pack, scatter) against the
dense copies it replaces -- not the xGMI saving, which only a multi-GPU node can measure.

It also measures, per rank, what RGBA32F costs through rt_render_sparse (one kernel, general schedule) against rt_render + rt_pack_sparse
(which keeps the wave-per-block schedule): the reason the multi layer packs.
usage: python tools/multi_sparse_ab.py [frames]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
import torch  # noqa: E402

FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 21
SIZES = ((3840, 2160), (7680, 4320))
TRANSPORTS = (("classic", 0), ("bandwise", pkg.RT_MULTI_BANDWISE), ("sparse", pkg.RT_MULTI_SPARSE))


def rank_level(sc, w, h):
    """one rank of 8 (band 16), RGBA32F: rt_render_sparse vs rt_render + rt_pack_sparse, device ms per frame (median)."""
    ren = pkg.Renderer(sc, device=0, rank=0, world=8, band_rows=16, fmt=pkg.RT_FMT_RGBA32F)
    cap = ((w + 15) // 16) * ((ren.local_rows + 15) // 16)
    msg = torch.empty(ren.sparse_msg_bytes(cap), dtype=torch.uint8, device="cuda:0")
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.current_stream().cuda_stream
    res = {"render_sparse": [], "render+pack": []}
    for k in range(4 + FRAMES):
        for label in res:
            start.record()
            if label == "render_sparse":
                ren.update_sparse(msg.data_ptr(), cap, stream=stream, timed=False)
            else:
                ren.update(stream=stream, timed=False)
                ren.pack_sparse(msg.data_ptr(), cap, stream=stream)
            end.record()
            end.synchronize()
            if k >= 4:
                res[label].append(start.elapsed_time(end))
    ren.cleanup_update()
    return {k: float(np.median(v)) for k, v in res.items()}


for W, H in SIZES:
    sc = pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", "20spheres.yml")).set_size(W, H)
    for fmt, name in ((pkg.RT_FMT_RGBA32F, "rgba32f"), (pkg.RT_FMT_RGBA8, "rgba8")):
        single = pkg.Renderer(sc, device=0, fmt=fmt)
        for _ in range(4):
            single.update()
        t_single = float(np.median([single.update() for _ in range(FRAMES)]))
        want = single.download()
        single.cleanup_update()
        ms = {label: [] for label, _ in TRANSPORTS}
        objs = {label: pkg.MultiRenderer(sc, [0, 0, 0, 0], band_rows=16, parts=2, fmt=fmt, flags=flags) for label, flags in TRANSPORTS}
        for k in range(4 + FRAMES):   # alternated: every transport sees the same clocks and the same thermal state
            for label, m in objs.items():
                t = m.update()
                if k >= 4:
                    ms[label].append(t)
        moved = {}
        for label, m in objs.items():
            assert np.array_equal(m.download(), want), (W, H, name, label)
            moved[label] = m.last_transfer()
            m.cleanup_update()
        med = {label: float(np.median(v)) for label, v in ms.items()}
        print(f"20spheres {W}x{H} {name}: one context {t_single * 1e3:.0f} us; 8 contexts on one GPU (median of {FRAMES} frames, root ms per frame):")
        for label, _ in TRANSPORTS:
            sent, dense = moved[label]
            print(f"  {label:9s} {med[label] * 1e3:7.0f} us   to the root {sent / 1e6:8.2f} MB of {dense / 1e6:8.2f} MB dense ({100.0 * sent / dense:5.1f} %)")
        torch.cuda.synchronize()
    rl = rank_level(sc, W, H)
    print(f"  rank 0 of 8, rgba32f: rt_render_sparse {rl['render_sparse'] * 1e3:.0f} us   rt_render + rt_pack_sparse {rl['render+pack'] * 1e3:.0f} us")
