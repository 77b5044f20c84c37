#!/usr/bin/env python3
"""Cost of rt_object_extents (csrc/rt_gbuffer.hip, extents_kernel) next to the G-buffer pass of the same context.

  python tools/extents_bench.py [--calls N] [--warmup W]
      One process; per scene at 1920 x 1080, start pose: the three-plane G-buffer pass (the yardstick: the same rays, 28 bytes written
      per pixel), rt_object_extents over the full frame (40 bytes per object written) and over a 64 x 64 rectangle in the middle of
      the frame.  The calls alternate, every call synchronised and timed by the library's own event pair, W warm-up rounds first,
      median of N.  Output: device microseconds and the ratio to the G-buffer pass.  Rows: 20spheres and clebsch.  No condition is
      checked: these are readings.
  It is one GPU step and runs under a limit of its own, as profiles/extents.txt was taken:
      timeout -k 10 120 python tools/extents_bench.py
  (under a profiler the same: timeout -k 10 240 rocprofv3 --kernel-trace --stats -d DIR -- python tools/extents_bench.py --calls 9 --warmup 2)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    pkg = graft.load_package()
    print(f"device us per call (the library's event pair around its kernels), median of {a.calls} synchronised calls after {a.warmup} warm-up rounds; "
          f"calls of one row alternate in one process; {W}x{H}, start pose; {torch.cuda.get_device_name(0)}")
    print(f"{'scene':<10} {'objects':>8} {'seen':>5} {'gbuffer':>9} {'extents':>9} {'x gb':>6} {'64x64':>9} {'x gb':>6}")
    rect = (W // 2 - 32, H // 2 - 32, W // 2 + 31, H // 2 + 31)
    for name in ("20spheres", "clebsch"):
        sc = pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", name + ".yml")).set_size(W, H)
        r = pkg.Renderer(sc, device=0)
        po, pt, pn, _ = r.gbuffer()
        n = sc.desc().n_objects
        out = torch.zeros((n * 5,), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        calls = [lambda: r.gbuffer_into(None, po.data_ptr(), pt.data_ptr(), pn.data_ptr()),
                 lambda: r.object_extents_into(None, None, out.data_ptr()),
                 lambda: r.object_extents_into(None, rect, out.data_ptr())]
        for _ in range(a.warmup):
            for c in calls:
                c()
        ms = [[] for _ in calls]
        for _ in range(a.calls):
            for i, c in enumerate(calls):
                ms[i].append(c())
        us = [1e3 * float(np.median(m)) for m in ms]
        seen = int((r.object_extents()["pixels"] > 0).sum())
        print(f"{name:<10} {n:8d} {seen:5d} {us[0]:9.1f} {us[1]:9.1f} {us[1] / us[0]:6.2f} {us[2]:9.1f} {us[2] / us[0]:6.2f}", flush=True)
        r.cleanup_update()
    return 0


if __name__ == "__main__":
    sys.exit(main())
