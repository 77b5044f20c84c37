#!/usr/bin/env python3
"""Cost of rt_trace_paths and rt_primary_rays (csrc/rt_paths.hip) next to rt_trace_rays and rt_shade_rays of the same context.

  python tools/paths_bench.py [--calls N] [--warmup W]
      One process; per scene at 1920 x 1080, start pose, strict RGBA32F context: the frame's own primary rays from rt_primary_rays, in
      pixel order and in a fixed random permutation.  The calls alternate -- rt_primary_rays, then per order rt_trace_rays (one
      segment: the floor), rt_trace_paths with max_segments = max_reflections + 1 and with max_segments = 0 (ends and last only),
      rt_shade_rays (the same bounces plus the lights) -- every call synchronised and timed by the library's own event pair, W warm-up
      rounds first, median of N.  Output: device microseconds and the paths' ratio to the two yardsticks.  Rows: 20spheres and the
      mirror configuration (reflection_test, reflection depth 4).  No condition is checked: these are readings.
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
    n = W * H
    print(f"device us per call (the library's event pair around its kernels), median of {a.calls} synchronised calls after {a.warmup} warm-up rounds; "
          f"calls of one row alternate in one process; {W}x{H}, start pose, strict RGBA32F; {torch.cuda.get_device_name(0)}")
    print("bytes per ray: rt_primary_rays 48 out; rt_trace_rays 48 in, 48 out; rt_trace_paths 48 in, 48 per plane + 48 (last) + 16 (ends) out; rt_shade_rays 48 in, 16 out")
    print(f"{'scene':<18} {'order':<9} {'primary':>8} {'GB/s':>6} {'trace':>8} {'paths':>8} {'x trace':>8} {'x shade':>8} {'paths M=0':>10} {'x trace':>8} {'shade':>8} {'segments mean / max':>20}")
    for name, depth in (("20spheres", None), ("reflection_test", 4)):
        sc = pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", name + ".yml")).set_size(W, H)
        if depth is not None:
            sc.set_max_reflections(depth)
        m = sc.desc().max_reflections + 1
        r = pkg.Renderer(sc, device=0)
        d_ord = torch.empty((n, 6), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        r.primary_rays_into(None, None, d_ord.data_ptr())
        perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).to("cuda:0")
        d_shuf = d_ord[perm].contiguous()
        seg = torch.empty((m * n, 6), dtype=torch.float64, device="cuda:0")
        last = torch.empty((n, 6), dtype=torch.float64, device="cuda:0")
        ends = torch.empty((n, 4), dtype=torch.int32, device="cuda:0")
        rgba = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        for label, d in (("ordered", d_ord), ("shuffled", d_shuf)):
            calls = [lambda: r.primary_rays_into(None, None, d_ord.data_ptr()),
                     lambda: r.trace_into(d.data_ptr(), n, last.data_ptr()),
                     lambda: r.paths_into(d.data_ptr(), n, m, seg.data_ptr(), last.data_ptr(), ends.data_ptr()),
                     lambda: r.paths_into(d.data_ptr(), n, 0, None, last.data_ptr(), ends.data_ptr()),
                     lambda: r.shade_into(d.data_ptr(), n, rgba.data_ptr())]
            for _ in range(a.warmup):
                for c in calls:
                    c()
            ms = [[] for _ in calls]
            for _ in range(a.calls):
                for i, c in enumerate(calls):
                    ms[i].append(c())
            us = [1e3 * float(np.median(x)) for x in ms]
            segs = ends[:, 0].cpu().numpy()
            print(f"{name + (f' depth {depth}' if depth is not None else ''):<18} {label:<9} {us[0]:8.1f} {48.0 * n / us[0] / 1e3:6.0f} {us[1]:8.1f} {us[2]:8.1f} {us[2] / us[1]:8.2f} "
                  f"{us[2] / us[4]:8.2f} {us[3]:10.1f} {us[3] / us[1]:8.2f} {us[4]:8.1f} {segs.mean():13.3f} / {int(segs.max())}", flush=True)
        r.cleanup_update()
    return 0


if __name__ == "__main__":
    sys.exit(main())
