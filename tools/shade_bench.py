#!/usr/bin/env python3
"""Cost of rt_shade_rays (csrc/rt_shade_rays.hip) next to rt_render of the same context.

  python tools/shade_bench.py [--calls N] [--warmup W]
      One process; per scene at 1920 x 1080, start pose, strict RGBA32F context: the frame's own primary rays uploaded as explicit rays
      in pixel order (a) and in a fixed random permutation (b), shaded without and with the hit records.  The calls alternate --
      rt_render, shade ordered, shade shuffled, shade ordered with hits -- every call synchronised and timed by the library's own
      event pair, W warm-up rounds first, median of N.  Output: device microseconds, rays per second, the ratio to the frame, bytes
      moved per ray.  Rows: 20spheres and the mirror configuration (reflection_test, reflection depth 4).  The ordered colours are
      compared with the frame once and the outcome is printed; no condition is checked: these are readings.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as graft  # noqa: E402
from rays_bench import H, W, primary_rays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    pkg = graft.load_package()
    print(f"device us per call (the library's event pair around its kernels), median of {a.calls} synchronised calls after {a.warmup} warm-up rounds; "
          f"calls of one row alternate in one process; {W}x{H}, start pose, strict RGBA32F; {torch.cuda.get_device_name(0)}")
    print("bytes per ray: 64 (48 in, 16 out), 112 with hits (48 more out); the frame writes 16 per pixel and reads no rays")
    print(f"{'scene':<18} {'rt_render':>9} {'ordered':>9} {'x frame':>8} {'Mray/s':>8} {'shuffled':>9} {'x frame':>8} {'Mray/s':>8} {'with hits':>10} {'x frame':>8} {'= frame':>8}")
    for name, depth in (("20spheres", None), ("reflection_test", 4)):
        sc = pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", name + ".yml")).set_size(W, H)
        if depth is not None:
            sc.set_max_reflections(depth)
        r = pkg.Renderer(sc, device=0)
        rays = primary_rays(sc.arrays())
        perm = np.random.default_rng(1).permutation(len(rays))
        d_ord, d_shuf = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (rays, rays[perm]))
        rgba = torch.empty((len(rays), 4), dtype=torch.float32, device="cuda:0")
        hits = torch.empty((len(rays), 6), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        r.update()
        r.shade_into(d_ord.data_ptr(), len(rays), rgba.data_ptr())
        same = bool(np.array_equal(rgba.cpu().numpy().view(np.uint32).reshape(H, W, 4), r.download().view(np.uint32)))
        calls = [lambda: r.update(),
                 lambda: r.shade_into(d_ord.data_ptr(), len(rays), rgba.data_ptr()),
                 lambda: r.shade_into(d_shuf.data_ptr(), len(rays), rgba.data_ptr()),
                 lambda: r.shade_into(d_ord.data_ptr(), len(rays), rgba.data_ptr(), hits.data_ptr())]
        for _ in range(a.warmup):
            for c in calls:
                c()
        ms = [[] for _ in calls]
        for _ in range(a.calls):
            for i, c in enumerate(calls):
                ms[i].append(c())
        us = [1e3 * float(np.median(m)) for m in ms]
        label = name + (f" depth {depth}" if depth is not None else "")
        print(f"{label:<18} {us[0]:9.1f} {us[1]:9.1f} {us[1] / us[0]:8.2f} {len(rays) / us[1]:8.0f} {us[2]:9.1f} {us[2] / us[0]:8.2f} {len(rays) / us[2]:8.0f} "
              f"{us[3]:10.1f} {us[3] / us[0]:8.2f} {'yes' if same else 'NO':>8}", flush=True)
        r.cleanup_update()
    return 0


if __name__ == "__main__":
    sys.exit(main())
