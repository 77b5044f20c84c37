#!/usr/bin/env python3
"""Cost of the primary-hit G-buffer pass (rt_render_gbuffer, csrc/rt_gbuffer.hip) next to a colour frame of the same pose.

  python tools/gbuffer_bench.py [--calls N] [--warmup W]
      In one process, per scene and size: a default context (the product render kernels) and an RT_FLAG_SIMPLE context (the
      one-thread-per-pixel tracer).  For each pose the calls alternate -- colour frame (product), colour frame (simple), G-buffer with
      all three planes, then each plane alone -- every call synchronised and timed by the library's own event pair (device time of
      the kernels), W warm-up rounds first, median of N.  Output: device microseconds, the bytes a pass writes and the store rate
      that implies.  Rows: 20spheres at 1080p and 4K, clebsch at 1080p; start pose and pose 16 of a 24-pose orbit (20spheres: the orbit
      of tools/flythrough_bench.py; clebsch: radius 6 around the origin).
      Condition: the three-plane pass is faster than the RT_FLAG_SIMPLE colour frame on every row.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

CONFIGS = [("20spheres", 1920, 1080), ("20spheres", 3840, 2160), ("clebsch", 1920, 1080)]
ORBITS = {"20spheres": ((5.0, 2.0, 15.0), 14.0), "clebsch": ((0.0, 0.0, 0.0), 6.0)}   # centre, radius


def orbit_pose(pkg, name, i, n=24):
    (cx, cy, cz), rad = ORBITS[name]
    a = 2.0 * np.pi * i / n
    pos = (cx + rad * np.sin(a), cy + 2.0 * np.sin(2 * a), cz - rad * np.cos(a))
    yaw = float(np.degrees(np.arctan2(cz - pos[2], cx - pos[0])))
    pitch = float(-np.degrees(np.arctan2(pos[1] - cy, rad)))
    return pkg.camera_matrix(pos, yaw, pitch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    pkg = graft.load_package()
    print(f"device us per call (the library's event pair around its kernels), median of {a.calls} synchronised calls after {a.warmup} warm-up rounds; "
          f"calls of one row alternate in one process; {torch.cuda.get_device_name(0)}")
    print(f"{'scene':<10} {'size':>10} {'pose':>6} {'colour':>9} {'simple':>9} {'gbuffer':>9} {'object':>8} {'t':>8} {'normal':>8} {'MB':>7} {'GB/s':>7} {'hit px':>8}  gb<simple  gb<=colour")
    ok = True
    for name, w, h in CONFIGS:
        sc = pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", name + ".yml")).set_size(w, h)
        prod, simple = pkg.Renderer(sc, device=0), pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_SIMPLE)
        po = torch.empty((h, w), dtype=torch.int32, device="cuda:0")
        pt = torch.empty((h, w), dtype=torch.float64, device="cuda:0")
        pn = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        for pose, cam in (("start", None), ("orb16", orbit_pose(pkg, name, 16))):
            calls = [lambda: prod.update(cam), lambda: simple.update(cam),
                     lambda: prod.gbuffer_into(cam, po.data_ptr(), pt.data_ptr(), pn.data_ptr()),
                     lambda: prod.gbuffer_into(cam, po.data_ptr(), None, None), lambda: prod.gbuffer_into(cam, None, pt.data_ptr(), None),
                     lambda: prod.gbuffer_into(cam, None, None, pn.data_ptr())]
            for _ in range(a.warmup):
                for c in calls:
                    c()
            ms = [[] for _ in calls]
            for _ in range(a.calls):
                for i, c in enumerate(calls):
                    ms[i].append(c())
            us = [1e3 * float(np.median(m)) for m in ms]
            prod.gbuffer_into(cam, po.data_ptr(), pt.data_ptr(), pn.data_ptr())
            hits = int((po >= 0).sum().item())
            mb = w * h * 28 / 1e6
            row_ok = us[2] < us[1]
            ok = ok and row_ok
            print(f"{name:<10} {w:>5}x{h:<4} {pose:>6} {us[0]:9.1f} {us[1]:9.1f} {us[2]:9.1f} {us[3]:8.1f} {us[4]:8.1f} {us[5]:8.1f} {mb:7.1f} {mb / us[2] * 1e3:7.0f} {hits:8d}"
                  f"  {'yes' if row_ok else 'NO':>9}  {'yes' if us[2] <= us[0] else f'no ({us[2] / us[0]:.2f}x)':>10}", flush=True)
        prod.cleanup_update()
        simple.cleanup_update()
    print("condition (G-buffer pass faster than the RT_FLAG_SIMPLE colour frame on every row):", "holds" if ok else "VIOLATED")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
