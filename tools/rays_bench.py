#!/usr/bin/env python3
"""Cost of the ray queries (rt_trace_rays / rt_occluded_rays, csrc/rt_rays.hip) next to the G-buffer pass of the same context.

  python tools/rays_bench.py [--calls N] [--warmup W]
      One process; per scene at 1920 x 1080, start pose: the frame's primary rays uploaded as explicit rays in pixel order (a) and in a
      fixed random permutation (b), and the frame's shadow rays, formed on the host from the G-buffer planes as include/mi355rt.h
      describes (hit x light, bias 1e-2 along the float normal, the direction through float) (c).  The calls alternate -- G-buffer with
      three planes, trace ordered, trace shuffled, occlusion -- every call synchronised and timed by the library's own event pair, W
      warm-up rounds first, median of N.  Output: device microseconds, rays per second, the ratio to the G-buffer pass, bytes moved
      per ray.  Rows: 20spheres and clebsch (d).  No condition is checked: these are readings.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

W, H = 1920, 1080


def primary_rays(desc):
    """The reference's primary directions for the identity camera (src/update-cpu.cpp:84-89), numpy float64."""
    th = np.tan(0.5 * desc["vertical_fov"])
    cx = (2.0 * ((np.arange(W) + 0.5) / W) - 1.0) * (float(W) / float(H)) * th
    cy = (2.0 * ((np.arange(H) + 0.5) / H) - 1.0) * th
    wx, wy, wz = np.broadcast_to(cx, (H, W)), np.broadcast_to(cy[:, None], (H, W)), np.ones((H, W))
    inv = 1.0 / np.sqrt((wx * wx + wy * wy) + wz * wz)
    rays = np.zeros((H * W, 6))
    rays[:, 3:] = np.stack([wx * inv, wy * inv, wz * inv], axis=-1).reshape(-1, 3)
    return rays


def shadow_rays(desc, rays, obj, t, nrm):
    """hit x light shadow rays from the planes: o = p + 1e-2 * n, d through float, t_max 1.0 (point light) or 1e6."""
    hit = obj.reshape(-1) >= 0
    p = rays[hit, 3:] * t.reshape(-1)[hit][:, None]
    n = nrm.reshape(-1, 4)[hit, :3].astype(np.float64)
    out, tmax = [], []
    for k in range(len(desc["light_is_spherical"])):
        lp = desc["light_p"][k]
        d = (lp - p) if desc["light_is_spherical"][k] else np.broadcast_to(lp, p.shape)
        out.append(np.concatenate([p + 1e-2 * n, d.astype(np.float32).astype(np.float64)], axis=1))
        tmax.append(np.full(len(p), 1.0 if desc["light_is_spherical"][k] else 1e6))
    return np.stack(out, axis=1).reshape(-1, 6), np.stack(tmax, axis=1).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    pkg = graft.load_package()
    print(f"device us per call (the library's event pair around its kernel), median of {a.calls} synchronised calls after {a.warmup} warm-up rounds; "
          f"calls of one row alternate in one process; {W}x{H}, start pose; {torch.cuda.get_device_name(0)}")
    print("bytes per ray: trace 96 (48 in, 48 out), occlusion 60 (48 + 8 in, 4 out); the G-buffer pass writes 28 per pixel")
    print(f"{'scene':<10} {'gbuffer':>9} {'ordered':>9} {'x gb':>6} {'Mray/s':>8} {'shuffled':>9} {'x gb':>6} {'Mray/s':>8} {'shadow rays':>12} {'occluded':>9} {'Mray/s':>8} {'blocked':>9}")
    for name in ("20spheres", "clebsch"):
        sc = pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", name + ".yml")).set_size(W, H)
        desc = sc.arrays()
        r = pkg.Renderer(sc, device=0)
        po, pt, pn, _ = r.gbuffer()
        rays = primary_rays(desc)
        srays, tmax = shadow_rays(desc, rays, po.cpu().numpy(), pt.cpu().numpy(), pn.cpu().numpy())
        perm = np.random.default_rng(1).permutation(len(rays))
        d_ord, d_shuf, d_sh, d_tm = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (rays, rays[perm], srays, tmax))
        hits = torch.empty((len(rays), 6), dtype=torch.float64, device="cuda:0")
        blocked = torch.empty((len(srays),), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        calls = [lambda: r.gbuffer_into(None, po.data_ptr(), pt.data_ptr(), pn.data_ptr()),
                 lambda: r.trace_into(d_ord.data_ptr(), len(rays), hits.data_ptr()),
                 lambda: r.trace_into(d_shuf.data_ptr(), len(rays), hits.data_ptr()),
                 lambda: r.occluded_into(d_sh.data_ptr(), d_tm.data_ptr(), len(srays), blocked.data_ptr())]
        for _ in range(a.warmup):
            for c in calls:
                c()
        ms = [[] for _ in calls]
        for _ in range(a.calls):
            for i, c in enumerate(calls):
                ms[i].append(c())
        us = [1e3 * float(np.median(m)) for m in ms]
        nb = int(blocked.sum().item())
        print(f"{name:<10} {us[0]:9.1f} {us[1]:9.1f} {us[1] / us[0]:6.2f} {len(rays) / us[1]:8.0f} {us[2]:9.1f} {us[2] / us[0]:6.2f} {len(rays) / us[2]:8.0f} "
              f"{len(srays):12d} {us[3]:9.1f} {len(srays) / us[3]:8.0f} {nb:9d}", flush=True)
        r.cleanup_update()
    return 0


if __name__ == "__main__":
    sys.exit(main())
