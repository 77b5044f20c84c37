#!/usr/bin/env python3
"""What the multi-GPU layer's G-buffer and scene update cost (results: profiles/multi_queries.txt).

1920 x 1080, 20spheres, strict, RGBA32F; devices [0, 0] x 2 parts (four contexts, device copies), band 16.  Synchronised calls, medians
of 31 after 5 warm-up calls, measured as tools/stream_bench.py measures:
  (a) rt_render_gbuffer_multi next to a single context's rt_render_gbuffer: the library's own event pair (device time on the root), and
      host wall time around the synchronised call;
  (b) rt_set_scene_multi + a frame next to rt_multi_destroy + rt_create_multi + a frame: host wall time from the first call to the
      frame being complete on the root (rt_multi_wait).

usage: multi_queries_bench.py [--out profiles/multi_queries.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

W, H, WARM, RUNS = 1920, 1080, 5, 31
DEVICES, PARTS, BAND = [0, 0], 2, 16


def med_us(samples):
    return float(np.median(samples)) * 1e6, float(min(samples)) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_queries.txt"))
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    sc = pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", "20spheres.yml")).set_size(W, H)
    a = sc.arrays()
    lines = [f"multi-GPU G-buffer and scene update, {W}x{H}, 20spheres, strict, RGBA32F; devices {DEVICES} x {PARTS} parts, band {BAND}; synchronised calls, "
             f"median of {RUNS} after {WARM} warm-up calls (us; min in brackets); {torch.cuda.get_device_name(0)}"]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    # (a) the G-buffer
    dev = torch.device("cuda", 0)
    po = torch.empty((H, W), dtype=torch.int32, device=dev)
    pt = torch.empty((H, W), dtype=torch.float64, device=dev)
    pn = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ptrs = (po.data_ptr(), pt.data_ptr(), pn.data_ptr())

    def gbuffer_times(call):
        for _ in range(WARM):
            call()
        dev_ms, wall = [], []
        for _ in range(RUNS):
            t0 = time.perf_counter()
            dev_ms.append(call() * 1e-3)
            wall.append(time.perf_counter() - t0)
        return med_us(dev_ms), med_us(wall)

    single = pkg.Renderer(sc, device=0)
    (sd, sd_lo), (sw, sw_lo) = gbuffer_times(lambda: single.gbuffer_into(None, *ptrs, timed=True))
    single.cleanup_update()
    m = pkg.MultiRenderer(sc, DEVICES, band_rows=BAND, parts=PARTS)
    (md, md_lo), (mw, mw_lo) = gbuffer_times(lambda: m.gbuffer_into(None, *ptrs, timed=True))
    say("(a) three planes (28 bytes per pixel): device time by the event pair | host wall time of the synchronised call")
    say(f"    rt_render_gbuffer, one context        {sd:10.1f} [{sd_lo:10.1f}] | {sw:10.1f} [{sw_lo:10.1f}]")
    say(f"    rt_render_gbuffer_multi               {md:10.1f} [{md_lo:10.1f}] | {mw:10.1f} [{mw_lo:10.1f}]   x{md / sd:5.2f} | x{mw / sw:5.2f}")

    # (b) a new scene and its first frame: two scenes in turn, so that every update changes something
    scenes = [a, dict(a, coefs=a["coefs"].copy())]
    for q in scenes[1]["coefs"]:   # every sphere a quarter of a unit along x: centre c = -k / 2, r^2 = c.c - constant
        c = -0.5 * q[16:19]
        r2 = float(np.dot(c, c)) - q[19]
        c = c + np.array([0.25, 0.0, 0.0])
        q[16:19] = -2.0 * c
        q[19] = float(np.dot(c, c)) - r2
    keys = ("coefs", "reflection", "albedo", "light_p", "light_color")

    def update_and_frame(k):
        t0 = time.perf_counter()
        m.set_scene(**{n: scenes[k % 2][n] for n in keys})
        m.update(None, timed=False)
        m.wait()
        return time.perf_counter() - t0

    for k in range(WARM):
        update_and_frame(k)
    upd, upd_lo = med_us([update_and_frame(k) for k in range(RUNS)])
    st = m.set_scene_status()
    assert st["rejected"] == 0 and st["applied"] == WARM + RUNS, st
    descs = [pkg.desc_from_arrays(s["width"], s["height"], s["vertical_fov"], s["bg_color"], s["max_reflections"], s["coefs"], s["reflection"], s["albedo"],
                                  s["light_is_spherical"], s["light_p"], s["light_color"]) for s in scenes]
    box = [m]

    def recreate_and_frame(k):
        t0 = time.perf_counter()
        box[0].cleanup_update()
        box[0] = pkg.MultiRenderer(descs[k % 2], DEVICES, band_rows=BAND, parts=PARTS)
        box[0].update(None, timed=False)
        box[0].wait()
        return time.perf_counter() - t0

    for k in range(WARM):
        recreate_and_frame(k)
    rec, rec_lo = med_us([recreate_and_frame(k) for k in range(RUNS)])
    box[0].cleanup_update()
    say("(b) a moved scene and its first frame, host wall time until the frame is complete on the root")
    say(f"    rt_set_scene_multi + frame            {upd:10.1f} [{upd_lo:10.1f}]")
    say(f"    destroy + rt_create_multi + frame     {rec:10.1f} [{rec_lo:10.1f}]   x{rec / upd:5.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
