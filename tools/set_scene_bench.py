#!/usr/bin/env python3
"""What a scene update costs (results: profiles/set_scene.txt).

  1. device time of one rt_set_scene kernel, 20spheres and a 1 000-sphere scene (hipEvent pair around R back-to-back kernels / R);
  2. per-frame time of a captured (rt_set_scene, rt_render) x K graph against the same graph without the updates, alternating;
  3. rt_destroy + rt_create of the same scene: the round trip the update replaces (host wall time, device idle before and after).

usage: set_scene_bench.py [--width 1920 --height 1080] [--frames 30] [--rounds 7]
With --create-only it measures (3) alone and needs no scene-update entry point, so it also runs on a build that has none."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def sphere_field(pkg, n, w, h):
    rng = np.random.default_rng(11)
    s = pkg.Scene.new(w, h, 60.0, 0, (0.0, 0.1, 0.2))
    for _ in range(n):
        s.add_object(pkg.surface_make("sphere", rng.uniform([-40, -25, 20], [40, 25, 120]), [float(rng.uniform(0.3, 1.2))]), rng.uniform(0, 1, 3))
    s.add_light("directional", (0.3, -1.0, 0.4), (1, 1, 1), 1.0)
    s.add_light("spherical", (0.0, 30.0, 10.0), (1, 0.9, 0.8), 900.0)
    return s


def median(v):
    return float(np.median(np.asarray(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--create-only", action="store_true")
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    scenes = {"20spheres": pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", "20spheres.yml")).set_size(args.width, args.height),
              "1000spheres": sphere_field(pkg, 1000, args.width, args.height)}
    cam = pkg.IDENTITY.copy()
    for name, sc in scenes.items():
        # (3) the round trip
        r = pkg.Renderer(sc, device=0)
        r.update(cam)
        trips = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.cleanup_update()
            r = pkg.Renderer(sc, device=0)
            torch.cuda.synchronize()
            trips.append((time.perf_counter() - t0) * 1e6)
        print(f"{name}: rt_destroy + rt_create {median(trips):9.1f} us (median of {args.rounds}, min {min(trips):.1f})")
        if args.create_only:
            r.cleanup_update()
            continue
        a = sc.arrays()
        s = torch.cuda.Stream()
        dev = torch.from_numpy(a["coefs"].copy()).to("cuda:0")
        torch.cuda.synchronize()
        r.update(cam, stream=s.cuda_stream, timed=False)
        # (1) the kernel alone
        reps, e0, e1 = 50, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        per = []
        for _ in range(args.rounds):
            with torch.cuda.stream(s):
                e0.record()
                for _ in range(reps):
                    r.set_scene_into(coefs=dev.data_ptr(), stream=s.cuda_stream)
                e1.record()
            s.synchronize()
            per.append(e0.elapsed_time(e1) * 1e3 / reps)
        st = r.set_scene_status()
        assert st["rejected"] == 0 and st["applied"] == reps * args.rounds, st
        print(f"{name}: rt_set_scene kernel      {median(per):9.2f} us per launch, back to back (median of {args.rounds} x {reps})")
        # (2) captured sequences with and without the updates, alternating
        graphs = {}
        for with_update in (False, True):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                for _ in range(args.frames):
                    if with_update:
                        r.set_scene_into(coefs=dev.data_ptr(), stream=s.cuda_stream)
                    r.update(cam, stream=s.cuda_stream, timed=False)
            graphs[with_update] = g
        times = {False: [], True: []}
        for rnd in range(args.rounds + 1):
            for with_update in (False, True):
                with torch.cuda.stream(s):
                    e0.record()
                    graphs[with_update].replay()
                    e1.record()
                s.synchronize()
                if rnd:   # (the first round warms up)
                    times[with_update].append(e0.elapsed_time(e1) * 1e3 / args.frames)
        print(f"{name}: captured frame, {args.width}x{args.height}: render only {median(times[False]):7.2f} us, update + render {median(times[True]):7.2f} us "
              f"(+{median(times[True]) - median(times[False]):.2f} us per frame; medians of {args.rounds} graphs of {args.frames} frames, alternating)")
        graphs.clear()
        torch.cuda.synchronize()
        r.cleanup_update()


if __name__ == "__main__":
    main()
