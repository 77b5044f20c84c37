"""Cost of edge-adaptive supersampling (RT_FLAG_SSAA_ADAPTIVE) against full supersampling (RT_FLAG_SSAA2 / RT_FLAG_SSAA4).

  python tools/ssaa_adaptive_bench.py [--frames N] [--warmup W]
      device ms per frame as Renderer.update times them (median of N after W warm-up frames), RGBA32F, start pose, for 20spheres and
      clebsch at 1080p and 4K, k = 2 and 4: full supersampling and adaptive at three thresholds, all contexts of one configuration
      alive in the same process and their frames alternated; the refined fraction of each adaptive row
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ada -- python tools/ssaa_adaptive_bench.py --trace-run
      the adaptive configurations at the default threshold, TRACE_FRAMES each
  python tools/ssaa_adaptive_bench.py --summarize DIR
      that trace's dispatches split into plain pass, classify and refine (median per frame)
"""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("20spheres", 1920, 1080), ("20spheres", 3840, 2160), ("clebsch", 1920, 1080), ("clebsch", 3840, 2160)]
TAUS = [1.0 / 32.0, 1.0 / 128.0, 1.0 / 8.0]   # the default first
TRACE_FRAMES = 20


def renderer(pkg, name, w, h, k, tau=None):
    flags = {2: pkg.RT_FLAG_SSAA2, 4: pkg.RT_FLAG_SSAA4}[k] | (pkg.RT_FLAG_SSAA_ADAPTIVE if tau is not None else 0)
    sc = pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", name + ".yml")).set_size(w, h)
    return pkg.Renderer(sc, device=0, flags=flags, ssaa_threshold=tau)


def timing(pkg, frames, warmup):
    print(f"frame time, device ms (Renderer.update), median of {frames} after {warmup} warm-up frames, RGBA32F, start pose; "
          f"full and adaptive contexts alternated frame by frame")
    head = "".join(f"  tau=1/{round(1 / t):<4} {'refined':>8}" for t in TAUS)
    print(f"{'scene':<10} {'size':>10} {'k':>2} {'full':>9}{head}   full/adaptive(default)")
    for name, w, h in CONFIGS:
        for k in (2, 4):
            rs = [renderer(pkg, name, w, h, k)] + [renderer(pkg, name, w, h, k, t) for t in TAUS]
            for _ in range(warmup):
                for r in rs:
                    r.update()
            ms = [[] for _ in rs]
            for _ in range(frames):
                for i, r in enumerate(rs):
                    ms[i].append(r.update())
            med = [float(np.median(m)) for m in ms]
            frac = [r.refined / (w * h) for r in rs[1:]]
            cells = "".join(f"  {m:11.4f} {100 * f:7.2f}%" for m, f in zip(med[1:], frac))
            print(f"{name:<10} {w:>5}x{h:<4} {k:>2} {med[0]:9.4f}{cells}   {med[0] / med[1]:6.2f}x")
            for r in rs:
                r.cleanup_update()


def trace_cases():
    return [(name, w, h, k) for name, w, h in CONFIGS for k in (2, 4)]


def trace_run(pkg):
    for name, w, h, k in trace_cases():
        r = renderer(pkg, name, w, h, k, TAUS[0])
        for _ in range(TRACE_FRAMES):
            r.update()
        r.cleanup_update()


def phase(kernel):
    if "classify_kernel" in kernel:
        return "classify"
    if "ray_list_kernel" in kernel:
        return "refine"
    if "wavefront" in kernel or "trace_tile_kernel" in kernel:
        return "plain"
    return None


def summarize(d):
    paths = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    if not paths:
        sys.exit(f"no *kernel_trace.csv under {d}")
    rows = []
    for p in paths:
        with open(p) as fh:
            rows += [r for r in csv.DictReader(fh) if phase(r.get("Kernel_Name", ""))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # one frame = plain (one dispatch of the wavefront kernel), classify, refine
    frames, cur = [], {}
    for r in rows:
        ph = phase(r["Kernel_Name"])
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
        cur[ph] = cur.get(ph, 0.0) + us
        if ph == "refine":
            frames.append(cur)
            cur = {}
    cases = trace_cases()
    if len(frames) != TRACE_FRAMES * len(cases):
        sys.exit(f"{len(frames)} frames in the trace, expected {TRACE_FRAMES * len(cases)}")
    print(f"adaptive frames at tau = 1/32 (rocprofv3 --kernel-trace), median kernel time per frame over {TRACE_FRAMES} frames, us")
    print(f"{'scene':<10} {'size':>10} {'k':>2} {'plain':>9} {'classify':>9} {'refine':>9} {'sum':>9}")
    for i, (name, w, h, k) in enumerate(cases):
        chunk = frames[i * TRACE_FRAMES:(i + 1) * TRACE_FRAMES]
        med = {ph: float(np.median([f.get(ph, 0.0) for f in chunk])) for ph in ("plain", "classify", "refine")}
        print(f"{name:<10} {w:>5}x{h:<4} {k:>2} {med['plain']:9.2f} {med['classify']:9.2f} {med['refine']:9.2f} {sum(med.values()):9.2f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--summarize", metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
        return
    import __graft_entry__ as graft
    pkg = graft.load_package()
    if a.trace_run:
        trace_run(pkg)
    else:
        timing(pkg, a.frames, a.warmup)


if __name__ == "__main__":
    main()
