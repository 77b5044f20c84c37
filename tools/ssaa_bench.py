"""Cost of supersampling (RT_FLAG_SSAA2 / RT_FLAG_SSAA4): frame time for k = 1, 2, 4 and the resolve kernel's own time.

  python tools/ssaa_bench.py [--frames N] [--warmup W]
      device ms per frame as Renderer.update times them (hipEvent pair around render + resolve; median of N after W warm-up frames)
      for 20spheres at 1080p and 4K and clebsch at 1080p, RGBA32F, start pose
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ssaa -- python tools/ssaa_bench.py --trace-run
      the same configurations with k = 2 and 4, resolve with plain and with non-temporal loads (MI355RT_RESOLVE_NT), TRACE_FRAMES each
  python tools/ssaa_bench.py --summarize DIR
      the resolve dispatches of that trace in launch order, TRACE_FRAMES per configuration: median kernel time and effective bytes/s
      (bytes = k^2 * W * H * 16 read + W * H * 16 written, the least the resolve must move)
"""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("20spheres", 1920, 1080), ("20spheres", 3840, 2160), ("clebsch", 1920, 1080)]
TRACE_FRAMES = 20


def renderer(pkg, name, w, h, k):
    flags = {1: 0, 2: pkg.RT_FLAG_SSAA2, 4: pkg.RT_FLAG_SSAA4}[k]
    sc = pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", name + ".yml")).set_size(w, h)
    return pkg.Renderer(sc, device=0, flags=flags)


def timing(pkg, frames, warmup):
    print(f"frame time, device ms (Renderer.update: render + resolve), median of {frames} after {warmup} warm-up frames, RGBA32F, start pose")
    print(f"{'scene':<10} {'size':>10} {'k=1':>9} {'k=2':>9} {'k=4':>9}   k=2/k=1  k=4/k=1")
    for name, w, h in CONFIGS:
        ms = {}
        for k in (1, 2, 4):
            r = renderer(pkg, name, w, h, k)
            for _ in range(warmup):
                r.update()
            ms[k] = float(np.median([r.update() for _ in range(frames)]))
            r.cleanup_update()
        print(f"{name:<10} {w:>5}x{h:<4} {ms[1]:9.4f} {ms[2]:9.4f} {ms[4]:9.4f}   {ms[2] / ms[1]:7.2f}  {ms[4] / ms[1]:7.2f}")


def trace_cases():
    return [(name, w, h, k, nt) for name, w, h in CONFIGS for k in (2, 4) for nt in (0, 1)]


def trace_run(pkg):
    for name, w, h, k, nt in trace_cases():
        os.environ["MI355RT_RESOLVE_NT"] = str(nt)   # (read when the context is created)
        r = renderer(pkg, name, w, h, k)
        for _ in range(TRACE_FRAMES):
            r.update()
        r.cleanup_update()


def summarize(d):
    paths = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    if not paths:
        sys.exit(f"no *kernel_trace.csv under {d}")
    rows = []
    for p in paths:
        with open(p) as fh:
            rows += [r for r in csv.DictReader(fh) if "resolve_kernel" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cases = trace_cases()
    if len(rows) != TRACE_FRAMES * len(cases):
        sys.exit(f"{len(rows)} resolve dispatches in the trace, expected {TRACE_FRAMES * len(cases)}")
    print(f"resolve kernel (rocprofv3 --kernel-trace), median of {TRACE_FRAMES} dispatches per configuration; bytes = k^2*W*H*16 in + W*H*16 out")
    print(f"{'scene':<10} {'size':>10} {'k':>2} {'loads':>6} {'us':>9} {'MB':>8} {'TB/s':>7}")
    for i, (name, w, h, k, nt) in enumerate(cases):
        chunk = rows[i * TRACE_FRAMES:(i + 1) * TRACE_FRAMES]
        assert all(f"<{k}," in r["Kernel_Name"] or f"ILi{k}E" in r["Kernel_Name"] for r in chunk), (name, k, chunk[0]["Kernel_Name"])
        us = float(np.median([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0 for r in chunk]))
        nbytes = (k * k + 1) * w * h * 16
        print(f"{name:<10} {w:>5}x{h:<4} {k:>2} {'nt' if nt else 'plain':>6} {us:9.2f} {nbytes / 1e6:8.1f} {nbytes / us / 1e6:7.2f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
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
