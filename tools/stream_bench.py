#!/usr/bin/env python3
"""What the streamed frame kernel costs (results: profiles/stream.txt).

Synchronised rt_render calls timed by the library's own event pair, median of 31 after 5 warm-up frames; 1920 x 1080, strict, RGBA32F.
  (a) 20spheres and reflection_test: default, RT_FLAG_SIMPLE and RT_FLAG_STREAM side by side;
  (b) a sphere field (tests/tools/extents_ref.py: sphere_field, with a point light more) with the largest sphere count the default kernel
      accepts: default against streamed, and streamed with RT_FLAG_NOCULL;
  (c) the first count beyond the limit and 10 000 spheres: streamed alone, next to the CPU oracle's time for the same frame with all
      host threads.

usage: stream_bench.py [--out profiles/stream.txt] [--threads N] [--no-cpu]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as graft  # noqa: E402
import extents_ref  # noqa: E402
import stream_scenes  # noqa: E402

W, H, WARM, RUNS = 1920, 1080, 5, 31


def field(pkg, n):
    sc = extents_ref.sphere_field(pkg, n, 3, w=W, h=H)
    sc.add_light("spherical", [3.0, 8.0, 5.0], (1.0, 0.9, 0.8), 400.0)
    return sc


def largest_default_count(pkg):
    """By the launcher's own rule (rt_wavefront_lds_bytes_strict on the words of a field of n culled spheres, two lights)."""
    return stream_scenes.first_count_beyond_lds(pkg, n_lights=2) - 1


def timed(pkg, sc, flags):
    r = pkg.Renderer(sc, device=0, flags=flags)
    try:
        for _ in range(WARM):
            r.update()
        ms = [r.update() for _ in range(RUNS)]
        return float(np.median(ms)) * 1e3, float(min(ms)) * 1e3, r.streamed
    finally:
        r.cleanup_update()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream.txt"))
    ap.add_argument("--threads", type=int, default=min(os.cpu_count() or 1, 16))
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    lines = [f"streamed frame kernel, {W}x{H}, strict, RGBA32F; synchronised rt_render calls, the library's event pair, median of {RUNS} after {WARM} "
             f"warm-up frames (us; min in brackets); {torch.cuda.get_device_name(0)}"]

    def row(what, sc, variants):
        cells = []
        for label, flags in variants:
            med, lo, streamed = timed(pkg, sc, flags)
            cells.append((label, med, lo, streamed))
        base = cells[0][1]
        text = "  ".join(f"{label} {med:10.1f} [{lo:10.1f}]{' (streamed)' if st else ''} x{med / base:6.2f}" for label, med, lo, st in cells)
        lines.append(f"{what:28s} {text}")
        print(lines[-1], flush=True)

    lines.append("(a) shipped scenes: default | RT_FLAG_SIMPLE | RT_FLAG_STREAM")
    for name in ("20spheres", "reflection_test"):
        sc = pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", name + ".yml")).set_size(W, H)
        row(name, sc, (("default", 0), ("simple", pkg.RT_FLAG_SIMPLE), ("stream", pkg.RT_FLAG_STREAM)))
    n = largest_default_count(pkg)
    lines.append(f"(b) sphere field, {n} spheres (the most the default kernel accepts), two lights: default | RT_FLAG_STREAM | RT_FLAG_STREAM + RT_FLAG_NOCULL")
    row(f"field {n}", field(pkg, n), (("default", 0), ("stream", pkg.RT_FLAG_STREAM), ("stream nocull", pkg.RT_FLAG_STREAM | pkg.RT_FLAG_NOCULL)))
    lines.append(f"(c) beyond the limit: flags = 0 (streamed) | the CPU oracle with {args.threads} threads")
    for m in (n + 1, 10000):
        sc = field(pkg, m)
        med, lo, streamed = timed(pkg, sc, 0)
        assert streamed
        text = f"field {m:<22d} stream {med:10.1f} [{lo:10.1f}]"
        if not args.no_cpu:
            osc = stream_scenes.oracle_of(pkg, sc)
            t0 = time.perf_counter()
            osc.render(nthreads=args.threads)
            cpu = (time.perf_counter() - t0) * 1e6
            text += f"  cpu oracle {cpu:12.1f}  x{cpu / med:8.1f}"
        lines.append(text)
        print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
