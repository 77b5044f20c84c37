#!/usr/bin/env python3
"""What RT_FLAG_STREAM_CULL changes in the streamed frame kernel's time (results: profiles/stream_cull.txt).

1920 x 1080, strict, RGBA32F.  Cases: 20spheres, and the sphere field of tools/stream_bench.py at the largest count the default kernel
accepts, the first count beyond it, and 10 000 spheres.  Each case is timed with RT_FLAG_STREAM without and with RT_FLAG_STREAM_CULL,
alternating five times in one process (two contexts, created once); one series entry = the median of 31 synchronised rt_render calls by
the library's own event pair, after 5 warm-up frames.  Reported: the median of each series' five medians, the spread (max - min) of the
unflagged series, and the flagged context's work words per frame (rt_debug_stream_cull; MI355RT_STREAM_CULL_STATS=1 is set here).

usage: stream_cull_bench.py [--out profiles/stream_cull.txt]"""
import argparse
import os
import sys

import numpy as np

os.environ["MI355RT_STREAM_CULL_STATS"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as graft  # noqa: E402
import stream_bench  # noqa: E402

W, H, WARM, RUNS, ROUNDS = stream_bench.W, stream_bench.H, 5, 31, 5


def series(pkg, sc):
    """(five medians without the flag, five with it, work words of one flagged frame), in us."""
    plain = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_STREAM)
    cull = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL)
    try:
        assert plain.streamed and cull.streamed and not plain.stream_cull
        on = cull.stream_cull
        for r in (plain, cull):
            for _ in range(WARM):
                r.update()
        before = cull.stream_cull_stats() if on else [0] * 8
        cull.update()
        words = [b - a for a, b in zip(before, cull.stream_cull_stats())] if on else [0] * 8
        a, b = [], []
        for _ in range(ROUNDS):
            a.append(float(np.median([plain.update() for _ in range(RUNS)])) * 1e3)
            b.append(float(np.median([cull.update() for _ in range(RUNS)])) * 1e3)
        same = bool(np.array_equal(plain.download().view(np.uint32), cull.download().view(np.uint32)))
        return a, b, words, on, same
    finally:
        plain.cleanup_update()
        cull.cleanup_update()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_cull.txt"))
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    n = stream_bench.largest_default_count(pkg)
    lines = [f"RT_FLAG_STREAM without | with RT_FLAG_STREAM_CULL, {W}x{H}, strict, RGBA32F; two contexts alternating {ROUNDS} times, one entry = the median of {RUNS} "
             f"synchronised rt_render calls (the library's event pair) after {WARM} warm-up frames; us; {torch.cuda.get_device_name(0)}",
             "per case: median of the five medians [min .. max] for each series, flagged / unflagged, the unflagged series' spread, and the flagged context's work "
             "words of one frame: primary chunks decided/staged, shadow chunks decided/staged, shadow entries decided/swept, unculled shadow queries"]
    cases = [("20spheres", pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", "20spheres.yml")).set_size(W, H))]
    cases += [(f"field {m}", stream_bench.field(pkg, m)) for m in (n, n + 1, 10000)]
    for name, sc in cases:
        a, b, w, on, same = series(pkg, sc)
        ma, mb, spread = float(np.median(a)), float(np.median(b)), max(a) - min(a)
        verdict = "gain beyond the spread" if ma - mb > spread else ("overhead beyond the spread" if mb - ma > spread else "within the spread")
        lines.append(f"{name:14s} stream {ma:10.1f} [{min(a):10.1f} .. {max(a):10.1f}]  stream+cull {mb:10.1f} [{min(b):10.1f} .. {max(b):10.1f}]  x{mb / ma:6.3f}  "
                     f"spread {spread:8.1f}  {verdict}  decision {int(on)}  same frame {same}  "
                     f"primary {w[0]}/{w[1]}  shadow chunks {w[2]}/{w[3]}  shadow entries {w[4]}/{w[5]}  unculled {w[6]}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
