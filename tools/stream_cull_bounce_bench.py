#!/usr/bin/env python3
"""What RT_FLAG_STREAM_CULL_BOUNCE changes in the culled streamed frame kernel's time (results:
profiles/stream_cull_bounce.txt).

1920 x 1080, strict, RGBA32F.  Cases: the mirrored sphere field of tests/tools/stream_scenes.py (every third sphere reflects,
max_reflections = 2) at 65, 1 685 and 10 000 spheres.  Each case is timed with RT_FLAG_STREAM | RT_FLAG_STREAM_CULL without and with
RT_FLAG_STREAM_CULL_BOUNCE, alternating five times in one process (two contexts, created once); one series entry = the median of 31
synchronised rt_render calls by the library's own event pair, after 5 warm-up frames.  Reported: the median of each series' five
medians with [min .. max], the spread (max - min) of the unflagged series, whether the two frames are equal bit for bit, and the flagged
context's bounce work words per frame (rt_debug_stream_cull_bounce; MI355RT_STREAM_CULL_STATS=1 is set here) with the staged fraction
[1] / [0] and the per-lane fraction [3] / [2].  A difference counts as a gain only beyond the unflagged series' spread.

usage: stream_cull_bounce_bench.py [--out profiles/stream_cull_bounce.txt] [--px 2.6] [--counts 65,1685,10000]"""
import argparse
import os
import sys

import numpy as np

os.environ["MI355RT_STREAM_CULL_STATS"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as graft  # noqa: E402
import stream_scenes as S  # noqa: E402

W, H, WARM, RUNS, ROUNDS = 1920, 1080, 5, 31, 5
SEED = 3


def series(pkg, sc):
    """(five medians without the flag, five with it, bounce work words of one flagged frame, the decision, frames equal), in us."""
    base = pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL
    plain = pkg.Renderer(sc, device=0, flags=base)
    bounce = pkg.Renderer(sc, device=0, flags=base | pkg.RT_FLAG_STREAM_CULL_BOUNCE)
    try:
        assert plain.stream_cull and bounce.stream_cull and not plain.stream_cull_bounce
        on = bounce.stream_cull_bounce
        for r in (plain, bounce):
            for _ in range(WARM):
                r.update()
        before = bounce.stream_cull_bounce_stats() if on else [0] * 8
        bounce.update()
        words = [b - a for a, b in zip(before, bounce.stream_cull_bounce_stats())] if on else [0] * 8
        a, b = [], []
        for _ in range(ROUNDS):
            a.append(float(np.median([plain.update() for _ in range(RUNS)])) * 1e3)
            b.append(float(np.median([bounce.update() for _ in range(RUNS)])) * 1e3)
        same = bool(np.array_equal(plain.download().view(np.uint32), bounce.download().view(np.uint32)))
        return a, b, words, on, same
    finally:
        plain.cleanup_update()
        bounce.cleanup_update()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_cull_bounce.txt"))
    ap.add_argument("--px", type=float, default=2.6, help="pixels across a sphere (stream_scenes.field)")
    ap.add_argument("--counts", default="65,1685,10000")
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    lines = [f"RT_FLAG_STREAM | RT_FLAG_STREAM_CULL without | with RT_FLAG_STREAM_CULL_BOUNCE, {W}x{H}, strict, RGBA32F; stream_scenes.field(mirrors=True, depth=2, "
             f"px={args.px:g}, seed {SEED}); two contexts alternating {ROUNDS} times, one entry = the median of {RUNS} synchronised rt_render calls (the library's event "
             f"pair) after {WARM} warm-up frames; us; {torch.cuda.get_device_name(0)}",
             "per case: median of the five medians [min .. max] for each series, flagged / unflagged, the unflagged series' spread, and the flagged context's bounce "
             "work words of one frame: chunk decisions/staged, (lane, chunk) pairs asked/reaching, queries without a lane to cull for"]
    for n in [int(x) for x in args.counts.split(",")]:
        sc = S.field(pkg, n, SEED, w=W, h=H, mirrors=True, depth=2, px=args.px)
        a, b, w, on, same = series(pkg, sc)
        ma, mb, spread = float(np.median(a)), float(np.median(b)), max(a) - min(a)
        verdict = "gain beyond the spread" if ma - mb > spread else ("overhead beyond the spread" if mb - ma > spread else "within the spread")
        staged = w[1] / w[0] if w[0] else float("nan")
        lanes = w[3] / w[2] if w[2] else float("nan")
        lines.append(f"field {n:6d}   cull {ma:10.1f} [{min(a):10.1f} .. {max(a):10.1f}]  cull+bounce {mb:10.1f} [{min(b):10.1f} .. {max(b):10.1f}]  x{mb / ma:6.3f}  "
                     f"spread {spread:8.1f}  {verdict}  decision {int(on)}  same frame {same}  "
                     f"chunks {w[0]}/{w[1]} (staged {staged:.3f})  pairs {w[2]}/{w[3]} (reach {lanes:.3f})  uncullable queries {w[4]}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
