#!/usr/bin/env python3
"""What the streamed adaptive passes cost (results: profiles/stream_adaptive.txt).

Synchronised rt_render calls timed by the library's own event pair, median of 21 after 3 warm-up calls, the contexts of a row alternating
call by call in one process; 1920 x 1080, strict, RGBA32F, k = 4, tau = 1/32; the sphere fields of tools/stream_bench.py.
  (a) 568 spheres, the most the staged passes accept: the staged adaptive context against the forced-streamed one
      (RT_FLAG_STREAM | RT_FLAG_STREAM_ADAPTIVE) and against the flag alone (decision false: the staged passes again); the two plain
      frames (default, RT_FLAG_STREAM) stand next to them, so that the plain pass can be told from the refine pass;
  (b) the first count beyond the wavefront kernel's limit and 10 000 spheres: the streamed adaptive frame (RT_FLAG_STREAM_ADAPTIVE, nothing
      forced) against the RT_FLAG_STREAM | RT_FLAG_SSAA4 frame and the plain streamed frame, with the refined share of the frame.

usage: stream_adaptive_bench.py [--out profiles/stream_adaptive.txt] [--small]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as graft  # noqa: E402
import stream_bench  # noqa: E402

WARM, RUNS, K, TAU = 3, 21, 4, 1.0 / 32.0


def alternating(pkg, sc, variants):
    """[(label, median us, min us, refined share or None, streamed, streamed_adaptive)]: one context per variant, all alive, called in turn."""
    ctxs = []
    try:
        for label, flags in variants:
            kw = dict(ssaa_threshold=TAU) if flags & pkg.RT_FLAG_SSAA_ADAPTIVE else {}
            ctxs.append((label, flags, pkg.Renderer(sc, device=0, flags=flags, **kw)))
        for _ in range(WARM):
            for _, _, r in ctxs:
                r.update()
        ms = [[] for _ in ctxs]
        for _ in range(RUNS):
            for i, (_, _, r) in enumerate(ctxs):
                ms[i].append(r.update())
        out = []
        for i, (label, flags, r) in enumerate(ctxs):
            share = r.refined / float(r.width * r.local_rows) if flags & pkg.RT_FLAG_SSAA_ADAPTIVE else None
            out.append((label, float(np.median(ms[i])) * 1e3, float(min(ms[i])) * 1e3, share, r.streamed, r.streamed_adaptive))
        return out
    finally:
        for _, _, r in ctxs:
            r.cleanup_update()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_adaptive.txt"))
    ap.add_argument("--small", action="store_true", help="320 x 180 and 2 000 instead of 10 000 spheres: a check of the tool, not a measurement")
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    if args.small:
        stream_bench.W, stream_bench.H = 320, 180
    ada = pkg.RT_FLAG_SSAA4 | pkg.RT_FLAG_SSAA_ADAPTIVE
    lines = [f"streamed adaptive supersampling, {stream_bench.W}x{stream_bench.H}, strict, RGBA32F, k = {K}, tau = 1/32; synchronised rt_render calls, the library's "
             f"event pair, median of {RUNS} after {WARM} warm-up calls, the contexts of a row alternating (us; min in brackets; x = against the row's first); "
             f"{torch.cuda.get_device_name(0)}"]

    def row(what, sc, variants):
        cells = alternating(pkg, sc, variants)
        base = cells[0][1]
        lines.append(what)
        for label, med, lo, share, streamed, sa in cells:
            kind = ("streamed plain pass" if streamed else "staged plain pass") + (", streamed adaptive passes" if sa else "")
            lines.append(f"    {label:38s} {med:12.1f} [{lo:12.1f}] x{med / base:7.3f}" + (f"  refined {100.0 * share:5.1f} %" if share is not None else "") + f"  ({kind})")
        print("\n".join(lines[-len(cells) - 1:]), flush=True)

    n = 568
    row(f"(a) sphere field, {n} spheres (the most the staged adaptive passes accept)", stream_bench.field(pkg, n),
        (("adaptive, staged", ada), ("adaptive, forced streamed", ada | pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_ADAPTIVE),
         ("adaptive, RT_FLAG_STREAM_ADAPTIVE only", ada | pkg.RT_FLAG_STREAM_ADAPTIVE), ("plain, default", 0), ("plain, RT_FLAG_STREAM", pkg.RT_FLAG_STREAM)))
    first = stream_bench.largest_default_count(pkg) + 1
    for m in (first, 2000 if args.small else 10000):
        row(f"(b) sphere field, {m} spheres (beyond the wavefront kernel's limit)", stream_bench.field(pkg, m),
            (("adaptive, RT_FLAG_STREAM_ADAPTIVE", ada | pkg.RT_FLAG_STREAM_ADAPTIVE), ("RT_FLAG_STREAM | RT_FLAG_SSAA4", pkg.RT_FLAG_STREAM | pkg.RT_FLAG_SSAA4),
             ("plain, streamed", 0)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
