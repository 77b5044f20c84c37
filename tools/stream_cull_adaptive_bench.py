#!/usr/bin/env python3
"""What culling the halo and refine passes changes in a streamed adaptive frame's time (results:
profiles/stream_cull_adaptive.txt).

1920 x 1080, strict, RGBA32F, k = 4, tau = 1/32, flags RT_FLAG_STREAM | RT_FLAG_SSAA4 | RT_FLAG_SSAA_ADAPTIVE | RT_FLAG_STREAM_ADAPTIVE |
RT_FLAG_STREAM_CULL.  Every row compares THIS TREE with A BUILD OF THE PARENT COMMIT under the same flags: there the plain pass is culled
and the refine pass is not.  Two builds of one library cannot share a process, so each build is loaded in a child process started afresh
for the row (this file with --serve); the two children hold one context each and this process asks them in turn, five times, for one
series entry = the median of 31 synchronised rt_render calls by the library's own event pair (`ms`), after 5 warm-up frames.
Rows: the sphere field of tools/stream_bench.py (the field of sections 20 .. 25) at 65, 1 685 and 10 000 spheres, tests/tools/
stream_scenes.field (spheres 2.6 pixels of a 48-row frame across, FIELD_SEED) at the same counts, and 20spheres.
Reported per row: the median of each series' five medians [min .. max], the ratio, the parent's spread (max - min), the refined share,
the decision, whether both builds stored the same frame, and this tree's eight work words of one frame (rt_debug_stream_cull_adaptive;
MI355RT_STREAM_CULL_STATS=1 is set for the children).  Behind the rows, on this tree alone: the plain culled frame and the full
RT_FLAG_SSAA4 culled frame of the 1 685- and 10 000-sphere fields, the frames an adaptive frame is weighed against.

usage: stream_cull_adaptive_bench.py --parent DIR [--out profiles/stream_cull_adaptive.txt]     DIR: a built checkout of the parent commit"""
import argparse
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, K, TAU, WARM, RUNS, ROUNDS = 1920, 1080, 4, 1.0 / 32.0, 5, 31, 5
CASES = [("field", 65), ("field", 1685), ("field", 10000), ("small-sphere field", 65), ("small-sphere field", 1685), ("small-sphere field", 10000), ("20spheres", 0)]


def serve(root, kind, n, mode="adaptive"):
    """A child: one context of the build at `root`; answers "run" with one series entry, "quit" ends it.  mode: "adaptive", or the
    comparison frames "plain" (RT_FLAG_STREAM | RT_FLAG_STREAM_CULL) and "full" (... | RT_FLAG_SSAA4)."""
    import numpy as np
    os.environ["MI355RT_STREAM_CULL_STATS"] = "1"
    for p in (root, os.path.join(root, "tools"), os.path.join(root, "tests", "tools")):
        sys.path.insert(0, p)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    if kind == "field":
        import stream_bench
        sc = stream_bench.field(pkg, n)
    elif kind == "small-sphere field":
        import stream_scenes
        sc = stream_scenes.field(pkg, n, stream_scenes.FIELD_SEED, w=W, h=H)
    else:
        sc = pkg.Scene.load_from_file(os.path.join(root, "scenes", "20spheres.yml")).set_size(W, H)
    flags = pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL
    if mode == "adaptive":
        flags |= pkg.RT_FLAG_SSAA4 | pkg.RT_FLAG_SSAA_ADAPTIVE | pkg.RT_FLAG_STREAM_ADAPTIVE
    elif mode == "full":
        flags |= pkg.RT_FLAG_SSAA4
    r = pkg.Renderer(sc, device=0, flags=flags, **(dict(ssaa_threshold=TAU) if mode == "adaptive" else {}))
    try:
        assert r.streamed and r.streamed_adaptive == (mode == "adaptive")
        decision = bool(getattr(r, "stream_cull_adaptive", False))   # (the parent commit has no such decision)
        for _ in range(WARM):
            r.update()
        words = [0] * 8
        if decision:
            before = r.stream_cull_adaptive_stats()
            r.update()
            words = [b - a for a, b in zip(before, r.stream_cull_adaptive_stats())]
        info = dict(decision=decision, stream_cull=bool(r.stream_cull), refined=int(r.refined) if mode == "adaptive" else 0, words=words,
                    frame=zlib.crc32(r.download().tobytes()))
        print(json.dumps(info), flush=True)
        for line in sys.stdin:
            if line.strip() != "run":
                break
            print(json.dumps(float(np.median([r.update() for _ in range(RUNS)])) * 1e3), flush=True)
    finally:
        r.cleanup_update()


def row(roots, kind, n, mode="adaptive"):
    """(what each child said of its context, one series per child): the children of `roots` asked in turn, ROUNDS times."""
    kids = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", root, kind, str(n), mode], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            for root in roots]
    try:
        info = [json.loads(k.stdout.readline()) for k in kids]
        series = tuple([] for _ in kids)
        for _ in range(ROUNDS):
            for k, s in zip(kids, series):
                k.stdin.write("run\n")
                k.stdin.flush()
                s.append(json.loads(k.stdout.readline()))
        return info, series
    finally:
        for k in kids:
            try:
                k.stdin.write("quit\n")
                k.stdin.close()
            except OSError:
                pass
            k.wait(timeout=60)


def main():
    if len(sys.argv) >= 5 and sys.argv[1] == "--serve":
        return serve(sys.argv[2], sys.argv[3], int(sys.argv[4]), *sys.argv[5:6])
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_cull_adaptive.txt"))
    args = ap.parse_args()
    lines = [f"adaptive frames under RT_FLAG_STREAM | RT_FLAG_SSAA4 | RT_FLAG_SSAA_ADAPTIVE | RT_FLAG_STREAM_ADAPTIVE | RT_FLAG_STREAM_CULL, tau = 1/32, {W}x{H}, strict, "
             f"RGBA32F: a build of the parent commit (refine pass not culled) | this tree; one child process per build and row, the two alternating {ROUNDS} times, one entry "
             f"= the median of {RUNS} synchronised rt_render calls (the library's event pair) after {WARM} warm-up frames; us",
             "per row: median of the five medians [min .. max] for each series, this tree / parent, the parent's spread, the refined share, and this tree's work words of one "
             "frame: primary chunks decided/staged, shadow chunks decided/staged, shadow entries decided/swept, unculled shadow queries, segment-0 queries without a cone"]
    for kind, n in CASES:
        info, (a, b) = row((os.path.abspath(args.parent), ROOT), kind, n)
        ma, mb, spread = float(np.median(a)), float(np.median(b)), max(a) - min(a)
        verdict = "gain beyond the spread" if ma - mb > spread else ("slower beyond the spread" if mb - ma > spread else "within the spread")
        w = info[1]["words"]
        name = kind if kind == "20spheres" else f"{kind} {n}"
        lines.append(f"{name:24s} parent {ma:10.1f} [{min(a):10.1f} .. {max(a):10.1f}]  this tree {mb:10.1f} [{min(b):10.1f} .. {max(b):10.1f}]  x{mb / ma:6.3f}  "
                     f"spread {spread:8.1f}  {verdict}  refined {100.0 * info[1]['refined'] / (W * H):5.2f} %  decision {int(info[1]['decision'])}  "
                     f"same frame {info[0]['frame'] == info[1]['frame'] and info[0]['refined'] == info[1]['refined']}  "
                     f"primary {w[0]}/{w[1]}  shadow chunks {w[2]}/{w[3]}  shadow entries {w[4]}/{w[5]}  unculled {w[6]}  no cone {w[7]}")
        print(lines[-1], flush=True)
    lines.append("this tree alone, the frames an adaptive frame is weighed against (RT_FLAG_STREAM | RT_FLAG_STREAM_CULL, and with RT_FLAG_SSAA4), same protocol:")
    for n in (1685, 10000):
        for mode in ("plain", "full"):
            _, (a,) = row((ROOT,), "field", n, mode)
            lines.append(f"field {n:<6d} {mode:5s} {float(np.median(a)):10.1f} [{min(a):10.1f} .. {max(a):10.1f}]")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
