#!/usr/bin/env python3
"""What RT_FLAG_STREAM_CULL_PIXELS changes in the time of the streamed pixel queries (results:
profiles/stream_cull_pixels.txt, whose last part is the table of that section).  The method is section 29's.

1920 x 1080, strict.  Scenes: the sphere field of tests/tools/stream_scenes.py at 65, 1 685 and 10 000 spheres.  Calls: rt_render_gbuffer
with all three planes, rt_object_extents over the whole frame, rt_pick of 1 and of 4 096 pixels (a fixed draw of unrelated pixels).  Each
row is timed with RT_FLAG_STREAM | RT_FLAG_STREAM_QUERIES | RT_FLAG_STREAM_CULL without and with RT_FLAG_STREAM_CULL_PIXELS, alternating
five times in one process (two contexts, created once, neither with work words); one series entry = the median of 31 synchronised calls
after 5 warm-up calls -- by the library's own event pair for the planes and the extents, by the host's clock around the blocking call for
rt_pick, which has no timer (upload, kernel, download, wait).  Reported: the median of each series' five medians with [min .. max], the
spread (max - min) of the unflagged series, whether the outputs are equal bit for bit, the work words of one flagged call
(rt_debug_stream_cull_pixels, from a third context created with MI355RT_STREAM_CULL_STATS=1) with the staged fraction [1] / [0] and the
swept fraction [3] / [2], and for scale the culled frame kernel's time on the same scene (rt_render of the unflagged context).  A
difference counts only beyond the unflagged series' spread.

usage: stream_cull_pixels_bench.py [--out profiles/stream_cull_pixels.txt] [--counts 65,1685,10000] [--rounds 5] [--runs 31]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as graft  # noqa: E402
import stream_scenes as S  # noqa: E402

W, H, WARM = 1920, 1080, 5
SEED = 3
CALLS = ("rt_render_gbuffer", "rt_object_extents", "rt_pick, 1 pixel", "rt_pick, 4096 pixels")


class Buffers:
    """Every output on the device and the picked pixels, once per scene."""

    def __init__(self, r, n_obj):
        import torch
        self.po = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
        self.pt = torch.zeros((H, W), dtype=torch.float64, device="cuda:0")
        self.pn = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        self.ext = torch.zeros((n_obj * 5,), dtype=torch.int64, device="cuda:0")
        rng = np.random.default_rng(29)
        self.xy = np.stack([rng.integers(0, W, 4096), rng.integers(0, H, 4096)], axis=1)
        self.rec = None
        torch.cuda.synchronize()

    def call(self, r, what):
        """One synchronised call; its time in us."""
        if what == "rt_render_gbuffer":
            return r.gbuffer_into(None, self.po.data_ptr(), self.pt.data_ptr(), self.pn.data_ptr()) * 1e3
        if what == "rt_object_extents":
            return r.object_extents_into(None, None, self.ext.data_ptr()) * 1e3
        xy = self.xy[:1] if what == "rt_pick, 1 pixel" else self.xy
        t0 = time.perf_counter()
        self.rec = r.pick(xy)
        return (time.perf_counter() - t0) * 1e6

    def output(self, what):
        import torch
        torch.cuda.synchronize()
        if what == "rt_render_gbuffer":
            return [o.cpu().numpy().tobytes() for o in (self.po, self.pt, self.pn)]
        if what == "rt_object_extents":
            return [self.ext.cpu().numpy().tobytes()]
        return [self.rec.tobytes()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_cull_pixels.txt"))
    ap.add_argument("--counts", default="65,1685,10000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=31)
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    base = pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_QUERIES | pkg.RT_FLAG_STREAM_CULL
    lines = [f"RT_FLAG_STREAM | RT_FLAG_STREAM_QUERIES | RT_FLAG_STREAM_CULL without | with RT_FLAG_STREAM_CULL_PIXELS, {W}x{H}, strict; stream_scenes.field(seed {SEED}); "
             f"two contexts alternating {args.rounds} times, one entry = the median of {args.runs} synchronised calls after {WARM} warm-up calls (the library's event pair; "
             f"rt_pick: the host's clock around the blocking call); us; {torch.cuda.get_device_name(0)}",
             "per row: median of the medians [min .. max] for each series, flagged / unflagged, the unflagged series' spread, the verdict, and the work words of one "
             "flagged call: chunk decisions/staged, entries asked in staged chunks/swept"]
    table = ["| spheres | call | unflagged us [min .. max] | flagged us [min .. max] | ratio | spread us | verdict | staged [1]/[0] | swept [3]/[2] |",
             "|---|---|---|---|---|---|---|---|---|"]

    def emit(text):
        lines.append(text)
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:      # (rewritten row by row: a run that is cut short leaves what it measured)
            fh.write("\n".join(lines + ["", "the table of DESIGN.md section 34:"] + table) + "\n")

    for n in [int(x) for x in args.counts.split(",")]:
        sc = S.field(pkg, n, SEED, w=W, h=H)
        os.environ.pop("MI355RT_STREAM_CULL_STATS", None)
        plain, cull = pkg.Renderer(sc, device=0, flags=base), pkg.Renderer(sc, device=0, flags=base | pkg.RT_FLAG_STREAM_CULL_PIXELS)
        os.environ["MI355RT_STREAM_CULL_STATS"] = "1"
        counted = pkg.Renderer(sc, device=0, flags=base | pkg.RT_FLAG_STREAM_CULL_PIXELS)
        try:
            assert plain.stream_cull and plain.streamed_queries and not plain.stream_cull_pixels and cull.stream_cull_pixels and counted.stream_cull_pixels
            buf = Buffers(plain, n)
            for _ in range(WARM):
                plain.update()
            frame = float(np.median([plain.update() for _ in range(args.runs)])) * 1e3
            emit(f"field {n:6d} culled frame kernel (rt_render of the unflagged context), for scale: {frame:10.1f}")
            for what in CALLS:
                for r in (plain, cull):
                    for _ in range(WARM):
                        buf.call(r, what)
                a, b = [], []
                for _ in range(args.rounds):
                    a.append(float(np.median([buf.call(plain, what) for _ in range(args.runs)])))
                    b.append(float(np.median([buf.call(cull, what) for _ in range(args.runs)])))
                out_cull = buf.output(what)
                buf.call(plain, what)
                same = out_cull == buf.output(what)
                before = counted.stream_cull_pixels_stats()
                buf.call(counted, what)
                w = [y - x for x, y in zip(before, counted.stream_cull_pixels_stats())]
                ma, mb, spread = float(np.median(a)), float(np.median(b)), max(a) - min(a)
                verdict = "gain" if ma - mb > spread else ("overhead" if mb - ma > spread else "within the spread")
                staged = w[1] / w[0] if w[0] else float("nan")
                swept = w[3] / w[2] if w[2] else float("nan")
                emit(f"field {n:6d} {what:22s} unflagged {ma:10.1f} [{min(a):10.1f} .. {max(a):10.1f}]  flagged {mb:10.1f} [{min(b):10.1f} .. {max(b):10.1f}]  "
                     f"x{mb / ma:6.3f}  spread {spread:8.1f}  {verdict:17s}  same outputs {same}  chunks {w[0]}/{w[1]} (staged {staged:.3f})  entries {w[2]}/{w[3]} "
                     f"(swept {swept:.3f})")
                table.append(f"| {n} | `{what}` | {ma:.1f} [{min(a):.1f} .. {max(a):.1f}] | {mb:.1f} [{min(b):.1f} .. {max(b):.1f}] | {mb / ma:.3f} | {spread:.1f} | {verdict} | "
                             f"{staged:.3f} | {swept:.3f} |")
            emit(f"field {n:6d} done")
        finally:
            for r in (plain, cull, counted):
                r.cleanup_update()
            del buf
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
