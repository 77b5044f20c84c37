#!/usr/bin/env python3
"""What RT_FLAG_STREAM_CULL_RAYS changes in the time of the streamed ray queries (results:
profiles/stream_cull_rays.txt, whose last part is the table of that section).

1920 x 1080 rays, strict.  Scenes: the sphere field of tests/tools/stream_scenes.py at 65, 1 685 and 10 000 spheres, plain and with
mirrors (every third sphere reflects, max_reflections = 2).  Rays: the context's own primary rays (rt_primary_rays), in row order and
shuffled (a fixed permutation); a wave is 64 consecutive rays.  Entry points: rt_trace_rays, rt_occluded_rays (NULL t_max),
rt_shade_rays, rt_trace_paths.  Each row is timed with RT_FLAG_STREAM | RT_FLAG_STREAM_QUERIES | RT_FLAG_STREAM_CULL without and with
RT_FLAG_STREAM_CULL_RAYS, alternating five times in one process (two contexts, created once, neither with work words); one series entry =
the median of 31 synchronised calls by the library's own event pair, after 5 warm-up calls.  Reported: the median of each series' five
medians with [min .. max], the spread (max - min) of the unflagged series, whether the outputs are equal bit for bit, the work words of
one flagged call (rt_debug_stream_cull_rays, from a third context created with MI355RT_STREAM_CULL_STATS=1) with the staged fraction
[1] / [0] and the per-lane fraction [3] / [2], and for scale the culled frame kernel's time on the same scene (rt_render of the
unflagged context).  A difference counts only beyond the unflagged series' spread.

usage: stream_cull_rays_bench.py [--out profiles/stream_cull_rays.txt] [--counts 65,1685,10000] [--rounds 5] [--runs 31]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as graft  # noqa: E402
import stream_scenes as S  # noqa: E402

W, H, WARM = 1920, 1080, 5
SEED = 3
ENTRY_POINTS = ("rt_trace_rays", "rt_occluded_rays", "rt_shade_rays", "rt_trace_paths")


class Buffers:
    """The rays in both orders and every output, on the device, once per scene."""

    def __init__(self, r):
        import torch
        self.n = W * H
        rays, _ = r.primary_rays()
        gen = torch.Generator(device="cpu").manual_seed(29)
        self.rays = {"row": rays.reshape(-1, 6).contiguous(), "shuffled": rays.reshape(-1, 6)[torch.randperm(self.n, generator=gen).to(rays.device)].contiguous()}
        self.m = r._max_segments(None)
        self.hits = torch.zeros((self.n, 6), dtype=torch.float64, device=rays.device)
        self.blocked = torch.zeros((self.n,), dtype=torch.int32, device=rays.device)
        self.rgba = torch.zeros((self.n, 4), dtype=torch.float32, device=rays.device)
        self.seg = torch.zeros((self.m * self.n, 6), dtype=torch.float64, device=rays.device)
        self.ends = torch.zeros((self.n, 4), dtype=torch.int32, device=rays.device)
        torch.cuda.synchronize()

    def call(self, r, entry, order):
        """One synchronised call; the library's own time in us."""
        p = self.rays[order].data_ptr()
        if entry == "rt_trace_rays":
            return r.trace_into(p, self.n, self.hits.data_ptr()) * 1e3
        if entry == "rt_occluded_rays":
            return r.occluded_into(p, None, self.n, self.blocked.data_ptr()) * 1e3
        if entry == "rt_shade_rays":
            return r.shade_into(p, self.n, self.rgba.data_ptr()) * 1e3
        return r.paths_into(p, self.n, self.m, self.seg.data_ptr(), None, self.ends.data_ptr()) * 1e3

    def output(self, entry):
        import torch
        torch.cuda.synchronize()
        out = {"rt_trace_rays": (self.hits,), "rt_occluded_rays": (self.blocked,), "rt_shade_rays": (self.rgba,), "rt_trace_paths": (self.seg, self.ends)}[entry]
        return [o.cpu().numpy().tobytes() for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_cull_rays.txt"))
    ap.add_argument("--counts", default="65,1685,10000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=31)
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    base = pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_QUERIES | pkg.RT_FLAG_STREAM_CULL
    lines = [f"RT_FLAG_STREAM | RT_FLAG_STREAM_QUERIES | RT_FLAG_STREAM_CULL without | with RT_FLAG_STREAM_CULL_RAYS, {W * H} rays (the {W}x{H} frame's own primary rays, "
             f"row order or shuffled), strict; stream_scenes.field(seed {SEED}), plain and mirrors=True, depth=2; two contexts alternating {args.rounds} times, one entry = "
             f"the median of {args.runs} synchronised calls (the library's event pair) after {WARM} warm-up calls; us; {torch.cuda.get_device_name(0)}",
             "per row: median of the medians [min .. max] for each series, flagged / unflagged, the unflagged series' spread, the verdict, and the work words of one "
             "flagged call: chunk decisions/staged, (lane, chunk) pairs asked/reaching, queries without a lane to cull for"]
    table = ["| spheres | scene | rays | entry point | unflagged us [min .. max] | flagged us [min .. max] | ratio | spread us | verdict | staged [1]/[0] | reach [3]/[2] |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]

    def emit(text):
        lines.append(text)
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:      # (rewritten row by row: a run that is cut short leaves what it measured)
            fh.write("\n".join(lines + ["", "the table of DESIGN.md section 29:"] + table) + "\n")

    for n in [int(x) for x in args.counts.split(",")]:
        for mirrors in (False, True):
            kind = "mirrors, depth 2" if mirrors else "plain"
            sc = S.field(pkg, n, SEED, w=W, h=H, mirrors=True, depth=2) if mirrors else S.field(pkg, n, SEED, w=W, h=H)
            os.environ.pop("MI355RT_STREAM_CULL_STATS", None)
            plain, cull = pkg.Renderer(sc, device=0, flags=base), pkg.Renderer(sc, device=0, flags=base | pkg.RT_FLAG_STREAM_CULL_RAYS)
            os.environ["MI355RT_STREAM_CULL_STATS"] = "1"
            counted = pkg.Renderer(sc, device=0, flags=base | pkg.RT_FLAG_STREAM_CULL_RAYS)
            try:
                assert plain.stream_cull and plain.streamed_queries and not plain.stream_cull_rays and cull.stream_cull_rays and counted.stream_cull_rays
                buf = Buffers(plain)
                for _ in range(WARM):
                    plain.update()
                frame = float(np.median([plain.update() for _ in range(args.runs)])) * 1e3
                emit(f"field {n:6d} {kind:16s} culled frame kernel (rt_render of the unflagged context), for scale: {frame:10.1f}")
                for order in ("row", "shuffled"):
                    for entry in ENTRY_POINTS:
                        for r in (plain, cull):
                            for _ in range(WARM):
                                buf.call(r, entry, order)
                        a, b = [], []
                        for _ in range(args.rounds):
                            a.append(float(np.median([buf.call(plain, entry, order) for _ in range(args.runs)])))
                            b.append(float(np.median([buf.call(cull, entry, order) for _ in range(args.runs)])))
                        out_cull = buf.output(entry)
                        buf.call(plain, entry, order)
                        same = out_cull == buf.output(entry)
                        before = counted.stream_cull_rays_stats()
                        buf.call(counted, entry, order)
                        w = [y - x for x, y in zip(before, counted.stream_cull_rays_stats())]
                        ma, mb, spread = float(np.median(a)), float(np.median(b)), max(a) - min(a)
                        verdict = "gain" if ma - mb > spread else ("overhead" if mb - ma > spread else "within the spread")
                        staged = w[1] / w[0] if w[0] else float("nan")
                        reach = w[3] / w[2] if w[2] else float("nan")
                        emit(f"field {n:6d} {kind:16s} {order:8s} {entry:16s} unflagged {ma:10.1f} [{min(a):10.1f} .. {max(a):10.1f}]  flagged {mb:10.1f} [{min(b):10.1f} .. "
                             f"{max(b):10.1f}]  x{mb / ma:6.3f}  spread {spread:8.1f}  {verdict:17s}  same outputs {same}  chunks {w[0]}/{w[1]} (staged {staged:.3f})  "
                             f"pairs {w[2]}/{w[3]} (reach {reach:.3f})  uncullable queries {w[4]}")
                        table.append(f"| {n} | {kind} | {order} | `{entry}` | {ma:.1f} [{min(a):.1f} .. {max(a):.1f}] | {mb:.1f} [{min(b):.1f} .. {max(b):.1f}] | {mb / ma:.3f} | "
                                     f"{spread:.1f} | {verdict} | {staged:.3f} | {reach:.3f} |")
                emit(f"field {n:6d} {kind:16s} done")
            finally:
                for r in (plain, cull, counted):
                    r.cleanup_update()
                del buf
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
