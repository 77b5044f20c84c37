#!/usr/bin/env python3
"""What rt_sort_rays buys the culled ray queries (results: profiles/sort_rays.txt, whose last part is the table of
that section).

1920 x 1080 rays, strict, RT_FLAG_STREAM | RT_FLAG_STREAM_QUERIES | RT_FLAG_STREAM_CULL | RT_FLAG_STREAM_CULL_RAYS.  Scenes: the sphere
field of tests/tools/stream_scenes.py at 10 000, 1 685 and 65 spheres.  Rays: the context's own primary rays (rt_primary_rays) in row
order, in 8 x 8 block order and shuffled (a fixed permutation); a wave is 64 consecutive rays.  Per row four series, alternating five times
in one process: the entry point on the caller's order; rt_sort_rays alone (sorted rays and perm, no keys); the entry point on the sorted
rays; rt_permute (scatter) of its result.  One series entry = the median of 31 synchronised calls by the library's own event pair, after 5
warm-up calls.  Reported: the median of each series' five medians with [min .. max], the sum of the last three, the spread (max - min) of
the unsorted series, the verdict -- a difference counts only beyond that spread --, whether the scattered result equals the unsorted call's
bit for bit, and the staged fraction [1] / [0] before and after (rt_debug_stream_cull_rays of a third context created with
MI355RT_STREAM_CULL_STATS=1).  Once per scene: rt_sort_rays' time against the bytes it has to move per ray.

usage: sort_rays_bench.py [--out profiles/sort_rays.txt] [--counts 10000,1685,65] [--entries rt_trace_rays,...] [--rounds 5] [--runs 31]"""
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
ORDERS = ("row", "block", "shuffled")
# what one ray costs rt_sort_rays in memory traffic: the box pass and the key pass read it (48 + 48) and write a pair (8); each of the four
# passes reads the keys for the histogram (4), reads and writes the pairs (8 + 8); the gather reads perm and the ray and writes the ray
SORT_BYTES_PER_RAY = 48 + 48 + 8 + 4 * (4 + 8 + 8) + (4 + 48 + 48)


class Buffers:
    """The rays in every order, the sort's outputs and work space and every entry point's outputs (in the order traced and scattered
    back), on the device, once per scene."""

    def __init__(self, r):
        import torch
        self.n = n = W * H
        rays, _ = r.primary_rays()
        dev = rays.device
        flat = rays.reshape(-1, 6)
        idx = np.arange(n)
        y, x = idx // W, idx % W
        block = np.lexsort((x % 8, y % 8, x // 8, y // 8))
        gen = torch.Generator(device="cpu").manual_seed(29)
        self.rays = {"row": flat.contiguous(), "block": flat[torch.from_numpy(block).to(dev)].contiguous(), "shuffled": flat[torch.randperm(n, generator=gen).to(dev)].contiguous()}
        self.m = r._max_segments(None)
        self.sorted = torch.zeros((n, 6), dtype=torch.float64, device=dev)
        self.perm = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.work_bytes = r.sort_work_bytes(n)
        self.work = torch.zeros((self.work_bytes,), dtype=torch.uint8, device=dev)
        shapes = {"rt_trace_rays": [((n, 6), torch.float64)], "rt_occluded_rays": [((n,), torch.int32)], "rt_shade_rays": [((n, 4), torch.float32)],
                  "rt_trace_paths": [((self.m * n, 6), torch.float64), ((n, 4), torch.int32)]}
        self.out = {k: [torch.zeros(s, dtype=t, device=dev) for s, t in v] for k, v in shapes.items()}
        self.back = {k: [torch.zeros(s, dtype=t, device=dev) for s, t in v] for k, v in shapes.items()}
        torch.cuda.synchronize()

    def call(self, r, entry, ray_ptr):
        """One synchronised call of the entry point; the library's own time in us."""
        o = self.out[entry]
        if entry == "rt_trace_rays":
            return r.trace_into(ray_ptr, self.n, o[0].data_ptr()) * 1e3
        if entry == "rt_occluded_rays":
            return r.occluded_into(ray_ptr, None, self.n, o[0].data_ptr()) * 1e3
        if entry == "rt_shade_rays":
            return r.shade_into(ray_ptr, self.n, o[0].data_ptr()) * 1e3
        return r.paths_into(ray_ptr, self.n, self.m, o[0].data_ptr(), None, o[1].data_ptr()) * 1e3

    def sort(self, r, order):
        return r.sort_rays_into(self.rays[order].data_ptr(), self.n, self.sorted.data_ptr(), self.perm.data_ptr(), None, self.work.data_ptr(), self.work_bytes) * 1e3

    def scatter(self, r, entry):
        """The entry point's outputs back into the caller's order: one rt_permute per output; us."""
        elems = {"rt_trace_rays": [(48, 1)], "rt_occluded_rays": [(4, 1)], "rt_shade_rays": [(16, 1)], "rt_trace_paths": [(48, self.m), (16, 1)]}[entry]
        return sum(r.permute_into(self.perm.data_ptr(), self.n, src.data_ptr(), dst.data_ptr(), e, planes=p, scatter=True)
                   for src, dst, (e, p) in zip(self.out[entry], self.back[entry], elems)) * 1e3

    def bytes_of(self, which, entry):
        import torch
        torch.cuda.synchronize()
        return [o.cpu().numpy().tobytes() for o in which[entry]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sort_rays.txt"))
    ap.add_argument("--counts", default="10000,1685,65")
    ap.add_argument("--entries", default=",".join(ENTRY_POINTS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=31)
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    flags = pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_QUERIES | pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_RAYS
    lines = [f"rt_sort_rays + entry point on the sorted rays + rt_permute against the entry point on the caller's order; RT_FLAG_STREAM | RT_FLAG_STREAM_QUERIES | "
             f"RT_FLAG_STREAM_CULL | RT_FLAG_STREAM_CULL_RAYS, {W * H} rays (the {W}x{H} frame's own primary rays in row order, 8 x 8 block order or shuffled), strict; "
             f"stream_scenes.field(seed {SEED}); four series alternating {args.rounds} times, one entry = the median of {args.runs} synchronised calls (the library's event "
             f"pair) after {WARM} warm-up calls; us; {torch.cuda.get_device_name(0)}",
             "per row: median of the medians [min .. max] of each series, the sum sort + sorted call + scatter, sum / unsorted, the unsorted series' spread, the verdict "
             "(a difference counts only beyond that spread), and the staged fraction [1]/[0] of the work words before and after the sort"]
    table = ["| spheres | rays | entry point | unsorted us [min .. max] | rt_sort_rays us | sorted call us | rt_permute us | sum us | sum / unsorted | spread us | verdict | "
             "staged before | staged after |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]

    def emit(text):
        lines.append(text)
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:      # (rewritten row by row: a run that is cut short leaves what it measured)
            fh.write("\n".join(lines + ["", "the table of DESIGN.md section 31:"] + table) + "\n")

    def med(f):
        return float(np.median([f() for _ in range(args.runs)]))

    for n in [int(x) for x in args.counts.split(",")]:
        sc = S.field(pkg, n, SEED, w=W, h=H)
        os.environ.pop("MI355RT_STREAM_CULL_STATS", None)
        r = pkg.Renderer(sc, device=0, flags=flags)
        os.environ["MI355RT_STREAM_CULL_STATS"] = "1"
        counted = pkg.Renderer(sc, device=0, flags=flags)
        os.environ.pop("MI355RT_STREAM_CULL_STATS", None)
        buf = None
        try:
            assert r.stream_cull_rays and counted.stream_cull_rays
            buf = Buffers(r)
            for order in ORDERS:
                for _ in range(WARM):
                    buf.sort(r, order)
                t = [med(lambda: buf.sort(r, order)) for _ in range(args.rounds)]
                gbs = SORT_BYTES_PER_RAY * buf.n / (float(np.median(t)) * 1e-6) / 1e9
                emit(f"field {n:6d} {order:8s} rt_sort_rays alone {float(np.median(t)):9.1f} [{min(t):9.1f} .. {max(t):9.1f}]  {SORT_BYTES_PER_RAY} bytes per ray to move: "
                     f"{gbs:7.1f} GB/s  ({buf.work_bytes / buf.n:.2f} bytes of work space per ray)")
                for entry in args.entries.split(","):
                    src, srt = buf.rays[order].data_ptr(), buf.sorted.data_ptr()
                    buf.sort(r, order)
                    for _ in range(WARM):
                        buf.call(r, entry, src), buf.call(r, entry, srt), buf.scatter(r, entry)
                    a, b, c, d = [], [], [], []
                    for _ in range(args.rounds):
                        a.append(med(lambda: buf.call(r, entry, src)))
                        b.append(med(lambda: buf.sort(r, order)))
                        c.append(med(lambda: buf.call(r, entry, srt)))
                        d.append(med(lambda: buf.scatter(r, entry)))
                    scattered = buf.bytes_of(buf.back, entry)
                    buf.call(r, entry, src)
                    same = scattered == buf.bytes_of(buf.out, entry)
                    words = []
                    for p in (src, srt):
                        before = counted.stream_cull_rays_stats()
                        buf.call(counted, entry, p)
                        words.append([y - x for x, y in zip(before, counted.stream_cull_rays_stats())])
                    staged = [w[1] / w[0] if w[0] else float("nan") for w in words]
                    ma, mb, mc, md = (float(np.median(v)) for v in (a, b, c, d))
                    total, spread = mb + mc + md, max(a) - min(a)
                    verdict = "gain" if ma - total > spread else ("loss" if total - ma > spread else "within the spread")
                    emit(f"field {n:6d} {order:8s} {entry:16s} unsorted {ma:10.1f} [{min(a):10.1f} .. {max(a):10.1f}]  sort {mb:8.1f} [{min(b):8.1f} .. {max(b):8.1f}]  sorted call "
                         f"{mc:10.1f} [{min(c):10.1f} .. {max(c):10.1f}]  scatter {md:7.1f} [{min(d):7.1f} .. {max(d):7.1f}]  sum {total:10.1f}  x{total / ma:6.3f}  spread {spread:8.1f}  "
                         f"{verdict:17s}  same result {same}  staged {staged[0]:.3f} -> {staged[1]:.3f}  (chunks {words[0][0]}/{words[0][1]} -> {words[1][0]}/{words[1][1]})")
                    table.append(f"| {n} | {order} | `{entry}` | {ma:.1f} [{min(a):.1f} .. {max(a):.1f}] | {mb:.1f} | {mc:.1f} | {md:.1f} | {total:.1f} | {total / ma:.3f} | {spread:.1f} | "
                                 f"{verdict} | {staged[0]:.3f} | {staged[1]:.3f} |")
            emit(f"field {n:6d} done")
        finally:
            r.cleanup_update()
            counted.cleanup_update()
            buf = None
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
