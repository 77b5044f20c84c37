#!/usr/bin/env python3
"""What the streamed query kernels cost next to the staged ones (results: profiles/stream_queries.txt).

Device time of one call by the entry point's own `ms` (the library's event pair around its kernels), median of 21 synchronised calls
after 3 warm-up calls; the staged and the streamed call of one row alternate in one process; 1920 x 1080, strict.
  (a) a field of 2 560 spheres (tests/tools/extents_ref.py: sphere_field, with a point light more: the most the staged kernels take), a
      context without the flag against one with RT_FLAG_STREAM_QUERIES (streamed by size, so the flag alone streams its queries):
      rt_trace_rays, rt_occluded_rays, rt_shade_rays and rt_trace_paths on the frame's primary rays (rt_primary_rays), rt_render_gbuffer
      and rt_object_extents of the whole frame, the last two also with RT_FLAG_NOCULL;
  (b) 10 000 spheres: the streamed figures alone.

usage: stream_queries_bench.py [--out profiles/stream_queries.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as graft  # noqa: E402
import extents_ref  # noqa: E402

W, H, WARM, RUNS = 1920, 1080, 3, 21
STAGED_LIMIT = 160 * 1024 // 64   # spheres whose table is exactly the LDS a workgroup can have


def field(pkg, n):
    sc = extents_ref.sphere_field(pkg, n, 3, w=W, h=H)
    sc.add_light("spherical", [3.0, 8.0, 5.0], (1.0, 0.9, 0.8), 400.0)
    return sc


class Calls:
    """The six timed calls of one context, on buffers of its own."""

    def __init__(self, pkg, sc, flags):
        import torch
        self.r = pkg.Renderer(sc, device=0, flags=flags)
        r, n, dev = self.r, W * H, "cuda:0"
        self.rays, _ = r.primary_rays()
        self.hits = torch.empty((n, 6), dtype=torch.float64, device=dev)
        self.last = torch.empty((n, 6), dtype=torch.float64, device=dev)
        self.seg = torch.empty((n, 6), dtype=torch.float64, device=dev)
        self.ends = torch.empty((n, 4), dtype=torch.int32, device=dev)
        self.flags = torch.empty((n,), dtype=torch.int32, device=dev)
        self.rgba = torch.empty((n, 4), dtype=torch.float32, device=dev)
        self.po = torch.empty((H, W), dtype=torch.int32, device=dev)
        self.pt = torch.empty((H, W), dtype=torch.float64, device=dev)
        self.pn = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        self.ext = torch.empty((r._desc.n_objects * 5,), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        p = self.rays.data_ptr()
        self.calls = {
            "rt_trace_rays": lambda: r.trace_into(p, n, self.hits.data_ptr()),
            "rt_occluded_rays": lambda: r.occluded_into(p, None, n, self.flags.data_ptr()),
            "rt_shade_rays": lambda: r.shade_into(p, n, self.rgba.data_ptr()),
            "rt_trace_paths": lambda: r.paths_into(p, n, 1, self.seg.data_ptr(), self.last.data_ptr(), self.ends.data_ptr()),
            "rt_render_gbuffer": lambda: r.gbuffer_into(None, self.po.data_ptr(), self.pt.data_ptr(), self.pn.data_ptr()),
            "rt_object_extents": lambda: r.object_extents_into(None, None, self.ext.data_ptr()),
        }

    def close(self):
        self.r.cleanup_update()


def alternating(contexts, name):
    """Per context the (median, min) in us of RUNS synchronised calls, the contexts taking turns."""
    import torch
    ms = [[] for _ in contexts]
    for k in range(WARM + RUNS):
        for i, c in enumerate(contexts):
            t = c.calls[name]()
            torch.cuda.synchronize()
            if k >= WARM:
                ms[i].append(t)
    return [(float(np.median(m)) * 1e3, float(min(m)) * 1e3) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_queries.txt"))
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    lines = [f"streamed query kernels, {W}x{H} ({W * H} rays / pixels), strict; device us per call by the entry point's own ms, median of {RUNS} synchronised calls "
             f"after {WARM} warm-up calls (min in brackets), staged and streamed alternating; {torch.cuda.get_device_name(0)}"]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    names = ("rt_trace_rays", "rt_occluded_rays", "rt_shade_rays", "rt_trace_paths", "rt_render_gbuffer", "rt_object_extents")
    say(f"(a) sphere field, {STAGED_LIMIT} spheres (the most the staged kernels take), two lights: no flag (staged) | RT_FLAG_STREAM_QUERIES (streamed)")
    sc = field(pkg, STAGED_LIMIT)
    for extra, label, which in ((0, "", names), (pkg.RT_FLAG_NOCULL, ", RT_FLAG_NOCULL", names[4:])):
        pair = [Calls(pkg, sc, extra), Calls(pkg, sc, extra | pkg.RT_FLAG_STREAM_QUERIES)]
        try:
            assert not pair[0].r.streamed_queries and pair[1].r.streamed_queries
            for name in which:
                (a, a_lo), (b, b_lo) = alternating(pair, name)
                say(f"{name + label:36s} staged {a:10.1f} [{a_lo:10.1f}]  streamed {b:10.1f} [{b_lo:10.1f}]  x{b / a:6.2f}")
        finally:
            for c in pair:
                c.close()
    say("(b) sphere field, 10000 spheres: RT_FLAG_STREAM_QUERIES (no staged kernel takes it)")
    sc = field(pkg, 10000)
    for extra, label, which in ((0, "", names), (pkg.RT_FLAG_NOCULL, ", RT_FLAG_NOCULL", names[4:])):
        c = Calls(pkg, sc, extra | pkg.RT_FLAG_STREAM_QUERIES)
        try:
            assert c.r.streamed_queries
            for name in which:
                (b, b_lo), = alternating([c], name)
                say(f"{name + label:36s} streamed {b:10.1f} [{b_lo:10.1f}]")
        finally:
            c.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
