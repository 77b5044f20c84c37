#!/usr/bin/env python3
"""What RT_FLAG_STREAM_CULL_GROUPS changes in the culled streamed frame kernel's time (results:
profiles/stream_cull_groups.txt).

1920 x 1080, strict, RGBA32F.  Cases: the sphere field of tests/tools/stream_scenes.py at 1 685 (one group: decision false), 10 000,
100 000 and 400 000 spheres, and the mirrored field (every third sphere reflects, max_reflections = 2) at 10 000 and 100 000 with
RT_FLAG_STREAM_CULL_BOUNCE.  Each case is timed without and with RT_FLAG_STREAM_CULL_GROUPS, alternating five times in one process (two
contexts, created once, WITHOUT the work words: the kernels a product context runs); one series entry = the median of 31 synchronised
rt_render calls by the library's own event pair, after 5 warm-up frames.  Reported: the median of each series' five medians with
[min .. max], the spread (max - min) of the unflagged series, whether the two frames are equal bit for bit, and -- from a second pair of
contexts created under MI355RT_STREAM_CULL_STATS=1 -- one frame's work words of all three families for both contexts.  A difference counts
only where it exceeds the unflagged series' own spread.  Where the decision is true a third pair of contexts (with
RT_FLAG_STREAM_CULL_REORDER) times `rt_set_scene` + `rt_reorder_scene` of the unchanged coefficients without and with the flag: what the
group-bounds kernel behind each of them adds (torch events around the two enqueues, median of 31).
The scene is stream_scenes.field's, object for object, put together as arrays (a Scene of 400 000 objects added one call at a time takes
minutes).  Every case's lines are appended to the output file as soon as the case is done.

usage: stream_cull_groups_bench.py [--out profiles/stream_cull_groups.txt] [--px 2.6] [--fields 1685,10000,100000,400000]
                                   [--mirrored 10000,100000] [--rounds 5] [--runs 31] [--append]"""
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


def field_desc(pkg, n, mirrors, px):
    """stream_scenes.field(pkg, n, SEED, w=W, h=H, mirrors=mirrors, depth=2 if mirrors else 0, px=px) as a descriptor from arrays: the same
    draws from the same generator in the same order, the same surface_make per sphere, that scene's lights."""
    rng = np.random.default_rng(SEED)
    tan = np.tan(np.radians(S.FOV / 2))
    coefs, alb, refl = np.zeros((n, 20)), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    for i in range(n):
        z = rng.uniform(20.0, 30.0)
        half_h, half_w = z * tan, z * tan * W / H
        c = np.array([rng.uniform(-half_w, half_w) * 0.96, rng.uniform(-half_h, half_h) * 0.96, z])
        alb[i] = rng.uniform(0.2, 1.0, 3)
        refl[i] = float(rng.uniform(0.3, 0.8)) if (mirrors and i % 3 == 0) else 0.0
        coefs[i] = pkg.surface_make("sphere", c, [0.5 * px * 2.0 * z * tan / H])
        if i % 50000 == 49999:
            print(f"    ... {i + 1} of {n} spheres", flush=True)
    a = S.field(pkg, 1, SEED, w=W, h=H, depth=2 if mirrors else 0).arrays()
    d = pkg.desc_from_arrays(W, H, a["vertical_fov"], a["bg_color"], a["max_reflections"], coefs, refl, alb, a["light_is_spherical"], a["light_p"], a["light_color"])
    return d, coefs


def update_cost(pkg, sc, coefs, base, runs):
    """us of rt_set_scene + rt_reorder_scene (the scene's own coefficients again) without and with the flag: median of `runs`, torch events."""
    import torch
    os.environ.pop("MI355RT_STREAM_CULL_STATS", None)
    out = []
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        arr = torch.from_numpy(coefs).to("cuda:0")
    for flags in (base | pkg.RT_FLAG_STREAM_CULL_REORDER, base | pkg.RT_FLAG_STREAM_CULL_REORDER | pkg.RT_FLAG_STREAM_CULL_GROUPS):
        r = pkg.Renderer(sc, device=0, flags=flags)
        try:
            r.update(stream=s.cuda_stream, timed=False)
            ms = []
            for k in range(runs + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                r.set_scene_into(coefs=arr.data_ptr(), stream=s.cuda_stream, reorder=True)
                e1.record(s)
                s.synchronize()
                if k >= 3:
                    ms.append(e0.elapsed_time(e1))
            assert r.set_scene_status()["rejected"] == 0
            out.append(float(np.median(ms)) * 1e3)
        finally:
            r.cleanup_update()
    return out


def series(pkg, sc, base, rounds, runs):
    """(medians without the flag, medians with it, the decision, frames equal), in us: contexts that keep no work words."""
    os.environ.pop("MI355RT_STREAM_CULL_STATS", None)
    plain = pkg.Renderer(sc, device=0, flags=base)
    groups = pkg.Renderer(sc, device=0, flags=base | pkg.RT_FLAG_STREAM_CULL_GROUPS)
    try:
        assert plain.stream_cull and groups.stream_cull and not plain.stream_groups
        on = groups.stream_groups
        for r in (plain, groups):
            for _ in range(WARM):
                r.update()
        a, b = [], []
        for k in range(rounds):
            a.append(float(np.median([plain.update() for _ in range(runs)])) * 1e3)
            b.append(float(np.median([groups.update() for _ in range(runs)])) * 1e3)
            print(f"    ... round {k + 1}: {a[-1]:.1f} | {b[-1]:.1f} us", flush=True)
        same = bool(np.array_equal(plain.download().view(np.uint32), groups.download().view(np.uint32)))
        return a, b, on, same
    finally:
        plain.cleanup_update()
        groups.cleanup_update()


def words(pkg, sc, flags):
    """One frame's work words of a context created under MI355RT_STREAM_CULL_STATS=1: (frame family, bounce family or None, groups or None)."""
    os.environ["MI355RT_STREAM_CULL_STATS"] = "1"
    r = pkg.Renderer(sc, device=0, flags=flags)
    try:
        r.update()
        return (r.stream_cull_stats(), r.stream_cull_bounce_stats() if r.stream_cull_bounce else None, r.debug_stream_groups() if r.stream_groups else None)
    finally:
        r.cleanup_update()
        os.environ.pop("MI355RT_STREAM_CULL_STATS", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_cull_groups.txt"))
    ap.add_argument("--px", type=float, default=2.6, help="pixels across a sphere (stream_scenes.field)")
    ap.add_argument("--fields", default="1685,10000,100000,400000")
    ap.add_argument("--mirrored", default="10000,100000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=31)
    ap.add_argument("--append", action="store_true", help="add the cases to an existing output file (a run split over several calls)")
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    lines = [f"RT_FLAG_STREAM | RT_FLAG_STREAM_CULL [| RT_FLAG_STREAM_CULL_BOUNCE] without | with RT_FLAG_STREAM_CULL_GROUPS, {W}x{H}, strict, RGBA32F; stream_scenes.field("
             f"px={args.px:g}, seed {SEED}; mirrored: mirrors=True, depth=2); two contexts alternating {args.rounds} times, one entry = the median of {args.runs} "
             f"synchronised rt_render calls (the library's event pair) after {WARM} warm-up frames; us; {torch.cuda.get_device_name(0)}",
             "per case: median of the medians [min .. max] for each series, flagged / unflagged, the unflagged series' spread, the verdict under the rule "
             "(a difference counts only beyond that spread), then one frame's work words of contexts created under MI355RT_STREAM_CULL_STATS=1: "
             "rt_debug_stream_cull, rt_debug_stream_cull_bounce, rt_debug_stream_groups; where the decision is true, rt_set_scene + rt_reorder_scene without | with "
             "the flag (median of the same number of calls)"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as fh:
        if not args.append:
            fh.write("\n".join(lines) + "\n")
    cases = [("field", int(x), False) for x in args.fields.split(",") if x] + [("mirrored", int(x), True) for x in args.mirrored.split(",") if x]
    for name, n, mirrors in cases:
        first = len(lines)
        sc, coefs = field_desc(pkg, n, mirrors, args.px)
        base = pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL | (pkg.RT_FLAG_STREAM_CULL_BOUNCE if mirrors else 0)
        a, b, on, same = series(pkg, sc, base, args.rounds, args.runs)
        ma, mb, spread = float(np.median(a)), float(np.median(b)), max(a) - min(a)
        verdict = "gain beyond the spread" if ma - mb > spread else ("loss beyond the spread" if mb - ma > spread else "within the spread")
        lines.append(f"{name} {n:7d}   cull {ma:11.1f} [{min(a):11.1f} .. {max(a):11.1f}]  cull+groups {mb:11.1f} [{min(b):11.1f} .. {max(b):11.1f}]  x{mb / ma:6.3f}  "
                     f"spread {spread:9.1f}  {verdict}  decision {int(on)}  same frame {same}")
        print(lines[-1], flush=True)
        for label, flags in (("without", base), ("with   ", base | pkg.RT_FLAG_STREAM_CULL_GROUPS)):
            c, bo, g = words(pkg, sc, flags)
            lines.append(f"    words {label}: cull {c}  bounce {bo}  groups {g}")
            print(lines[-1], flush=True)
        if on:
            u0, u1 = update_cost(pkg, sc, coefs, base, args.runs)
            lines.append(f"    rt_set_scene + rt_reorder_scene: without {u0:9.1f}  with {u1:9.1f}  (+{u1 - u0:.1f} us: the group-bounds kernel behind each)")
            print(lines[-1], flush=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines[first:]) + "\n")


if __name__ == "__main__":
    main()
