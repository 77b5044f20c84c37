#!/usr/bin/env python3
"""What rt_reorder_scene costs and what it buys (RT_FLAG_STREAM_CULL_REORDER; results: profiles/reorder_scene.txt).

1920 x 1080, strict, RT_FLAG_STREAM | RT_FLAG_STREAM_CULL | RT_FLAG_STREAM_CULL_REORDER.  Scenes: the sphere field of
tests/tools/stream_scenes.py at 65, 1 685, 10 000 and 100 000 spheres (S0).  Motions (S1; radii, materials and classes kept, so rt_set_scene
accepts them): "mix" -- object i takes the centre of object pi(i) for a seeded permutation, plus a jitter (tests/tools/reorder_lab.py) --
and "drift k" -- k steps of a smooth flow, a rotation about the view axis whose rate falls with the distance from it, so neighbours
part slowly.

Per scene and motion, three contexts: `stale` (created on S0, rt_set_scene(S1)), `reordered` (the same, then rt_reorder_scene) and `fresh`
(created on S1).  Device time: each call is captured into a graph of K back-to-back repeats (K chosen so that one launch is about a
millisecond or one call), the graph is launched `runs` times between a pair of events after warm-up launches, one entry = the median
launch / K; the three frame series alternate `rounds` times in one process and a row shows the median of the medians with [min .. max].
Reported: rt_set_scene, rt_reorder_scene, the three frames, whether the reordered frame is the fresh one within the fresh series'
spread (they run the same bytes) and whether the three frames are equal bit for bit, the work words of one frame of each context
(from contexts created with MI355RT_STREAM_CULL_STATS=1), and the break-even: the number of frames after which the stale order's extra
frame time exceeds one reorder, reorder / (stale - reordered).

usage: reorder_scene_bench.py [--out profiles/reorder_scene.txt] [--counts 65,1685,10000,100000] [--drift 16,64,256] [--rounds 3] [--runs 15]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as graft  # noqa: E402
import reorder_lab as RL  # noqa: E402
import stream_scenes as S  # noqa: E402

W, H, WARM = 1920, 1080, 3
SEED = 3


def drift(coefs, steps, rate=0.02):
    """k steps of the flow: every centre turns about the view axis (x = y = 0) by rate / (1 + rho / 4) per step, rho its distance from it."""
    c, _ = RL.sphere_parts(coefs)
    rho = np.hypot(c[:, 0], c[:, 1])
    ang = steps * rate / (1.0 + rho / 4.0)
    new = c.copy()
    new[:, 0] = np.cos(ang) * c[:, 0] - np.sin(ang) * c[:, 1]
    new[:, 1] = np.sin(ang) * c[:, 0] + np.cos(ang) * c[:, 1]
    return RL.with_centres(coefs, new)


class Timed:
    """One call captured K times into a graph; series() = the median device time of one call over `runs` launches, in us."""

    def __init__(self, torch, stream, call, k):
        self.torch, self.s, self.k = torch, stream, k
        self.g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g, stream=stream):
            for _ in range(k):
                call()
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def launch(self):
        with self.torch.cuda.stream(self.s):
            self.e0.record()
            self.g.replay()
            self.e1.record()
        self.e1.synchronize()
        return self.e0.elapsed_time(self.e1) * 1e3 / self.k

    def series(self, runs):
        for _ in range(WARM):
            self.launch()
        return float(np.median([self.launch() for _ in range(runs)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reorder_scene.txt"))
    ap.add_argument("--counts", default="65,1685,10000,100000")
    ap.add_argument("--drift", default="16,64,256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--runs", type=int, default=15)
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    flags = pkg.RT_FLAG_STREAM | pkg.RT_FLAG_STREAM_CULL | pkg.RT_FLAG_STREAM_CULL_REORDER
    lines = [f"rt_reorder_scene: RT_FLAG_STREAM | RT_FLAG_STREAM_CULL | RT_FLAG_STREAM_CULL_REORDER, {W}x{H}, strict; stream_scenes.field(seed {SEED}); device time per call "
             f"from graphs of K repeats, median of {args.runs} launches after {WARM}; the frame series alternate {args.rounds} times: median of the medians [min .. max]; us; "
             f"{torch.cuda.get_device_name(0)}"]
    table = ["| spheres | motion | rt_set_scene us | rt_reorder_scene us | stale frame us | reordered frame us | fresh frame us | reordered vs fresh | chunks staged, primary [1]: stale / "
             "reordered / fresh | shadow [3]: stale / reordered / fresh | frames to break even |", "|---|---|---|---|---|---|---|---|---|---|---|"]

    def emit(text):
        lines.append(text)
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:      # (rewritten row by row: a run that is cut short leaves what it measured)
            fh.write("\n".join(lines + ["", "the table of DESIGN.md section 36:"] + table) + "\n")

    s = torch.cuda.Stream()
    for n in [int(x) for x in args.counts.split(",")]:
        sc = S.field(pkg, n, SEED, w=W, h=H)
        a = sc.arrays()
        motions = [("mix", RL.mix(a["coefs"]))] + ([(f"drift {k}", drift(a["coefs"], k)) for k in [int(x) for x in args.drift.split(",") if x]] if n <= 10000 else [])
        for name, coefs in motions:
            s1 = RL.scene_with(pkg, sc, coefs)
            os.environ.pop("MI355RT_STREAM_CULL_STATS", None)
            ctx = dict(stale=pkg.Renderer(sc, device=0, flags=flags), reordered=pkg.Renderer(sc, device=0, flags=flags), fresh=pkg.Renderer(s1, device=0, flags=flags))
            os.environ["MI355RT_STREAM_CULL_STATS"] = "1"
            counted = dict(live=pkg.Renderer(sc, device=0, flags=flags), fresh=pkg.Renderer(s1, device=0, flags=flags))
            os.environ.pop("MI355RT_STREAM_CULL_STATS", None)
            try:
                assert all(r.stream_cull and r.stream_cull_reorder for r in list(ctx.values()) + list(counted.values()))
                with torch.cuda.stream(s):
                    arr = torch.from_numpy(coefs.copy()).to("cuda:0")
                    bufs = {k: torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0") for k in ctx}
                for k, r in ctx.items():
                    r.update(stream=s.cuda_stream, timed=False)       # (every call of a context on the one stream the graphs are captured on)
                    if k != "fresh":
                        r.set_scene_into(coefs=arr.data_ptr(), stream=s.cuda_stream)
                    if k == "reordered":
                        r.reorder_scene(stream=s.cuda_stream)
                torch.cuda.synchronize()
                # one frame of each, for the repeat counts and the bit comparison
                once = {}
                for k, r in ctx.items():
                    once[k] = r.update(dev_fb=bufs[k].data_ptr(), stream=s.cuda_stream) * 1e3
                torch.cuda.synchronize()
                frames_equal = bool(torch.equal(bufs["stale"], bufs["fresh"]) and torch.equal(bufs["reordered"], bufs["fresh"]))
                reps = lambda us: max(1, min(16, int(1000.0 / max(us, 1.0))))   # noqa: E731
                runs = lambda us: max(5, min(args.runs, int(2e6 / max(us, 1.0))))   # noqa: E731
                live = ctx["reordered"]
                t_set = Timed(torch, s, lambda: live.set_scene_into(coefs=arr.data_ptr(), stream=s.cuda_stream), 8).series(args.runs)
                # (the update above leaves the order as it is; the reorder's launches and work do not depend on the order it meets)
                t_re = Timed(torch, s, lambda: live.reorder_scene(stream=s.cuda_stream), 4).series(args.runs)
                live.reorder_scene(stream=s.cuda_stream)
                graphs = {k: Timed(torch, s, (lambda r=r, k=k: r.update(dev_fb=bufs[k].data_ptr(), stream=s.cuda_stream, timed=False)), reps(once[k])) for k, r in ctx.items()}
                series = {k: [] for k in ctx}
                for _ in range(args.rounds):
                    for k in ctx:
                        series[k].append(graphs[k].series(runs(once[k])))
                med = {k: float(np.median(v)) for k, v in series.items()}
                spread = max(series["fresh"]) - min(series["fresh"])
                agree = "within the fresh series' spread" if abs(med["reordered"] - med["fresh"]) <= max(spread, 0.01 * med["fresh"]) else "DIFFERS beyond the fresh series' spread"
                # the work words of one frame each
                words = {}
                c = counted["live"]
                c.update()
                c.set_scene(coefs=coefs)
                for k in ("stale", "reordered"):
                    if k == "reordered":
                        c.reorder_scene()
                    before = c.stream_cull_stats()
                    c.update()
                    words[k] = [y - x for x, y in zip(before, c.stream_cull_stats())]
                before = counted["fresh"].stream_cull_stats()
                counted["fresh"].update()
                words["fresh"] = [y - x for x, y in zip(before, counted["fresh"].stream_cull_stats())]
                gain = med["stale"] - med["reordered"]
                even = f"{t_re / gain:.2f}" if gain > spread else "never (no gain beyond the spread)"
                fmt = lambda k: f"{med[k]:.1f} [{min(series[k]):.1f} .. {max(series[k]):.1f}]"   # noqa: E731
                emit(f"field {n:6d} {name:9s} rt_set_scene {t_set:9.1f}  rt_reorder_scene {t_re:9.1f}  frame: stale {fmt('stale')}  reordered {fmt('reordered')}  fresh {fmt('fresh')}  "
                     f"reordered vs fresh: {agree}; frames bit-equal {frames_equal}; words equal {words['reordered'] == words['fresh']}; break-even after {even} frames")
                for k in ("stale", "reordered", "fresh"):
                    emit(f"field {n:6d} {name:9s}   work words, {k:9s}: {words[k]}")
                table.append(f"| {n} | {name} | {t_set:.1f} | {t_re:.1f} | {fmt('stale')} | {fmt('reordered')} | {fmt('fresh')} | {agree} | "
                             f"{words['stale'][1]} / {words['reordered'][1]} / {words['fresh'][1]} | {words['stale'][3]} / {words['reordered'][3]} / {words['fresh'][3]} | {even} |")
                emit(f"field {n:6d} {name:9s} done")
                del graphs
            finally:
                torch.cuda.synchronize()
                for r in list(ctx.values()) + list(counted.values()):
                    r.cleanup_update()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
