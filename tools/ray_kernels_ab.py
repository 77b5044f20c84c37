#!/usr/bin/env python3
"""Two builds of libmi355rt.so on the kernels for caller-supplied rays (results: profiles/ray_kernel_bodies.txt).

  python tools/ray_kernels_ab.py --parent <another build's libmi355rt.so> [--out FILE] [--only staged,streamed,culled] [--rounds 4] [--runs 31]

The other library is selected with MI355RT_LIB; the Python binding and the scenes are this tree's for both.  Per configuration (a scene
and the context's flags) one child process per library, each holding one context and its buffers: the frame's own primary rays
(rt_primary_rays) in row order and in a fixed random permutation, 1920 x 1080, strict, RGBA32F.  A series is (configuration, entry point,
ray order); the two children are asked in turn, `rounds` times; one entry = the median of `runs` synchronised calls by the library's own
event pair after 5 warm-up calls; us.  Per series: the median of each side's medians [min .. max], this tree / parent, the parent's
spread (max - min of its medians), the verdict -- a difference counts only beyond the spread of the unchanged side -- and whether the
two libraries' outputs are equal bit for bit.  Configurations: the scenes and flags of tools/rays_bench.py, shade_bench.py, paths_bench.py
(20spheres, clebsch, reflection_test at depth 4; staged kernels), stream_queries_bench.py (its field at 2 560 spheres staged and streamed,
at 10 000 streamed) and stream_cull_rays_bench.py (its field at 1 685 and 10 000 spheres with RT_FLAG_STREAM_CULL_RAYS).  The control is
rt_render of the first configuration's context, whose kernel no build of these files changes."""
import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, WARM = 1920, 1080, 5
ENTRY_POINTS = ("rt_trace_rays", "rt_occluded_rays", "rt_shade_rays", "rt_trace_paths")
# name -> (family, scene, flag names)
CONFIGS = {
    "20spheres": ("staged", ("file", "20spheres", -1), ()),
    "clebsch": ("staged", ("file", "clebsch", -1), ()),
    "reflection_test d4": ("staged", ("file", "reflection_test", 4), ()),
    "field 2560 staged": ("staged", ("queries_field", 2560), ()),
    "field 2560 streamed": ("streamed", ("queries_field", 2560), ("RT_FLAG_STREAM_QUERIES",)),
    "field 10000 streamed": ("streamed", ("queries_field", 10000), ("RT_FLAG_STREAM_QUERIES",)),
    "field 1685 culled": ("culled", ("cull_field", 1685, False), ("RT_FLAG_STREAM", "RT_FLAG_STREAM_QUERIES", "RT_FLAG_STREAM_CULL", "RT_FLAG_STREAM_CULL_RAYS")),
    "mirrors 1685 culled": ("culled", ("cull_field", 1685, True), ("RT_FLAG_STREAM", "RT_FLAG_STREAM_QUERIES", "RT_FLAG_STREAM_CULL", "RT_FLAG_STREAM_CULL_RAYS")),
    "mirrors 10000 culled": ("culled", ("cull_field", 10000, True), ("RT_FLAG_STREAM", "RT_FLAG_STREAM_QUERIES", "RT_FLAG_STREAM_CULL", "RT_FLAG_STREAM_CULL_RAYS")),
}


def child(config, runs):
    """Holds one context; answers `entry order` with the median of `runs` calls (5 warm-up calls the first time), `out entry order` with a
    digest of the outputs of one call, on stdout; leaves at end of input."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import torch
    import __graft_entry__ as graft
    pkg = graft.load_package()
    family, scene, flag_names = CONFIGS[config]
    if scene[0] == "file":
        sc = pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", scene[1] + ".yml")).set_size(W, H)
        if scene[2] >= 0:
            sc.set_max_reflections(scene[2])
    elif scene[0] == "queries_field":
        import extents_ref
        sc = extents_ref.sphere_field(pkg, scene[1], 3, w=W, h=H)
        sc.add_light("spherical", [3.0, 8.0, 5.0], (1.0, 0.9, 0.8), 400.0)
    else:
        import stream_scenes
        sc = stream_scenes.field(pkg, scene[1], 3, w=W, h=H, mirrors=True, depth=2) if scene[2] else stream_scenes.field(pkg, scene[1], 3, w=W, h=H)
    flags = 0
    for name in flag_names:
        flags |= getattr(pkg, name)
    r = pkg.Renderer(sc, device=0, flags=flags)
    assert r.streamed_queries == (family != "staged") and r.stream_cull_rays == (family == "culled"), config
    n, dev = W * H, "cuda:0"
    rays, _ = r.primary_rays()
    gen = torch.Generator(device="cpu").manual_seed(29)
    order = {"row": rays.reshape(-1, 6).contiguous(), "shuffled": rays.reshape(-1, 6)[torch.randperm(n, generator=gen).to(rays.device)].contiguous()}
    m = r._max_segments(None)
    hits = torch.zeros((n, 6), dtype=torch.float64, device=dev)
    blocked = torch.zeros((n,), dtype=torch.int32, device=dev)
    rgba = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    seg = torch.zeros((m * n, 6), dtype=torch.float64, device=dev)
    last = torch.zeros((n, 6), dtype=torch.float64, device=dev)
    ends = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    calls = {"rt_trace_rays": (lambda p: r.trace_into(p, n, hits.data_ptr()), (hits,)),
             "rt_occluded_rays": (lambda p: r.occluded_into(p, None, n, blocked.data_ptr()), (blocked,)),
             "rt_shade_rays": (lambda p: r.shade_into(p, n, rgba.data_ptr(), hits.data_ptr()), (rgba, hits)),       # with the hit records
             "rt_trace_paths": (lambda p: r.paths_into(p, n, m, seg.data_ptr(), last.data_ptr(), ends.data_ptr()), (seg, last, ends)),
             "rt_render": (lambda p: r.update(), ())}
    warm = set()
    print("ready", flush=True)
    for line in sys.stdin:
        words = line.split()
        digest = words[0] == "out"
        entry, which = words[-2], words[-1]
        call, outputs = calls[entry]
        p = order[which].data_ptr()
        if digest:
            call(p)
            torch.cuda.synchronize()
            h = hashlib.sha256()
            for o in outputs:
                h.update(o.cpu().numpy().tobytes())
            if not outputs:
                h.update(np.ascontiguousarray(r.download()).tobytes())      # (the control: the frame)
            print(h.hexdigest(), flush=True)
            continue
        if (entry, which) not in warm:
            for _ in range(WARM):
                call(p)
            warm.add((entry, which))
        print(repr(float(np.median([call(p) for _ in range(runs)])) * 1e3), flush=True)
    r.cleanup_update()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_kernel_bodies_timings.txt"))
    ap.add_argument("--only", default="staged,streamed,culled")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--runs", type=int, default=31)
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.runs)
    lines = []

    def emit(text):
        lines.append(text)
        print(text, flush=True)
        with open(args.out, "w") as fh:      # (rewritten row by row: a run that is cut short leaves what it measured)
            fh.write("\n".join(lines) + "\n")

    def ask(proc, text):
        proc.stdin.write(text + "\n")
        proc.stdin.flush()
        answer = proc.stdout.readline().strip()
        if not answer:
            raise RuntimeError(f"a child left ({proc.poll()}) at: {text}")
        return answer

    first = True
    for config, (family, _, _) in CONFIGS.items():
        if family not in args.only.split(","):
            continue
        procs = []
        try:
            for lib in (args.parent, None):
                env = dict(os.environ)
                env.pop("MI355RT_LIB", None)
                if lib:
                    env["MI355RT_LIB"] = os.path.abspath(lib)
                procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", config, "--runs", str(args.runs)], env=env, stdin=subprocess.PIPE,
                                              stdout=subprocess.PIPE, text=True))
            for p in procs:
                if p.stdout.readline().strip() != "ready":
                    raise RuntimeError(f"{config}: a child did not start ({p.poll()})")
            series = [(e, o) for o in ("row", "shuffled") for e in ENTRY_POINTS] + ([("rt_render", "row")] if first else [])
            first = False
            for entry, which in series:
                a, b = [], []
                for _ in range(args.rounds):
                    a.append(float(ask(procs[0], f"{entry} {which}")))
                    b.append(float(ask(procs[1], f"{entry} {which}")))
                same = ask(procs[0], f"out {entry} {which}") == ask(procs[1], f"out {entry} {which}")
                ma, mb, spread = float(np.median(a)), float(np.median(b)), max(a) - min(a)
                verdict = "faster beyond the spread" if ma - mb > spread else ("SLOWER beyond the spread" if mb - ma > spread else "within the spread")
                name = "control: rt_render" if entry == "rt_render" else entry
                emit(f"{family:9s}{config:22s}{name:19s}{which:9s} parent {ma:10.1f} [{min(a):10.1f} .. {max(a):10.1f}]  this tree {mb:10.1f} [{min(b):10.1f} .. {max(b):10.1f}]  "
                     f"x {mb / ma:6.4f}  spread {spread:8.1f} ({100.0 * spread / ma:5.2f} %)  {verdict:25s} same result {same}")
        finally:
            for p in procs:
                p.stdin.close()
            for p in procs:
                p.wait(timeout=60)
    return 0


if __name__ == "__main__":
    sys.exit(main())
