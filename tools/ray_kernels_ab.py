#!/usr/bin/env python3
"""Two builds of libmi355rt.so on the kernels for caller-supplied rays (results: profiles/ray_kernel_bodies.txt), on
the pixel queries (section 32; profiles/pixel_kernel_bodies.txt) and on the adaptive passes (section 33; profiles/adaptive_passes.txt).

  python tools/ray_kernels_ab.py --parent <another build's libmi355rt.so> [--out FILE] [--only staged,streamed,culled] [--rounds 4] [--runs 31]
  python tools/ray_kernels_ab.py --parent <another build's libmi355rt.so> --only pixels,geometry [--fast] [--out FILE]
  python tools/ray_kernels_ab.py --parent <another build's libmi355rt.so> --only adaptive,geometry [--fast] [--out FILE]

The other library is selected with MI355RT_LIB; the Python binding and the scenes are this tree's for both.  Per configuration (a scene
and the context's flags) one child process per library, each holding one context and its buffers: the frame's own primary rays
(rt_primary_rays) in row order and in a fixed random permutation, 1920 x 1080, strict, RGBA32F.  A series is (configuration, entry point,
ray order); the two children are asked in turn, `rounds` times; one entry = the median of `runs` synchronised calls by the library's own
event pair after 5 warm-up calls; us.  Per series: the median of each side's medians [min .. max], this tree / parent, the parent's
spread (max - min of its medians), the verdict -- a difference counts only beyond the spread of the unchanged side -- and whether the
two libraries' outputs are equal bit for bit.  Configurations: the scenes and flags of tools/rays_bench.py, shade_bench.py, paths_bench.py
(20spheres, clebsch, reflection_test at depth 4; staged kernels), stream_queries_bench.py (its field at 2 560 spheres staged and streamed,
at 10 000 streamed) and stream_cull_rays_bench.py (its field at 1 685 and 10 000 spheres with RT_FLAG_STREAM_CULL_RAYS).  The control is
rt_render of the first configuration's context, whose kernel no build of these files changes.
The pixel queries (--only pixels,geometry; --fast: RT_FLAG_FAST contexts): per configuration rt_render_gbuffer with all three planes,
rt_object_extents of the whole frame and of a 64 x 64 rectangle in its middle, and rt_pick of 4 096 fixed random pixels (outputs only:
the call has no event pair) -- the scenes of tools/gbuffer_bench.py and extents_bench.py (20spheres, clebsch) and of
stream_queries_bench.py (its field at 2 560 spheres staged and streamed, with and without RT_FLAG_NOCULL, and at 10 000 streamed) --;
and the frame of an RT_FLAG_SSAA4 | RT_FLAG_SSAA_ADAPTIVE | RT_FLAG_SSAA_GEOMETRY context (min_cos 0.999, tau 1/32: the G pass writes
ids and normals) as the only rank and as rank 0 of 2 (the halo rows' records: the kernel's picking mode), the scenes of
tools/ssaa_geometry_bench.py staged and the culled field at 1 685 spheres with the adaptive passes streamed.
The adaptive passes (--only adaptive): the frame (rt_render) of RT_FLAG_SSAA2 | RT_FLAG_SSAA_ADAPTIVE and RT_FLAG_SSAA4 | RT_FLAG_SSAA_ADAPTIVE
contexts at the default threshold, RGBA32F and RGBA8, as the only rank and as rank 0 of 2 (the halo pass), the scenes of
tools/ssaa_adaptive_bench.py (20spheres, clebsch); and the field at 1 685 spheres with the passes streamed (RT_FLAG_STREAM |
RT_FLAG_STREAM_ADAPTIVE) and with RT_FLAG_STREAM_CULL added.  Compared outputs: the frame and the refined count."""
import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, WARM = 1920, 1080, 5
ENTRY_POINTS = ("rt_trace_rays", "rt_occluded_rays", "rt_shade_rays", "rt_trace_paths")
GEOMETRY = ("RT_FLAG_SSAA4", "RT_FLAG_SSAA_ADAPTIVE", "RT_FLAG_SSAA_GEOMETRY")
ADAPTIVE = {2: ("RT_FLAG_SSAA2", "RT_FLAG_SSAA_ADAPTIVE"), 4: ("RT_FLAG_SSAA4", "RT_FLAG_SSAA_ADAPTIVE")}
# name -> (family, scene, flag names[, world[, format]])
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
    # the pixel queries: family "pixels" (G-buffer, extents, picks) and "geometry" (name, world) -> the adaptive frame with the geometric term
    "px 20spheres": ("pixels", ("file", "20spheres", -1), ()),
    "px clebsch": ("pixels", ("file", "clebsch", -1), ()),
    "px field 2560": ("pixels", ("queries_field", 2560), ()),
    "px field 2560 nocull": ("pixels", ("queries_field", 2560), ("RT_FLAG_NOCULL",)),
    "px field 2560 str": ("pixels", ("queries_field", 2560), ("RT_FLAG_STREAM_QUERIES",)),
    "px field 2560 str nc": ("pixels", ("queries_field", 2560), ("RT_FLAG_STREAM_QUERIES", "RT_FLAG_NOCULL")),
    "px field 10000 str": ("pixels", ("queries_field", 10000), ("RT_FLAG_STREAM_QUERIES",)),
    "geo 20spheres": ("geometry", ("file", "20spheres", -1), GEOMETRY, 1),
    "geo 20spheres 0/2": ("geometry", ("file", "20spheres", -1), GEOMETRY, 2),
    "geo clebsch": ("geometry", ("file", "clebsch", -1), GEOMETRY, 1),
    "geo clebsch 0/2": ("geometry", ("file", "clebsch", -1), GEOMETRY, 2),
    "geo field 1685 str": ("geometry", ("cull_field", 1685, False), GEOMETRY + ("RT_FLAG_STREAM", "RT_FLAG_STREAM_ADAPTIVE"), 1),
    "geo field 1685 str 0/2": ("geometry", ("cull_field", 1685, False), GEOMETRY + ("RT_FLAG_STREAM", "RT_FLAG_STREAM_ADAPTIVE"), 2),
}
# the adaptive passes: family "adaptive" -> the adaptive frame without the geometric term, per k, format and layout
for _scene in ("20spheres", "clebsch"):
    for _k in (2, 4):
        for _fmt in ("RGBA32F", "RGBA8"):
            for _world in (1, 2):
                CONFIGS[f"ada{_k} {_scene} {_fmt[4:].lower()}" + (" 0/2" if _world == 2 else "")] = ("adaptive", ("file", _scene, -1), ADAPTIVE[_k], _world, _fmt)
CONFIGS["ada4 field 1685 str"] = ("adaptive", ("cull_field", 1685, False), ADAPTIVE[4] + ("RT_FLAG_STREAM", "RT_FLAG_STREAM_ADAPTIVE"), 1, "RGBA32F")
CONFIGS["ada4 field 1685 cull"] = ("adaptive", ("cull_field", 1685, False), ADAPTIVE[4] + ("RT_FLAG_STREAM", "RT_FLAG_STREAM_ADAPTIVE", "RT_FLAG_STREAM_CULL"), 1, "RGBA32F")
PIXEL_SERIES = (("rt_render_gbuffer", "planes"), ("rt_object_extents", "frame"), ("rt_object_extents", "64x64"), ("rt_pick", "4096px"))
UNTIMED = ("rt_pick",)      # (blocks and copies to the host: no event pair of its own; its outputs are compared)


def child(config, runs, fast=False):
    """Holds one context; answers `entry order` with the median of `runs` calls (5 warm-up calls the first time), `out entry order` with a
    digest of the outputs of one call, on stdout; leaves at end of input."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import torch
    import __graft_entry__ as graft
    pkg = graft.load_package()
    family, scene, flag_names = CONFIGS[config][:3]
    world = CONFIGS[config][3] if len(CONFIGS[config]) > 3 else 1
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
    flags = pkg.RT_FLAG_FAST if fast else 0
    for name in flag_names:
        flags |= getattr(pkg, name)
    n, dev = W * H, "cuda:0"
    if family == "adaptive":
        r = pkg.Renderer(sc, device=0, rank=0, world=world, flags=flags, fmt=getattr(pkg, "RT_FMT_" + CONFIGS[config][4]))
        assert r.streamed_adaptive == ("RT_FLAG_STREAM_ADAPTIVE" in flag_names) and r.stream_cull_adaptive == ("RT_FLAG_STREAM_CULL" in flag_names), config
        assert (world == 1) == (r.local_rows == H)
        return serve(torch, r, {("rt_render", "frame"): (lambda: r.update(), ())}, runs, refined=True)
    if family in ("pixels", "geometry"):
        return pixel_child(pkg, torch, family, sc, flags, flag_names, world, runs)
    r = pkg.Renderer(sc, device=0, flags=flags)
    assert r.streamed_queries == (family != "staged") and r.stream_cull_rays == (family == "culled"), config
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
    serve(torch, r, {(e, o): ((lambda c=c, p=order[o].data_ptr(): c(p)), outs) for e, (c, outs) in calls.items() for o in order}, runs)


def pixel_child(pkg, torch, family, sc, flags, flag_names, world, runs):
    """The calls of one pixel configuration: (entry, which) -> (a call that returns its device ms, its outputs)."""
    dev = "cuda:0"
    if family == "geometry":
        r = pkg.Renderer(sc, device=0, rank=0, world=world, flags=flags, ssaa_threshold=1.0 / 32.0, ssaa_min_cos=0.999)
        assert r.streamed_adaptive == ("RT_FLAG_STREAM_ADAPTIVE" in flag_names) and (world == 1) == (r.local_rows == H)
        return serve(torch, r, {("rt_render", "frame"): (lambda: r.update(), ())}, runs)
    r = pkg.Renderer(sc, device=0, flags=flags)
    assert r.streamed_queries == ("RT_FLAG_STREAM_QUERIES" in flag_names)
    po = torch.zeros((H, W), dtype=torch.int32, device=dev)
    pt = torch.zeros((H, W), dtype=torch.float64, device=dev)
    pn = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    ext = torch.zeros((max(len(r.object_extents()), 1), 5), dtype=torch.int64, device=dev)      # (40-byte records)
    rng = np.random.default_rng(31)
    xy = np.stack([rng.integers(0, W, 4096), rng.integers(0, H, 4096)], axis=1).astype(np.uint32)
    picked = []

    def pick():
        picked[:] = [r.pick(xy)]
        return 0.0
    rect = (W // 2 - 32, H // 2 - 32, W // 2 + 31, H // 2 + 31)
    serve(torch, r, {("rt_render_gbuffer", "planes"): (lambda: r.gbuffer_into(None, po.data_ptr(), pt.data_ptr(), pn.data_ptr()), (po, pt, pn)),
                     ("rt_object_extents", "frame"): (lambda: r.object_extents_into(None, None, ext.data_ptr()), (ext,)),
                     ("rt_object_extents", "64x64"): (lambda: r.object_extents_into(None, rect, ext.data_ptr()), (ext,)),
                     ("rt_pick", "4096px"): (pick, picked)}, runs)


def serve(torch, r, calls, runs, refined=False):
    warm = set()
    print("ready", flush=True)
    for line in sys.stdin:
        words = line.split()
        digest = words[0] == "out"
        key = (words[-2], words[-1])
        call, outputs = calls[key]
        if digest:
            call()
            torch.cuda.synchronize()
            h = hashlib.sha256()
            for o in outputs:
                h.update(o.tobytes() if isinstance(o, np.ndarray) else o.cpu().numpy().tobytes())
            if not outputs:
                h.update(np.ascontiguousarray(r.download()).tobytes())      # (the control and the adaptive frames: the frame)
            if refined:
                h.update(str(int(r.refined)).encode())      # (... and the refined count)
            print(h.hexdigest(), flush=True)
            continue
        if key not in warm:
            for _ in range(WARM):
                call()
            warm.add(key)
        print(repr(float(np.median([call() for _ in range(runs)])) * 1e3), flush=True)
    r.cleanup_update()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--tree", help="a third build in this tree's place (default: the in-tree library)")
    ap.add_argument("--configs", help="comma-separated configuration names (default: all of the families of --only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_kernel_bodies_timings.txt"))
    ap.add_argument("--only", default="staged,streamed,culled")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--runs", type=int, default=31)
    ap.add_argument("--fast", action="store_true", help="RT_FLAG_FAST contexts")
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.runs, args.fast)
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
    for config, cfg in CONFIGS.items():
        family = cfg[0]
        if family not in args.only.split(",") or (args.configs and config not in args.configs.split(",")):
            continue
        procs = []
        try:
            for lib in (args.parent, args.tree):
                env = dict(os.environ)
                env.pop("MI355RT_LIB", None)
                if lib:
                    env["MI355RT_LIB"] = os.path.abspath(lib)
                procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", config, "--runs", str(args.runs)] + (["--fast"] if args.fast else []), env=env, stdin=subprocess.PIPE,
                                              stdout=subprocess.PIPE, text=True))
            for p in procs:
                if p.stdout.readline().strip() != "ready":
                    raise RuntimeError(f"{config}: a child did not start ({p.poll()})")
            if family in ("geometry", "adaptive"):
                series = [("rt_render", "frame")]
            elif family == "pixels":
                series = list(PIXEL_SERIES)
            else:
                series = [(e, o) for o in ("row", "shuffled") for e in ENTRY_POINTS] + ([("rt_render", "row")] if first else [])
                first = False
            for entry, which in series:
                if entry in UNTIMED:
                    same = ask(procs[0], f"out {entry} {which}") == ask(procs[1], f"out {entry} {which}")
                    emit(f"{family:9s}{config:24s}{entry:19s}{which:9s} outputs only: same result {same}")
                    continue
                a, b = [], []
                for _ in range(args.rounds):
                    a.append(float(ask(procs[0], f"{entry} {which}")))
                    b.append(float(ask(procs[1], f"{entry} {which}")))
                same = ask(procs[0], f"out {entry} {which}") == ask(procs[1], f"out {entry} {which}")
                ma, mb, spread = float(np.median(a)), float(np.median(b)), max(a) - min(a)
                verdict = "faster beyond the spread" if ma - mb > spread else ("SLOWER beyond the spread" if mb - ma > spread else "within the spread")
                name = "control: rt_render" if (entry, which) == ("rt_render", "row") else entry
                emit(f"{family:9s}{config:24s}{name:19s}{which:9s} parent {ma:10.1f} [{min(a):10.1f} .. {max(a):10.1f}]  this tree {mb:10.1f} [{min(b):10.1f} .. {max(b):10.1f}]  "
                     f"x {mb / ma:6.4f}  spread {spread:8.1f} ({100.0 * spread / ma:5.2f} %)  {verdict:25s} same result {same}")
        finally:
            for p in procs:
                p.stdin.close()
            for p in procs:
                p.wait(timeout=60)
    return 0


if __name__ == "__main__":
    sys.exit(main())
