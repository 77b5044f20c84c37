"""Cost of the geometric term of adaptive supersampling (RT_FLAG_SSAA_GEOMETRY).

  python tools/ssaa_geometry_bench.py [--calls N] [--warmup W]
      device us per call (the library's event pair around its kernels; every call synchronised), median of N after W warm-up rounds,
      RGBA32F, k = 4; the calls of one row alternate in one process.  Rows: 20spheres and clebsch at 1080p and 4K, start pose and
      pose 16 of tools/gbuffer_bench.py's orbit.
      tau = -1 (every pixel is refined either way, so the difference is the G pass plus the wider classifier alone):
        (a) an adaptive context, (b) the same with the geometry flag at min_cos = -inf (ids only) and at 0.999 (ids and normals),
        (c) rt_render_gbuffer of the same planes (object; object and normal) on a k = 1 context.
      Condition: (b) - (a) <= 2 x (c) on every row, for both values of min_cos.
      tau = 1/32, for information: the refined share and the frame time without the flag, with it at -inf and at 0.999.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as graft  # noqa: E402
from gbuffer_bench import orbit_pose  # noqa: E402

CONFIGS = [("20spheres", 1920, 1080), ("20spheres", 3840, 2160), ("clebsch", 1920, 1080), ("clebsch", 3840, 2160)]
K = 4
MIN_COS = 0.999


def median_us(calls, n, warmup):
    for _ in range(warmup):
        for c in calls:
            c()
    ms = [[] for _ in calls]
    for _ in range(n):
        for i, c in enumerate(calls):
            ms[i].append(c())
    return [1e3 * float(np.median(m)) for m in ms]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    pkg = graft.load_package()
    ada = pkg.RT_FLAG_SSAA4 | pkg.RT_FLAG_SSAA_ADAPTIVE
    print(f"device us per call, median of {a.calls} synchronised calls after {a.warmup} warm-up rounds, k = {K}, RGBA32F; calls of one row alternate "
          f"in one process; {torch.cuda.get_device_name(0)}")
    print(f"{'scene':<10} {'size':>10} {'pose':>6} | tau=-1: {'(a) ada':>9} {'(b) ids':>9} {'(b) 0.999':>9} {'(c) obj':>8} {'(c) o+n':>8} {'b-a ids':>8} {'b-a nrm':>8} {'<=2c':>5}"
          f" | tau=1/32: {'ada':>9} {'share':>7} {'ids':>9} {'share':>7} {'0.999':>9} {'share':>7}")
    ok = True
    for name, w, h in CONFIGS:
        sc = pkg.Scene.load_from_file(os.path.join(ROOT, "scenes", name + ".yml")).set_size(w, h)
        plain = pkg.Renderer(sc, device=0)
        ra = pkg.Renderer(sc, device=0, flags=ada)
        rg = pkg.Renderer(sc, device=0, flags=ada | pkg.RT_FLAG_SSAA_GEOMETRY)
        rn = pkg.Renderer(sc, device=0, flags=ada | pkg.RT_FLAG_SSAA_GEOMETRY, ssaa_min_cos=MIN_COS)
        po = torch.empty((h, w), dtype=torch.int32, device="cuda:0")
        pn = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        for pose, cam in (("start", None), ("orb16", orbit_pose(pkg, name, 16))):
            for r in (ra, rg, rn):
                r.set_ssaa_threshold(-1.0)
            full = median_us([lambda: ra.update(cam), lambda: rg.update(cam), lambda: rn.update(cam),
                              lambda: plain.gbuffer_into(cam, po.data_ptr(), None, None),
                              lambda: plain.gbuffer_into(cam, po.data_ptr(), None, pn.data_ptr())], a.calls, a.warmup)
            for r in (ra, rg, rn):
                r.set_ssaa_threshold(1.0 / 32.0)
            part = median_us([lambda: ra.update(cam), lambda: rg.update(cam), lambda: rn.update(cam)], a.calls, a.warmup)
            share = [100.0 * r.refined / (w * h) for r in (ra, rg, rn)]
            d_ids, d_nrm = full[1] - full[0], full[2] - full[0]
            row_ok = d_ids <= 2.0 * full[3] and d_nrm <= 2.0 * full[4]
            ok = ok and row_ok
            print(f"{name:<10} {w:>5}x{h:<4} {pose:>6} |         {full[0]:9.1f} {full[1]:9.1f} {full[2]:9.1f} {full[3]:8.1f} {full[4]:8.1f} {d_ids:8.1f} {d_nrm:8.1f} "
                  f"{'yes' if row_ok else 'NO':>5} |           {part[0]:9.1f} {share[0]:6.2f}% {part[1]:9.1f} {share[1]:6.2f}% {part[2]:9.1f} {share[2]:6.2f}%", flush=True)
        for r in (plain, ra, rg, rn):
            r.cleanup_update()
    print("condition ((b) - (a) <= 2 x (c) on every row, ids only and ids + normals):", "holds" if ok else "VIOLATED")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
