#!/usr/bin/env python3
"""Host lab behind RT_FLAG_STREAM_CULL_PIXELS.  No GPU.
The culled pixel queries ask sphere_in_cone (csrc/rt_wavefront_math.hpp) about the chunk bounds of an RT_FLAG_STREAM_CULL context, one
verdict per (8 x 8 block, chunk).  Here: that predicate restated in numpy, the cones of a frame's blocks (cull_lab's frame records: the
axis through lane 36, the opening from the four corner lanes), the bounds by the library's own host functions (stream_cull_lab.image),
and the count the GPU statistics test is held to.
usage: python tests/tools/pixel_cull_lab.py      prints the counts of the statistics scene"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOOLS = os.path.join(ROOT, "tests", "tools")
sys.path.insert(0, ROOT)
sys.path.insert(0, TOOLS)
import cull_lab as L  # noqa: E402
import stream_cull_lab as SC  # noqa: E402


def sphere_in_cone(k, r, inv_r, org, axis, cos_t):
    """sphere_in_cone, operation for operation in float64 (numpy contracts nothing): k [n, 3], r, inv_r, cos_t [n], org, axis [n, 3].
    True = the sphere may reach into the cone."""
    with np.errstate(invalid="ignore", over="ignore"):
        cc = -0.5 * k
        v = cc - org
        vv = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
        h = v[:, 0] * axis[:, 0] + v[:, 1] * axis[:, 1] + v[:, 2] * axis[:, 2]
        rho2 = vv - h * h
        rho2 = np.where(rho2 > 0.0, rho2, 0.0)
        v1 = np.abs(v[:, 0]) + np.abs(v[:, 1]) + np.abs(v[:, 2])
        s2 = cc[:, 0] * cc[:, 0] + cc[:, 1] * cc[:, 1] + cc[:, 2] * cc[:, 2] + org[:, 0] * org[:, 0] + org[:, 1] * org[:, 1] + org[:, 2] * org[:, 2]
        c = cos_t * (1.0 - 1e-9)
        sin2 = 1.0 - c * c
        sin2 = np.where(sin2 > 0.0, sin2, 0.0)
        sn = np.sqrt(sin2)
        lim = r + 1e-6 * (v1 + r + 1.0) + 1e-12 * (s2 + 1.0) * inv_r
        rhs = lim + h * sn
        rel = ~(rhs < 0.0) & ~(rho2 * c * c > rhs * rhs)
    return np.where(~(r < np.inf) | ~(cos_t > 0.2), True, rel)


def block_cones(osc):
    """(origin, axis, cos_t) of every 8 x 8 block of the oracle scene's frame under the identity camera, in block order (row-major):
    [n_blocks, 3], [n_blocks, 3], [n_blocks]."""
    n_blocks, n_o = ((osc.width + 7) // 8) * ((osc.height + 7) // 8), len(osc.objects)
    rec, _ = L.frame(osc, stride=1 << 30).get("cone")
    assert len(rec) == n_blocks * n_o
    one = rec.reshape(n_blocks, n_o, L.REC["cone"])
    assert (one[:, :, 5:12] == one[:, :1, 5:12]).all()      # one cone per block
    return one[:, 0, 5:8].copy(), one[:, 0, 8:11].copy(), one[:, 0, 11].copy()


def verdicts(pkg, sc):
    """[n_blocks, n_chunks] bool: the block's cone reaches the chunk's bound (the chunk is staged).  Both by the numpy restatement and by
    the predicate itself, compiled for the host (cull_lab.evaluate): they must agree."""
    import stream_scenes as S
    osc = S.oracle_of(pkg, sc)
    org, axis, cos_t = block_cones(osc)
    _, bounds, w = SC.image(sc.arrays())
    b = bounds.view(SC.US_DTYPE)
    nb, nc = len(org), len(b)
    assert nc == w["n_chunks"]
    rec = np.zeros((nb, nc, L.REC["cone"]))
    rec[:, :, 0:3], rec[:, :, 3], rec[:, :, 4] = b["k"][None], b["r"][None], b["inv_r"][None]
    rec[:, :, 5:8], rec[:, :, 8:11], rec[:, :, 11] = org[:, None], axis[:, None], cos_t[:, None]
    flat = rec.reshape(-1, L.REC["cone"])
    mine = sphere_in_cone(flat[:, 0:3], flat[:, 3], flat[:, 4], flat[:, 5:8], flat[:, 8:11], flat[:, 11])
    theirs = L.evaluate("cone", flat) != 0
    assert np.array_equal(mine, theirs), int((mine != theirs).sum())
    return mine.reshape(nb, nc)


def expectation(pkg, sc):
    """dict(blocks, n_chunks, D = blocks x chunks, staged, skipped) for one rt_render_gbuffer of the scene's frame."""
    v = verdicts(pkg, sc)
    return dict(blocks=v.shape[0], n_chunks=v.shape[1], D=int(v.size), staged=int(v.sum()), skipped=int((~v).sum()))


def main():
    import __graft_entry__ as g
    import bounce_cull_lab as BL
    pkg = g.load_package()
    for name, sc in (("stream_cull_lab.cluster_scene", SC.cluster_scene(pkg)), ("bounce_cull_lab.bounce_scene", BL.bounce_scene(pkg))):
        print(name, expectation(pkg, sc))


if __name__ == "__main__":
    main()
