"""The object extents' reference statement (include/mi355rt.h, "Object extents"): the G-buffer composer's object and t planes
(tests/tools/gbuffer_ref.py) reduced per object with numpy -- test infrastructure.

Record i describes the pixels (x, y) of `rect` (x0, y0, x1, y1 inclusive; None = the whole frame) in the global rows `rows` (None = all)
whose object is i: their number, the minima and maxima of x and y, the minimum and maximum of t.  An object without such a pixel keeps
the identities: pixels 0, x_min = y_min = 0xFFFFFFFF, x_max = y_max = 0, t_min +inf, t_max +0.0."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gbuffer_ref  # noqa: E402

DTYPE = np.dtype([("pixels", np.uint64), ("x_min", np.uint32), ("y_min", np.uint32), ("x_max", np.uint32), ("y_max", np.uint32),
                  ("t_min", np.float64), ("t_max", np.float64)])


def identity(n):
    out = np.zeros(n, dtype=DTYPE)
    out["x_min"] = out["y_min"] = 0xFFFFFFFF
    out["t_min"] = np.inf
    return out


def reduce_planes(obj, t, n_objects, xs, ys, rect=None):
    """Records from the planes obj / t [R, C] whose columns are the global x coordinates `xs` and whose rows are the global rows `ys`."""
    obj, t, xs, ys = np.asarray(obj), np.asarray(t), np.asarray(xs, dtype=np.int64), np.asarray(ys, dtype=np.int64)
    assert obj.shape == t.shape == (len(ys), len(xs))
    x = np.broadcast_to(xs[None, :], obj.shape)
    y = np.broadcast_to(ys[:, None], obj.shape)
    inside = np.ones(obj.shape, dtype=bool)
    if rect is not None:
        x0, y0, x1, y1 = (int(v) for v in rect)
        inside = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    out = identity(n_objects)
    for i in np.unique(obj[inside & (obj >= 0)]).tolist():
        m = inside & (obj == i)
        out[i] = (int(m.sum()), x[m].min(), y[m].min(), x[m].max(), y[m].max(), t[m].min(), t[m].max())
    return out


def compose(osc, cam=None, rect=None, rows=None):
    """Records of the oracle scene `osc`: gbuffer_ref.compose over the rows and columns of the rectangle, reduced."""
    rows = np.arange(osc.height) if rows is None else np.asarray(rows, dtype=np.int64)
    cols = np.arange(osc.width)
    if rect is not None:
        rows = rows[(rows >= rect[1]) & (rows <= rect[3])]
        cols = cols[(cols >= rect[0]) & (cols <= rect[2])]
    n = len(osc.objects)
    if len(rows) == 0:
        return identity(n)
    ref = gbuffer_ref.compose(osc, cam, rows=rows, cols=cols)
    return reduce_planes(ref["object"], ref["t"], n, cols, rows, None)


def merge(a, b):
    """Records of two ranks (or two disjoint pixel sets) merged: sum / min / max, no special case."""
    out = a.copy()
    out["pixels"] = a["pixels"] + b["pixels"]
    for f in ("x_min", "y_min", "t_min"):
        out[f] = np.minimum(a[f], b[f])
    for f in ("x_max", "y_max", "t_max"):
        out[f] = np.maximum(a[f], b[f])
    return out


def same(a, b):
    """Equal on all bits (t_min / t_max as uint64)."""
    return a.dtype == b.dtype == DTYPE and a.shape == b.shape and a.tobytes() == b.tobytes()


def sphere_field(pkg, n, seed, w=64, h=48):
    """n small spheres spread over the view of a w x h frame (vertical field of view 50 degrees, camera at the origin looking along +z):
    about one and a half pixels across each, at depths 20 .. 30, so that a good share of them owns a pixel and hardly any hides another."""
    rng = np.random.default_rng(seed)
    sc = pkg.Scene.new(w, h, 50.0, 0, (0.0, 0.0, 0.0))
    tan = np.tan(np.radians(25.0))
    for _ in range(n):
        z = rng.uniform(20.0, 30.0)
        half_h, half_w = z * tan, z * tan * w / h
        c = (rng.uniform(-half_w, half_w) * 0.98, rng.uniform(-half_h, half_h) * 0.98, z)
        sc.add_object(pkg.surface_make("sphere", c, [0.8 * 2.0 * z * tan / h]), (0.8, 0.8, 0.8))
    sc.add_light("directional", [0.0, -1.0, 0.5])
    return sc
