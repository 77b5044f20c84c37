"""numpy statement of edge-adaptive supersampling (include/mi355rt.h, RT_FLAG_SSAA_ADAPTIVE), bit for bit.

refine_mask(P, tau): P = [H, W, >=3] float32 plain frame -> bool [H, W].  True where tau < 0, or where some 8-neighbour n inside
the image and some channel c of R, G, B gives !(abs(P[y, x, c] - P[n, c]) <= tau): one float32 subtraction, so NaN differences
refine.  halo = (below, above): optional [W, >=3] rows just outside P (row -1 and row H of a larger image), or None where the image
ends there.
compose(P, S, k, tau, halo=None): the resolve (ssaa_ref.resolve) of the samples S = [k*H, k*W, >=3] where the mask is set, P elsewhere;
alpha 1.0.
"""
import numpy as np

import ssaa_ref


def refine_mask(p, tau, halo=None):
    p = np.asarray(p)[..., :3]
    assert p.dtype == np.float32, p.dtype
    h, w = p.shape[:2]
    tau = np.float32(tau)
    if tau < 0:
        return np.ones((h, w), dtype=bool)
    below, above = halo if halo is not None else (None, None)
    nan = np.full((1, w, 3), np.nan, dtype=np.float32)
    ext = np.concatenate([nan if below is None else np.asarray(below, np.float32)[None, :, :3], p,
                          nan if above is None else np.asarray(above, np.float32)[None, :, :3]], axis=0)
    valid_row = np.array([below is not None] + [True] * h + [above is not None])
    ext = np.concatenate([nan[:, :1].repeat(h + 2, 0), ext, nan[:, :1].repeat(h + 2, 0)], axis=1)   # [h+2, w+2, 3]
    mask = np.zeros((h, w), dtype=bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            n = ext[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            inside = valid_row[1 + dy:1 + dy + h][:, None] & (np.arange(w) + dx >= 0)[None, :] & (np.arange(w) + dx < w)[None, :]
            with np.errstate(invalid="ignore"):
                differs = ~(np.abs(p - n) <= tau)
            mask |= inside & differs.any(axis=-1)
    return mask


def compose(p, s, k, tau, halo=None):
    p = np.asarray(p, dtype=np.float32)
    m = refine_mask(p, tau, halo)
    out = np.empty(p.shape[:2] + (4,), dtype=np.float32)
    out[..., :3] = p[..., :3]
    out[..., 3] = np.float32(1.0)
    if m.any():
        r = ssaa_ref.resolve(np.asarray(s, dtype=np.float32), k)
        out[m] = r[m]
    return out
