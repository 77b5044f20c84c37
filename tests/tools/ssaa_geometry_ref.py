"""numpy statement of the geometric term of adaptive supersampling (include/mi355rt.h, RT_FLAG_SSAA_GEOMETRY), bit for bit.

geo_mask(obj, nrm, min_cos, halo=None): obj = [H, W] int32 primary-hit object (-1: miss), nrm = [H, W, >=3] float32 normals ->
bool [H, W].  True where some 8-neighbour n inside the image has another object, or the same object (>= 0) and
!(dotf(N, N(n)) >= min_cos) with dotf = ((a.x * b.x) + (a.y * b.y)) + (a.z * b.z) in float32, every operation rounded on its own (a
NaN dot product refines).  halo = (below, above): optional (obj [W], nrm [W, >=3]) pairs of the rows just outside the planes (row -1
and row H of a larger image), or None where the image ends there.
compose(p, s, k, tau, obj, nrm, min_cos, halo=None): the resolve (ssaa_ref.resolve) of the samples S where
ssaa_adaptive_ref.refine_mask(P, tau) or geo_mask is set, P elsewhere; alpha 1.0.  halo = (below, above) of (colour row, obj row,
nrm row) triples.
"""
import numpy as np

import ssaa_adaptive_ref
import ssaa_ref


def dotf(a, b):
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        xx = (a[..., 0].astype(f) * b[..., 0].astype(f)).astype(f)
        yy = (a[..., 1].astype(f) * b[..., 1].astype(f)).astype(f)
        zz = (a[..., 2].astype(f) * b[..., 2].astype(f)).astype(f)
        return ((xx + yy).astype(f) + zz).astype(f)


def geo_mask(obj, nrm, min_cos, halo=None):
    obj = np.asarray(obj)
    nrm = np.asarray(nrm)[..., :3]
    assert obj.dtype == np.int32 and nrm.dtype == np.float32, (obj.dtype, nrm.dtype)
    h, w = obj.shape
    c = np.float32(min_cos)
    below, above = halo if halo is not None else (None, None)
    pad_o, pad_n = np.full((1, w), -2, dtype=np.int32), np.zeros((1, w, 3), dtype=np.float32)
    eo = np.concatenate([pad_o if below is None else np.asarray(below[0], np.int32)[None, :], obj,
                         pad_o if above is None else np.asarray(above[0], np.int32)[None, :]], axis=0)
    en = np.concatenate([pad_n if below is None else np.asarray(below[1], np.float32)[None, :, :3], nrm,
                         pad_n if above is None else np.asarray(above[1], np.float32)[None, :, :3]], axis=0)
    valid_row = np.array([below is not None] + [True] * h + [above is not None])
    eo = np.concatenate([np.full((h + 2, 1), -2, np.int32), eo, np.full((h + 2, 1), -2, np.int32)], axis=1)        # [h+2, w+2]
    en = np.concatenate([np.zeros((h + 2, 1, 3), np.float32), en, np.zeros((h + 2, 1, 3), np.float32)], axis=1)
    mask = np.zeros((h, w), dtype=bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            no = eo[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            nn = en[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            inside = valid_row[1 + dy:1 + dy + h][:, None] & (np.arange(w) + dx >= 0)[None, :] & (np.arange(w) + dx < w)[None, :]
            with np.errstate(invalid="ignore"):
                turned = ~(dotf(nrm, nn) >= c)
            mask |= inside & ((no != obj) | ((no == obj) & (obj >= 0) & turned))
    return mask


def compose(p, s, k, tau, obj, nrm, min_cos, halo=None):
    p = np.asarray(p, dtype=np.float32)
    below, above = halo if halo is not None else (None, None)
    colour_halo = None if halo is None else (None if below is None else below[0], None if above is None else above[0])
    geo_halo = None if halo is None else (None if below is None else below[1:3], None if above is None else above[1:3])
    m = ssaa_adaptive_ref.refine_mask(p, tau, colour_halo) | geo_mask(obj, nrm, min_cos, geo_halo)
    out = np.empty(p.shape[:2] + (4,), dtype=np.float32)
    out[..., :3] = p[..., :3]
    out[..., 3] = np.float32(1.0)
    if m.any():
        r = ssaa_ref.resolve(np.asarray(s, dtype=np.float32), k)
        out[m] = r[m]
    return out
