"""numpy statement of the supersampling resolve (include/mi355rt.h, RT_FLAG_SSAA2 / RT_FLAG_SSAA4), bit for bit.

resolve(S, k): S = [k*rows, k*W, C] float32 samples (C = 3 or 4, row 0 = bottom) -> [rows, W, 4] float32.  Sub-pixel (i, j) of output
pixel (x, y) is S[k*y + j, k*x + i]; per channel every sub-row is summed as a pairwise tree over i (k = 2: s0 + s1; k = 4:
(s0 + s1) + (s2 + s3)), the sub-row sums by the same tree over j, the sum multiplied by 1/k^2; alpha 1.0.  Every operation is one
float32 operation (numpy rounds each one), so there is nothing to contract.
quantise(v): the render kernels' RGBA8 store, (unsigned char)(int)(v * 255.0f + 0.5f), alpha 255.
"""
import numpy as np


def _tree(parts):
    """Pairwise float32 sum of 2 or 4 arrays in the contract's order."""
    if len(parts) == 2:
        return parts[0] + parts[1]
    if len(parts) == 4:
        return (parts[0] + parts[1]) + (parts[2] + parts[3])
    raise ValueError(f"supersampling factor {len(parts)}: only 2 and 4 are defined")


def resolve(samples, k):
    s = np.asarray(samples)
    assert s.dtype == np.float32, s.dtype
    kh, kw = s.shape[0], s.shape[1]
    assert kh % k == 0 and kw % k == 0, (s.shape, k)
    a = s[..., :3].reshape(kh // k, k, kw // k, k, 3)          # [y, j, x, i, c]
    rows = [_tree([a[:, j, :, i, :] for i in range(k)]) for j in range(k)]
    avg = _tree(rows) * np.float32(1.0 / (k * k))
    out = np.empty((kh // k, kw // k, 4), dtype=np.float32)
    out[..., :3] = avg
    out[..., 3] = np.float32(1.0)
    return out


def quantise(img):
    """float32 [..., >=3] -> uint8 [..., 4] exactly as the kernels store RGBA8 (truncating conversion of v * 255 + 0.5)."""
    v = np.asarray(img, dtype=np.float32)[..., :3]
    t = v * np.float32(255.0) + np.float32(0.5)
    q = np.empty(v.shape[:-1] + (4,), dtype=np.uint8)
    q[..., :3] = t.astype(np.int32).astype(np.uint8)   # (int) truncates towards zero; (unsigned char) keeps the low 8 bits
    q[..., 3] = 255
    return q


def resolve_rgba8(samples, k):
    return quantise(resolve(samples, k))
