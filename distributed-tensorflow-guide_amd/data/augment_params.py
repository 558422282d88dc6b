"""Augmentation parameters, made on the host as integers: ``(x0, y0, cw, ch, flip)`` per sample.

The device never draws anything.  Every draw comes from one counter hash over (seed, epoch, sample index, draw
number), so a sample's row depends on nothing else -- not on the rank, the batch it landed in, or the thread that
produced it -- and the GPU result can be reproduced bit for bit on the CPU from the same table.
"""
import math

import numpy as np

from .sampler import hash32

_TRIES = 10
_FLIP_DRAW = 4 * _TRIES


def _uniform(seed, epoch, indices, draw):
    """float64 in [0, 1): the 32-bit counter hash of (seed, epoch, index, draw) / 2**32."""
    return hash32(seed, epoch, indices, draw).astype(np.float64) / 4294967296.0


def train_params(indices, epoch, seed, H, W, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """Random-resized-crop as usually defined (up to 10 tries of area x log-uniform aspect, then a centre-crop
    fallback) plus a fair flip bit.  indices: the samples' record indices [N] -> int32 [N, 5]."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    n = idx.shape[0]
    out = np.zeros((n, 5), dtype=np.int32)
    done = np.zeros(n, dtype=bool)
    log_r = (math.log(ratio[0]), math.log(ratio[1]))
    for t in range(_TRIES):
        area = H * W * (scale[0] + (scale[1] - scale[0]) * _uniform(seed, epoch, idx, 4 * t))
        aspect = np.exp(log_r[0] + (log_r[1] - log_r[0]) * _uniform(seed, epoch, idx, 4 * t + 1))
        cw = np.rint(np.sqrt(area * aspect)).astype(np.int64)
        ch = np.rint(np.sqrt(area / aspect)).astype(np.int64)
        ok = ~done & (cw >= 1) & (cw <= W) & (ch >= 1) & (ch <= H)
        cwc, chc = np.clip(cw, 1, W), np.clip(ch, 1, H)
        x0 = np.minimum((_uniform(seed, epoch, idx, 4 * t + 2) * (W - cwc + 1)).astype(np.int64), W - cwc)
        y0 = np.minimum((_uniform(seed, epoch, idx, 4 * t + 3) * (H - chc + 1)).astype(np.int64), H - chc)
        for col, v in enumerate((x0, y0, cwc, chc)):
            out[ok, col] = v[ok]
        done |= ok
    if not done.all():  # centre crop at the nearest allowed aspect
        in_ratio = W / H
        if in_ratio < ratio[0]:
            cw, ch = W, min(H, int(round(W / ratio[0])))
        elif in_ratio > ratio[1]:
            cw, ch = min(W, int(round(H * ratio[1]))), H
        else:
            cw, ch = W, H
        out[~done, :4] = ((W - cw) // 2, (H - ch) // 2, cw, ch)
    out[:, 4] = (hash32(seed, epoch, idx, _FLIP_DRAW) >> np.uint64(31)).astype(np.int32)
    return out


def eval_params(n, H, W, crop=0.875):
    """The centre box of ``crop`` x the image, no flip: int32 [n, 5]."""
    cw, ch = max(1, int(round(W * crop))), max(1, int(round(H * crop)))
    row = np.array([(W - cw) // 2, (H - ch) // 2, cw, ch, 0], dtype=np.int32)
    return np.tile(row, (n, 1))


def validate_params(p, H, W):
    """Raise ValueError unless every box lies inside the H x W image with cw, ch >= 1 and flip in {0, 1}."""
    p = np.asarray(p)
    if p.ndim != 2 or p.shape[1] != 5 or p.dtype != np.int32:
        raise ValueError("params must be int32 [N, 5], got %s %s" % (p.dtype, p.shape))
    q = p.astype(np.int64)
    x0, y0, cw, ch, flip = (q[:, i] for i in range(5))
    bad = (x0 < 0) | (y0 < 0) | (cw < 1) | (ch < 1) | (x0 + cw > W) | (y0 + ch > H) | (flip < 0) | (flip > 1)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError("params row %d = %s does not lie inside a %d x %d image" % (i, p[i].tolist(), H, W))
