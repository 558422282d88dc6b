"""Random-resized-crop + flip + normalize + cast, one launch per batch (csrc/kernels/augment.hip).

``crop_resize_norm(raw u8 [N,H,W,3], params i32 [N,5], S, scale f32 [3], shift f32 [3])`` returns the bf16
``[N, 3, S, S]`` channels_last tensor the models take.  The arithmetic is specified in integers (8.8 fixed-point
bilinear weights from a 16.16 source step) up to two separately rounded fp32 operations, so the kernel and
``crop_resize_norm_ref`` -- the same formulas in torch int64 -- agree bit for bit; CPU tensors take the mirror.
"""
import numpy as np
import torch

from ._native import lib

MAX_SIDE = 8192  # H, W <= this: the coordinate arithmetic stays in 32 bits

IMAGENET_MEAN = (0.485 * 255.0, 0.456 * 255.0, 0.406 * 255.0)  # on the 0..255 scale of the stored pixels
IMAGENET_STD = (0.229 * 255.0, 0.224 * 255.0, 0.225 * 255.0)


def norm_constants(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """(scale, shift) fp32 CPU tensors [3]: ``out = p * scale + shift`` with p the bilinear sum carrying 2**16, so
    ``scale = 1 / (65536 * std)`` and ``shift = -mean / std``; computed once in fp32 and handed to both
    implementations."""
    m, s = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    if m.shape != (3,) or s.shape != (3,) or not (s > 0).all():
        raise ValueError("mean and std must be 3 values, std > 0")
    scale = np.float32(1.0) / (np.float32(65536.0) * s)
    shift = -m / s
    return torch.from_numpy(scale.astype(np.float32)), torch.from_numpy(shift.astype(np.float32))


def _check(raw, params, S):
    if raw.dtype != torch.uint8 or raw.dim() != 4 or raw.shape[3] != 3:
        raise ValueError("raw must be uint8 [N, H, W, 3], got %s %s" % (raw.dtype, tuple(raw.shape)))
    N, H, W = raw.shape[:3]
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE and 1 <= S <= MAX_SIDE):
        raise ValueError("1 <= H, W, S <= %d required" % MAX_SIDE)
    if params.dtype != torch.int32 or tuple(params.shape) != (N, 5):
        raise ValueError("params must be int32 [%d, 5], got %s %s" % (N, params.dtype, tuple(params.shape)))
    if params.device.type == "cpu":  # a device table was validated where it was made (the loader); no sync here
        from ..data.augment_params import validate_params
        validate_params(params.numpy(), H, W)
    return N, H, W


def _axis(o, c, S):
    """Output coordinates o [.., S] and crop extents c [.., 1] (int64) -> (i, i1, f): the two taps and the weight."""
    step = (c << 16) // S
    u = torch.minimum(torch.clamp(o * step + (step >> 1) - 32768, min=0), (c - 1) << 16)
    i = u >> 16
    return i, torch.minimum(i + 1, c - 1), (u >> 8) & 255


def crop_resize_norm_ref(raw, params, S, scale, shift):
    """The mirror: integer formulas in torch int64, then ``.to(float32) * scale + shift`` as two eager ops, then
    ``.to(bfloat16)``.  Runs on the device of ``raw``."""
    N, H, W = _check(raw, params, S)
    dev = raw.device
    p = params.to(device=dev, dtype=torch.int64)
    x0 = p[:, 0].clamp(0, W - 1).view(N, 1)
    y0 = p[:, 1].clamp(0, H - 1).view(N, 1)
    cw = torch.minimum(p[:, 2].clamp(min=1).view(N, 1), W - x0)
    ch = torch.minimum(p[:, 3].clamp(min=1).view(N, 1), H - y0)
    flip = (p[:, 4] != 0).view(N, 1)
    o = torch.arange(S, device=dev, dtype=torch.int64).view(1, S)
    ix, ix1, fx = _axis(torch.where(flip, S - 1 - o, o), cw, S)
    iy, iy1, fy = _axis(o.expand(N, S), ch, S)
    img = raw.to(torch.int64)
    n = torch.arange(N, device=dev).view(N, 1, 1)

    def tap(yy, xx):  # [N, S] rows, [N, S] columns -> [N, S, S, 3]
        return img[n, (y0 + yy).view(N, S, 1), (x0 + xx).view(N, 1, S)]

    fx, fy = fx.view(N, 1, S, 1), fy.view(N, S, 1, 1)
    top = tap(iy, ix) * (256 - fx) + tap(iy, ix1) * fx
    bot = tap(iy1, ix) * (256 - fx) + tap(iy1, ix1) * fx
    acc = top * (256 - fy) + bot * fy
    y = acc.to(torch.float32) * scale.to(dev).view(1, 1, 1, 3)
    y = y + shift.to(dev).view(1, 1, 1, 3)
    return y.to(torch.bfloat16).permute(0, 3, 1, 2)  # [N, 3, S, S] over NHWC storage = channels_last


def crop_resize_norm(raw, params, S, scale, shift, out=None, _grid=None):
    """GPU tensors go through the HIP kernel (a missing extension is an error), CPU tensors through the mirror.

    out: optional bf16 destination, either ``[N, 3, S, S]`` channels_last or its NHWC view ``[N, S, S, 3]``
    (contiguous; may be a view into a larger buffer).  _grid: tests only -- force the workgroup count so that the
    kernel's grid-stride loop repeats at small sizes."""
    N, H, W = _check(raw, params, S)
    if out is not None:
        if out.dtype != torch.bfloat16 or out.device != raw.device:
            raise ValueError("out must be a bf16 tensor on raw's device")
        if tuple(out.shape) == (N, 3, S, S) and out.permute(0, 2, 3, 1).is_contiguous():
            nhwc = out.permute(0, 2, 3, 1)
        elif tuple(out.shape) == (N, S, S, 3) and out.is_contiguous():
            nhwc = out
        else:
            raise ValueError("out must be [N, 3, S, S] channels_last or contiguous [N, S, S, 3]")
    if not raw.is_cuda:
        y = crop_resize_norm_ref(raw, params, S, scale, shift)
        if out is None:
            return y
        nhwc.copy_(y.permute(0, 2, 3, 1))
        return out
    dev = raw.device
    if out is None:
        out = torch.empty((N, 3, S, S), dtype=torch.bfloat16, device=dev).contiguous(memory_format=torch.channels_last)
        nhwc = out.permute(0, 2, 3, 1)
    lib().crop_resize_norm(raw.contiguous(), params.to(dev).contiguous(), nhwc, scale.to(dev), shift.to(dev),
                           int(_grid or 0))
    return out
