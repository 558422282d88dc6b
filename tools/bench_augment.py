#!/usr/bin/env python3
"""crop_resize_norm (csrc/kernels/augment.hip) against a batched PyTorch equivalent, on one GPU.

Device events around ``--launches`` back-to-back calls, every shape warmed, ``--rounds`` rounds alternating the two
paths on the same inputs.  The PyTorch path is what one would assemble from framework ops without a per-image loop:
``F.affine_grid`` + ``F.grid_sample`` (bilinear) on a float copy of the batch, normalize, cast to bf16
channels_last.  It is an equivalent, not a mirror: its weights are fp32, not 8.8 fixed point.

Reported: time per call, algorithmic bytes (source bytes inside the crop boxes + output bytes) over time, that rate
next to the HBM copy rate of profiles/r05_hbm_probe, and the number of ATen ops the PyTorch path dispatches (each is
at least one launch).

    python tools/bench_augment.py [--n 1024 --size 256 --out_size 224] [--json FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dtg  # noqa: E402,F401
from dtg.data import train_params  # noqa: E402
from dtg.ops.augment import IMAGENET_MEAN, IMAGENET_STD, crop_resize_norm, norm_constants  # noqa: E402

HBM_COPY_TBS = 5.28  # profiles/r05_hbm_probe: read + written bytes of a large copy over its time


def torch_path(raw, theta, S, mean, std):
    x = raw.permute(0, 3, 1, 2).float()
    grid = F.affine_grid(theta, (raw.shape[0], 3, S, S), align_corners=False)
    y = F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False)
    y = (y - mean) / std
    return y.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def box_theta(params, H, W, device):
    """(x0, y0, cw, ch, flip) -> the [N, 2, 3] affine maps of affine_grid's normalized coordinates."""
    p = params.astype(np.float64)
    x0, y0, cw, ch, flip = p.T
    t = np.zeros((len(p), 2, 3))
    t[:, 0, 0] = np.where(flip > 0, -1.0, 1.0) * cw / W
    t[:, 0, 2] = (2 * x0 + cw) / W - 1
    t[:, 1, 1] = ch / H
    t[:, 1, 2] = (2 * y0 + ch) / H - 1
    return torch.tensor(t, dtype=torch.float32, device=device)


def count_ops(fn):
    from torch.utils._python_dispatch import TorchDispatchMode

    class Counter(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Counter.n += 1
            return func(*args, **(kwargs or {}))

    with Counter():
        fn()
    return Counter.n


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches  # ms per call


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out_size", type=int, default=224)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures on a GPU; none is available")
    dev = torch.device("cuda", 0)
    N, H, S = a.n, a.size, a.out_size
    g = torch.Generator().manual_seed(0)
    raw = torch.randint(0, 256, (N, H, H, 3), dtype=torch.uint8, generator=g).to(dev)
    p = train_params(np.arange(N), 0, 0, H, H)
    params = torch.from_numpy(p).to(dev)
    scale, shift = (t.to(dev) for t in norm_constants())
    theta = box_theta(p, H, H, dev)
    mean = torch.tensor(IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=dev).view(1, 3, 1, 1)
    out = torch.empty((N, 3, S, S), dtype=torch.bfloat16, device=dev).contiguous(memory_format=torch.channels_last)

    def ours():
        crop_resize_norm(raw, params, S, scale, shift, out=out)

    def theirs():
        torch_path(raw, theta, S, mean, std)

    src_bytes = int((p[:, 2].astype(np.int64) * p[:, 3] * 3).sum())
    out_bytes = N * S * S * 3 * 2
    # the two paths agree up to the fixed-point weights and bf16 (reported, not asserted: they are not mirrors)
    ours()
    diff = (out.float() - torch_path(raw, theta, S, mean, std).float()).abs()
    ops = count_ops(theirs)
    for fn in (ours, theirs):  # warm every shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rows = []
    for r in range(a.rounds):
        t_ours, t_theirs = timed(ours, a.launches), timed(theirs, a.launches)
        rows.append({"round": r, "hip_ms": t_ours, "torch_ms": t_theirs})
        print("round %d: crop_resize_norm %.4f ms, PyTorch path %.4f ms" % (r, t_ours, t_theirs), flush=True)
    hip = np.array([x["hip_ms"] for x in rows])
    tor = np.array([x["torch_ms"] for x in rows])
    rate = (src_bytes + out_bytes) / (np.median(hip) * 1e-3) / 1e12
    res = {"n": N, "size": H, "out_size": S, "launches": a.launches, "rounds": rows,
           "hip_ms_median": float(np.median(hip)), "hip_ms_min": float(hip.min()), "hip_ms_max": float(hip.max()),
           "torch_ms_median": float(np.median(tor)), "torch_ms_min": float(tor.min()), "torch_ms_max": float(tor.max()),
           "source_bytes_in_boxes": src_bytes, "output_bytes": out_bytes, "algorithmic_TBps": float(rate),
           "share_of_hbm_copy_rate": float(rate / HBM_COPY_TBS), "hbm_copy_TBps": HBM_COPY_TBS,
           "torch_path_aten_ops": ops, "hip_launches": 1,
           "max_abs_diff_vs_torch_path": float(diff.max()), "mean_abs_diff_vs_torch_path": float(diff.mean())}
    print("crop_resize_norm: median %.4f ms [%.4f, %.4f]; %.1f MB in boxes + %.1f MB out = %.3f TB/s algorithmic, "
          "%.0f%% of the %.2f TB/s HBM copy rate (the bound that applies: the kernel moves bytes, it has no reuse)"
          % (res["hip_ms_median"], res["hip_ms_min"], res["hip_ms_max"], src_bytes / 1e6, out_bytes / 1e6, rate,
             100 * rate / HBM_COPY_TBS, HBM_COPY_TBS))
    print("PyTorch path: median %.4f ms [%.4f, %.4f], %d ATen ops per batch; crop_resize_norm is %.1fx faster"
          % (res["torch_ms_median"], res["torch_ms_min"], res["torch_ms_max"], ops,
             res["torch_ms_median"] / res["hip_ms_median"]))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
