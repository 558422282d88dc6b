"""Score a ResNet-50 checkpoint on a held-out record set: top-k accuracy and the mean cross-entropy.

Every rank restores the latest checkpoint of ``--ckpt_dir`` (the TensorBundle resnet50_train.py writes), reads its
slice of every global batch of ``--data_dir`` (tools/make_shards.py) -- every record exactly once over the ranks, the
centre box, no flip -- and runs the model in eval mode; ``dtg.train.Evaluator`` scores each batch with the metric
kernels on the device, all-reduces one fp64 accumulator and reads it once.  The chief prints one line,

    eval step N: n=... loss=... top1=... top5=...

the same line resnet50_train.py's ``--eval_dir`` hook prints for that checkpoint.  Exit status 1 when ``--ckpt_dir``
holds no checkpoint.

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 resnet50_eval.py \\
        --ckpt_dir /path/to/ckpt --data_dir /path/to/val [--batch 256] [--image 224] [--tiny] [--topk 1 5]
"""
import argparse
import sys

import _path  # noqa: F401

import torch

import dtg
from dtg.data import DeviceLoader
from dtg.models import resnet
from dtg.parallel import FlatParams, comm
from dtg.train.evaluation import format_result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt_dir", required=True)
    ap.add_argument("--data_dir", required=True, help="directory of *.dtgrec record shards")
    ap.add_argument("--batch", type=int, default=256, help="per-GPU batch")
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--tiny", action="store_true", help="4-block narrow ResNet on 32x32 images (CPU tests)")
    ap.add_argument("--topk", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--loader_depth", type=int, default=3)
    a, _ = ap.parse_known_args()
    rank, _, world, device = comm.init()
    is_chief = rank == 0
    status = 0
    prefix = dtg.train.latest_checkpoint(a.ckpt_dir)
    if prefix is None:
        if is_chief:
            print("no checkpoint in %s" % a.ckpt_dir, file=sys.stderr, flush=True)
        status = 1
    else:
        model = (resnet.resnet18_like_tiny(10) if a.tiny else resnet.resnet50()).to(device)
        model = model.to(memory_format=torch.channels_last)
        dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
        flat = FlatParams(model, compute_dtype=dtype)
        step = dtg.train.restore_flat(flat, prefix)
        with DeviceLoader(a.data_dir, a.batch, 32 if a.tiny else a.image, device, world=world, rank=rank, train=False,
                          drop_last=False, depth=a.loader_depth, dtype=dtype) as loader:
            res = dtg.train.Evaluator(model, loader, ks=a.topk).run()
        if is_chief:
            print(format_result(-1 if step is None else step, res, tuple(a.topk)), flush=True)
            print("evaluated %s: %d records in %.2f s (%.1f images/s), nonfinite rows %d" % (
                prefix, res["n"], res["seconds"], res["images_per_sec"], res["nonfinite"]), flush=True)
    comm.barrier()
    comm.shutdown()
    return status


if __name__ == "__main__":
    sys.exit(main())
