"""Score a BERT pre-training checkpoint on a held-out token set: masked-LM loss and top-k accuracy, next-sentence loss
and accuracy.

Every rank restores the latest checkpoint of ``--ckpt_dir`` (the TensorBundle bert_train.py writes), reads its slice of
every global batch of ``--data_dir`` (tools/make_shards.py) -- every record exactly once over the ranks, masked by the
evaluation seed at epoch 0, so every evaluation of a set sees the same masks -- and runs the model's
``pretraining_logits``; ``dtg.train.BertEvaluator`` scores each batch with the metric kernels on the device,
all-reduces one fp64 accumulator and reads it once.  The chief prints one line,

    eval step N: n=... mlm_n=... mlm_loss=... mlm_top1=... mlm_top5=... nsp_loss=... nsp_acc=...

the same line bert_train.py's ``--eval_dir`` hook prints for that checkpoint.  Exit status 1 when ``--ckpt_dir`` holds
no checkpoint.

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 bert_eval.py \\
        --ckpt_dir /path/to/ckpt --data_dir /path/to/val [--batch 256] [--tiny] [--topk 1 5]
"""
import argparse
import sys

import _path  # noqa: F401

import torch

import dtg
from dtg.data import TokenLoader, masking_args, read_token_meta
from dtg.models import bert
from dtg.parallel import FlatParams, comm
from dtg.train.evaluation import format_bert_result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt_dir", required=True)
    ap.add_argument("--data_dir", required=True, help="directory of *.dtgrec token shards")
    ap.add_argument("--batch", type=int, default=256, help="per-GPU sequences")
    ap.add_argument("--tiny", action="store_true", help="2-layer, 64-wide BERT (CPU tests)")
    ap.add_argument("--topk", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--max_predictions", type=int, default=20)
    ap.add_argument("--loader_depth", type=int, default=3)
    ap.add_argument("--unpad", action="store_true", help="run the encoder on packed token rows (dtg.ops.seqpack)")
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
        cfg = bert.BertConfig.tiny() if a.tiny else bert.BertConfig.base()
        model = bert.BertForPreTraining(cfg).to(device)
        dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
        flat = FlatParams(model, compute_dtype=dtype)
        step = dtg.train.restore_flat(flat, prefix)
        with TokenLoader(a.data_dir, a.batch, device, world=world, rank=rank, train=False, drop_last=False,
                         depth=a.loader_depth, P=a.max_predictions, pack=a.unpad,
                         **masking_args(read_token_meta(a.data_dir))) as loader:
            res = dtg.train.BertEvaluator(model, loader, ks=a.topk, unpad=a.unpad).run()
        if is_chief:
            print(format_bert_result(-1 if step is None else step, res, tuple(a.topk)), flush=True)
            print("evaluated %s: %d sequences in %.2f s (%.1f sequences/s), nonfinite rows %d" % (
                prefix, res["n"], res["seconds"], res["sequences_per_sec"], res["nonfinite"]), flush=True)
    comm.barrier()
    comm.shutdown()
    return status


if __name__ == "__main__":
    sys.exit(main())
