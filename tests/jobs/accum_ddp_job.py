#!/usr/bin/env python3
"""Gradient accumulation through DataParallel's bucket path on one GPU rank (tests/test_grad_accum_gpu.py starts it
with DTG_DDP_FORCE=1 on a one-rank RCCL group, where the hooks are live and every bucket's all-reduce is enqueued
from the side stream):

1. tiny BERT, A = 3, at least three buckets: after ``dp.finish()`` the flat gradient is bf16(sum_i float(g_i)) of the
   micro-gradients cloned after each backward, bit for bit -- a bucket unfolded before its last gradient landed, or
   after its collective read it, would break this;
2. a Linear stack (its backward has no float atomics, so two runs give the same bits), FusedLAMB with clip_norm: two
   windows of ``dp.step(opt)`` are bit-equal to the same windows without DataParallel.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    import torch
    import dtg  # noqa: F401
    from dtg import ops
    from dtg.models import bert
    from dtg.models.layers import Linear
    from dtg.optim import FusedLAMB
    from dtg.parallel import DataParallel, FlatParams, GradAccumulator, comm, overlap

    rank, _, world, dev = comm.init()
    assert dev.type == "cuda" and world == 1 and os.environ.get("DTG_DDP_FORCE") == "1"
    ops.lib()

    def same_bits(a, b):
        iv = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
        nan = torch.isnan(b)
        return a.dtype == b.dtype and torch.equal(torch.isnan(a), nan) and torch.equal(a.view(iv)[~nan], b.view(iv)[~nan])

    # ---- 1. the flat gradient after finish() --------------------------------------------------------------------
    A = 3
    cfg = bert.BertConfig.tiny()
    torch.manual_seed(3)
    model = bert.BertForPreTraining(cfg).to(dev)
    model.train()
    flat = FlatParams(model)
    groups = list(flat)
    dp = DataParallel(flat, bucket_mb=0.05)
    assert dp.overlap and len(dp.buckets) >= 3, len(dp.buckets)
    acc = GradAccumulator(flat, A, dp)
    opt = FusedLAMB(flat, lr=1e-3, clip_norm=1.0)
    # the micro-steps 0 .. A-2 are cloned after their backward, before the fold.  The last one's buckets are unfolded
    # from inside its backward, so each bucket's own input (final when the bucket fires) is cloned on the launching
    # stream right before the accumulator is added onto it
    unfold = dp._pre_launch
    last = {}

    def record_then_unfold(bk):
        last[bk.index] = bk.view().clone()
        unfold(bk)
    dp._pre_launch = record_then_unfold
    for window in range(2):
        b = bert.synthetic_batch(4 * A, 64, cfg, dev, max_predictions=8, seed=window)
        clones = []
        last.clear()
        for i in range(A):
            acc.begin()
            model(*[t[4 * i:4 * (i + 1)] for t in b]).backward()
            if i < A - 1:
                assert all(bk.work is None for bk in dp.buckets) and not last, "a collective before the last micro-step"
                overlap.join()
                clones.append([g.grad.clone() for g in flat])
            acc.end()
        launched = len(last)
        dp.finish()
        torch.cuda.synchronize()
        assert sorted(last) == list(range(len(dp.buckets)))
        for bk in dp.buckets:
            j = groups.index(bk.group)
            s = clones[0][j][bk.start:bk.end].float()
            for c in clones[1:]:
                s = s + c[j][bk.start:bk.end].float()
            s = s + last[bk.index].float()
            assert same_bits(bk.view(), s.to(bk.group.grad.dtype)), ("bucket", window, bk.index, bk.group.name)
        print("window %d: buckets=%d launched_in_backward=%d" % (window, len(dp.buckets), launched), flush=True)
        assert launched > 0, "no bucket was launched from inside the backward"
        opt.step(grad_scale=dp.grad_scale / A)  # the apply zeroes the gradient; the window is closed by hand
        acc.reset()
    dp._pre_launch = None
    dp.remove_hooks()

    # ---- 2. dp.step(opt) windows == the same windows without DataParallel -------------------------------------------
    def run(with_dp):
        torch.manual_seed(4)
        m = torch.nn.Sequential(Linear(64, 128, act="relu"), Linear(128, 128, act="relu"), Linear(128, 16)).to(dev)
        m.train()
        fl = FlatParams(m)
        d = DataParallel(fl, bucket_mb=0.001) if with_dp else None
        if d is not None:
            assert d.overlap and len(d.buckets) >= 3
        ga = GradAccumulator(fl, A, d)
        o = FusedLAMB(fl, lr=1e-2, clip_norm=0.5)
        for window in range(2):
            g = torch.Generator().manual_seed(window)
            x = torch.randn(8 * A, 64, generator=g).to(dev, torch.bfloat16)
            y = torch.randint(0, 16, (8 * A,), generator=g).to(dev)
            for i in range(A):
                ga.begin()
                ops.softmax_cross_entropy(m(x[8 * i:8 * (i + 1)]), y[8 * i:8 * (i + 1)]).backward()
                ga.end()
            ga.step(o)
        torch.cuda.synchronize()
        out = []
        for grp in fl:
            out += [grp.master.clone()] + ([grp.mirror.clone()] if grp.mirror is not None else [])
            out += [v.clone() for _, v in sorted(grp.state.items())]
        if d is not None:
            ga.detach()
            d.remove_hooks()
        return out

    a, b2 = run(True), run(False)
    assert len(a) == len(b2) and all(same_bits(x, y) for x, y in zip(a, b2)), "dp.step window != plain window"
    comm.shutdown()
    print("accum ddp ok", flush=True)


if __name__ == "__main__":
    main()
