#!/usr/bin/env python3
"""The evaluation path on one GPU: the metric kernels against framework ops, and the eval-mode ResNet-50 forward.

Part 1 -- ``xent_topk`` + ``metric_accumulate`` (csrc/kernels/eval_metrics.hip) against what one would assemble from
framework ops on the same tensors: ``F.cross_entropy(reduction="none")`` + ``topk(5)`` + the comparisons and sums
that turn them into the same five numbers, at ``[1024, 1000]`` (the ResNet head) and ``[5120, 30528]`` (BERT's MLM
decoder) in bf16.  Device events around ``--launches`` back-to-back calls, every shape warmed, ``--rounds`` rounds
alternating the two paths.  Reported: time per call, and for the MLM shape ``B * V * 2`` bytes over that time next to
the HBM copy rate of profiles/r05_hbm_probe.  The 2 MB ResNet shape is launch-bound (two launches, the second one
workgroup): its time is reported, a bandwidth is not.

Part 2 -- ``Evaluator`` over a generated record set with ResNet-50 in eval mode at ``--batch`` (default 1024): images/s
of the second pass (the first warms every shape), and the model forward alone under device events for comparison.

Nothing here is a pass/fail number.

    python tools/bench_eval.py [--skip_model] [--records 2048 --batch 1024 --image 224] [--json FILE]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dtg  # noqa: E402,F401
from dtg.ops.metrics import metric_accumulate, xent_topk  # noqa: E402

HBM_COPY_TBS = 5.28  # profiles/r05_hbm_probe: read + written bytes of a large copy over its time
KS = (1, 5)


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches  # ms per call


def torch_path(logits, labels, acc):
    """the same sums from framework ops: n, loss sum, top-1 and top-5 counts (labels all in range here)"""
    loss = F.cross_entropy(logits.float(), labels, reduction="none")
    top = logits.topk(5, dim=1).indices
    hit = top == labels[:, None]
    acc[0] += labels.numel()
    acc[1] += loss.double().sum()
    acc[4] += hit[:, 0].sum()
    acc[5] += hit.any(1).sum()


def bench_metrics(B, V, launches, rounds, dev):
    g = torch.Generator(device="cuda").manual_seed(B + V)
    logits = (torch.randn(B, V, device=dev, generator=g) * 3).bfloat16()
    labels = torch.randint(0, V, (B,), device=dev, generator=g)
    acc = torch.zeros(8, device=dev, dtype=torch.float64)
    acc_t = torch.zeros(8, device=dev, dtype=torch.float64)

    def ours():
        loss, rank = xent_topk(logits, labels)
        metric_accumulate(acc, loss, rank, KS, V)

    def theirs():
        torch_path(logits, labels, acc_t)

    ours()
    theirs()
    torch.cuda.synchronize()
    # bf16 ties make topk's choice among equal logits differ from the lower-column rule: reported, not asserted
    agree = {"n": acc[0].item() == acc_t[0].item(), "top1_diff": acc[4].item() - acc_t[4].item(),
             "top5_diff": acc[5].item() - acc_t[5].item(),
             "loss_rel_diff": abs(acc[1].item() - acc_t[1].item()) / abs(acc_t[1].item())}
    for fn in (ours, theirs):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rows = []
    for r in range(rounds):
        t_o, t_t = timed(ours, launches), timed(theirs, launches)
        rows.append({"round": r, "hip_ms": t_o, "torch_ms": t_t})
        print("[%d, %d] round %d: xent_topk + metric_accumulate %.4f ms, PyTorch path %.4f ms" % (B, V, r, t_o, t_t),
              flush=True)
    hip = np.array([x["hip_ms"] for x in rows])
    tor = np.array([x["torch_ms"] for x in rows])
    nbytes = B * V * 2
    res = {"B": B, "V": V, "launches": launches, "rounds": rows, "logit_bytes": nbytes,
           "hip_ms_median": float(np.median(hip)), "hip_ms_min": float(hip.min()), "hip_ms_max": float(hip.max()),
           "torch_ms_median": float(np.median(tor)), "torch_ms_min": float(tor.min()), "torch_ms_max": float(tor.max()),
           "agreement_with_torch_path": agree}
    line = "[%d, %d] bf16: ours median %.4f ms [%.4f, %.4f], PyTorch path median %.4f ms [%.4f, %.4f] (%.1fx)" % (
        B, V, res["hip_ms_median"], res["hip_ms_min"], res["hip_ms_max"], res["torch_ms_median"], res["torch_ms_min"],
        res["torch_ms_max"], res["torch_ms_median"] / res["hip_ms_median"])
    if nbytes >= 64 << 20:
        rate = nbytes / (res["hip_ms_median"] * 1e-3) / 1e12
        res.update(logit_TBps=float(rate), share_of_hbm_copy_rate=float(rate / HBM_COPY_TBS),
                   hbm_copy_TBps=HBM_COPY_TBS)
        line += "; %.0f MB of logits read once = %.3f TB/s, %.0f%% of the %.2f TB/s HBM copy rate" % (
            nbytes / 1e6, rate, 100 * rate / HBM_COPY_TBS, HBM_COPY_TBS)
    else:
        res["logit_TBps"] = None
        line += "; %.1f MB of logits: launch-bound (two launches), no bandwidth quoted" % (nbytes / 1e6)
    print(line, flush=True)
    return res


def bench_model(records, batch, image, dev):
    from dtg.data import DeviceLoader, synthetic_image_set, write_image_shards
    from dtg.models import resnet
    from dtg.parallel import FlatParams
    from dtg.train import Evaluator
    torch.manual_seed(0)
    model = resnet.resnet50().to(dev).to(memory_format=torch.channels_last)
    FlatParams(model)
    with tempfile.TemporaryDirectory() as d:
        images, labels = synthetic_image_set(records, size=image + 8, classes=1000, seed=0)
        write_image_shards(d, images, labels, per_shard=512)
        del images
        with DeviceLoader(d, batch, image, dev, train=False, drop_last=False) as loader:
            ev = Evaluator(model, loader, ks=KS)
            warm = ev.run()
            res = ev.run()
            counters = loader.counters()
    x, _ = resnet.synthetic_batch(batch, dev, torch.bfloat16, image, 1000)
    model.eval()
    with torch.no_grad():
        for _ in range(2):
            model(x)
        torch.cuda.synchronize()
        fwd_ms = [timed(lambda: model(x), 3) for _ in range(3)]
    out = {"records": records, "batch": batch, "image": image, "evaluator_images_per_sec": res["images_per_sec"],
           "evaluator_seconds": res["seconds"], "first_pass_seconds": warm["seconds"], "n": res["n"],
           "loader_wait_ms": counters["wait_ms"], "loader_gather_ms": counters["gather_ms"],
           "forward_ms_median": float(np.median(fwd_ms)),
           "forward_images_per_sec": batch / (float(np.median(fwd_ms)) * 1e-3)}
    print("ResNet-50 eval mode, batch %d at %d x %d: Evaluator %.0f images/s over %d records (second pass, %.3f s; "
          "loader waits %.0f ms over both passes); the forward alone %.2f ms = %.0f images/s" % (
              batch, image, image, out["evaluator_images_per_sec"], res["n"], res["seconds"], counters["wait_ms"],
              out["forward_ms_median"], out["forward_images_per_sec"]), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip_model", action="store_true")
    ap.add_argument("--records", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures on a GPU; none is available")
    dev = torch.device("cuda", 0)
    res = {"metrics": [bench_metrics(1024, 1000, a.launches, a.rounds, dev),
                       bench_metrics(5120, 30528, a.launches, a.rounds, dev)]}
    if not a.skip_model:
        res["resnet50_eval"] = bench_model(a.records, a.batch, a.image, dev)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
