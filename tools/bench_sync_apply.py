#!/usr/bin/env python3
"""The synchronous PS's hot path: the fused k-way sum-apply against the unfused sequence it replaces.

  fused    one ``momentum_sum`` / ``adam_sum`` launch over k bf16 gradient buffers (csrc/kernels/optim.hip)
  unfused  k x ``axpby`` into an fp32 accumulator, then ``momentum`` / ``adam`` on it with ``zero_grad``
           (accumulate-as-they-arrive, what the kernels before the sum-apply allow)

at the compute-group sizes of ResNet-50 and BERT-base, k = 2 and k = 7.  Bytes per element, from the kernels'
access lists (bf16 gradients, fp32 master + slots, bf16 mirror):

  momentum  fused 2k + 18   unfused 10k + 26        adam  fused 2k + 26   unfused 10k + 34

Method: every shape is warmed up, each variant is timed with device events over a window of about
``--window`` seconds, the two variants alternate over ``--rounds`` rounds, and the table reports the median with
the min..max spread.  GB/s = the bytes above x elements / time (an algorithmic rate: what the infinity cache
serves is not subtracted).  Needs a GPU; prints the device it ran on.  Exits 1 if the fused form is not faster
at some point.

    python tools/bench_sync_apply.py [--out profiles/sync_ps/apply_table.md]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dtg  # noqa: E402,F401
from dtg.ops import optim_kernels as K  # noqa: E402

SIZES = {"resnet50": 25502912, "bert_base": 109956096}  # FlatParams(model).groups["compute"].numel


def _bytes(kind, k, fused):
    state = 18 if kind == "momentum" else 26
    return (2 * k + state) if fused else (10 * k + state + 8)


def _make(kind, n, k, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    s = {"w": torch.randn(n, device=dev, generator=g), "mir": torch.empty(n, device=dev, dtype=torch.bfloat16),
         "s0": torch.zeros(n, device=dev), "s1": torch.zeros(n, device=dev), "acc": torch.zeros(n, device=dev),
         "src": [(torch.randn(n, device=dev, generator=g) * 1e-3).bfloat16() for _ in range(k)],
         "hyper": torch.tensor([1e-3, 1.0], device=dev)}
    return s


def _fused(kind, s, k):
    if kind == "momentum":
        K.momentum_sum(s["w"], s["src"], s["s0"], s["hyper"], s["mir"], mu=0.9, wd=5e-5, gscale=1.0 / k)
    else:
        K.adam_sum(s["w"], s["src"], s["s0"], s["s1"], s["hyper"], s["mir"], wd=0.01, gscale=1.0 / k)


def _unfused(kind, s, k):
    for src in s["src"]:
        K.axpby(s["acc"], src, 1.0, 1.0)
    if kind == "momentum":
        K.momentum(s["w"], s["acc"], s["s0"], s["hyper"], s["mir"], mu=0.9, wd=5e-5, gscale=1.0 / k, zero_grad=True)
    else:
        K.adam(s["w"], s["acc"], s["s0"], s["s1"], s["hyper"], s["mir"], wd=0.01, gscale=1.0 / k, zero_grad=True)


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the markdown table here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sync_apply needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    where = "%s, torch %s, hip %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip)
    lines = ["Measured on: %s (one device, device events, %d rounds alternating fused / unfused, ~%.1f s windows)"
             % (where, a.rounds, a.window), "",
             "| model (elements) | rule | k | fused ms (min..max) | unfused ms (min..max) | speed-up | "
             "fused B/elem, GB/s | unfused B/elem, GB/s |", "|---|---|---|---|---|---|---|---|"]
    ok = True
    for model, n in SIZES.items():
        for kind in ("momentum", "adam"):
            for k in (2, 7):
                s = _make(kind, n, k, dev)
                variants = {"fused": lambda: _fused(kind, s, k), "unfused": lambda: _unfused(kind, s, k)}
                iters = {}
                for name, fn in variants.items():
                    for _ in range(a.warmup):
                        fn()
                    torch.cuda.synchronize()
                    iters[name] = max(10, int(a.window / _time(fn, 10)))
                t = {name: [] for name in variants}
                for _ in range(a.rounds):
                    for name, fn in variants.items():
                        t[name].append(_time(fn, iters[name]))
                med = {name: statistics.median(v) for name, v in t.items()}
                bf, bu = _bytes(kind, k, True), _bytes(kind, k, False)
                faster = max(t["fused"]) < min(t["unfused"])
                ok &= faster
                row = {"model": model, "n": n, "rule": kind, "k": k, "fused_ms": med["fused"] * 1e3,
                       "unfused_ms": med["unfused"] * 1e3, "speedup": med["unfused"] / med["fused"],
                       "fused_bytes_per_elem": bf, "unfused_bytes_per_elem": bu,
                       "fused_gbs": bf * n / med["fused"] / 1e9, "unfused_gbs": bu * n / med["unfused"] / 1e9,
                       "fused_faster_in_every_round": faster, "where": where}
                print(json.dumps(row), flush=True)
                lines.append("| %s (%d) | %s | %d | %.3f (%.3f..%.3f) | %.3f (%.3f..%.3f) | %.2fx | %d, %.0f | %d, %.0f |"
                             % (model, n, kind, k, med["fused"] * 1e3, min(t["fused"]) * 1e3, max(t["fused"]) * 1e3,
                                med["unfused"] * 1e3, min(t["unfused"]) * 1e3, max(t["unfused"]) * 1e3,
                                row["speedup"], bf, row["fused_gbs"], bu, row["unfused_gbs"]))
                del s, variants
                torch.cuda.empty_cache()
    table = "\n".join(lines) + "\n"
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table)
    print("fused faster than unfused at every point (slowest fused round < fastest unfused round):", ok)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
