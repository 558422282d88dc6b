#!/usr/bin/env python3
"""What the gradient-accumulation kernels cost (csrc/include/dtg/grad_fold.cuh), at the compute-group sizes of
ResNet-50 (25.5 M bf16 gradient elements) and BERT-base (110 M), next to what they replace:

  grad_fold first / grad_fold add          one launch: acc (+)= float(g), g = 0
  grad_sum(k=1) + fill_zero, first / add   the same arithmetic and bytes in two launches (the pair that existed)
  grad_fold nt first / nt add              grad_fold with non-temporal accumulator stores (the lab extension's form)
  grad_unfold                              g = bf16(acc + float(g)) over the whole buffer

Algorithmic bytes per bf16 element: fold 8 with ``first`` (read g 2, write acc 4, zero g 2), 12 otherwise (+ read acc
4); unfold 8 (read acc 4, read g 2, write g 2).  TB/s = bytes x elements / time, beside the 5.28 TB/s copy rate of
profiles/r05_hbm_probe; what the infinity cache serves is not subtracted (ResNet-50's 51 MB + 102 MB fit in its
256 MiB, BERT's 220 MB + 440 MB do not).  Timing: device events around a window of back-to-back launches, the variants
alternating over ``--rounds`` rounds; the table gives the median and the rounds' min..max.  Needs a GPU.

    python tools/bench_accum.py [--out profiles/grad_accum/kernels.md]
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
from dtg.ops._native import lab as _lab_loader, lib  # noqa: E402

SIZES = {"resnet50": 25_500_000, "bert_base": 110_000_000}
COPY_TBS = 5.28  # profiles/r05_hbm_probe


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def _lab():
    try:
        return _lab_loader()
    except (ImportError, RuntimeError):  # the lab extension is optional: without it the nt rows are left out
        return None


def _variants(n, dev):
    acc = torch.zeros(n, device=dev)
    g = (torch.randn(n, device=dev) * 1e-3).to(torch.bfloat16)
    fill = lib().zero_  # the fill_zero kernel of optim.hip

    def pair(first):
        def run():
            K.grad_sum(acc, [g], first)
            fill(g)
        return run
    v = {
        "grad_fold first": (lambda: K.grad_fold(acc, g, True), 8),
        "grad_sum(k=1) + fill_zero, first": (pair(True), 8),
        "grad_fold add": (lambda: K.grad_fold(acc, g, False), 12),
        "grad_sum(k=1) + fill_zero, add": (pair(False), 12),
        "grad_unfold": (lambda: K.grad_unfold(g, acc), 8),
    }
    lab = _lab()
    if lab is not None and hasattr(lab, "grad_fold_nt"):
        v["grad_fold nt first"] = (lambda: lab.grad_fold_nt(acc, g, True), 8)
        v["grad_fold nt add"] = (lambda: lab.grad_fold_nt(acc, g, False), 12)
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2, help="seconds per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--models", default="resnet50,bert_base")
    ap.add_argument("--out", default=None, help="also write the markdown table here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_accum needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    where = "%s, torch %s, hip %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip)
    lines = ["Measured on: %s (one device, device events, %d rounds alternating over the variants, ~%.2f s windows)"
             % (where, a.rounds, a.window), ""]
    for model in a.models.split(","):
        n = SIZES[model]
        variants = _variants(n, dev)
        iters = {}
        for name, (fn, _) in variants.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            iters[name] = max(5, int(a.window / _time(fn, 5)))
        t = {name: [] for name in variants}
        for _ in range(a.rounds):
            for name, (fn, _) in variants.items():
                t[name].append(_time(fn, iters[name]))
        med = {name: statistics.median(x) for name, x in t.items()}
        lines += ["**%s**: %d bf16 gradient elements, fp32 accumulator" % (model, n), "",
                  "| variant | ms (min..max) | B/elem | TB/s | of the %.2f TB/s copy rate |" % COPY_TBS,
                  "|---|---|---|---|---|"]
        for name, (_, bpe) in variants.items():
            rate = bpe * n / med[name] / 1e12
            row = {"model": model, "variant": name, "ms": med[name] * 1e3, "min_ms": min(t[name]) * 1e3,
                   "max_ms": max(t[name]) * 1e3, "bytes_per_elem": bpe, "tbs": rate, "of_copy": rate / COPY_TBS,
                   "where": where}
            print(json.dumps(row), flush=True)
            lines.append("| %s | %.4f (%.4f..%.4f) | %d | %.2f | %.2f |" % (name, row["ms"], row["min_ms"],
                                                                           row["max_ms"], bpe, rate, rate / COPY_TBS))
        for x, y in (("grad_fold first", "grad_sum(k=1) + fill_zero, first"),
                     ("grad_fold add", "grad_sum(k=1) + fill_zero, add"),
                     ("grad_fold nt first", "grad_fold first"), ("grad_fold nt add", "grad_fold add")):
            if x in med and y in med:
                lines += ["", "%s / %s: %.3fx the time" % (x, y, med[x] / med[y])]
        lines.append("")
        del variants
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
