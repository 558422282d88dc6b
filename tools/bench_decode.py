#!/usr/bin/env python3
"""Incremental-decoding benchmark (csrc/kernels/attention_decode.hip, CausalLM.decode_step).

    python tools/bench_decode.py --lens 512,2048,8192 --batches 1,8,64 --rounds 5

(a) ``attn_decode`` alone at BERT-base heads: per (B, len) the median over the rounds (device events, a warm-up before
    every timing; each round times every shape once), the rounds' min / max, the split count the launcher chose, and
    the visible K/V bytes (B * nh * len * 256) over the median beside ``--copy_tbs``, the device copy bandwidth of
    profiles/r05_hbm_probe.  The cache of a shape is read again by every iteration: a shape whose K/V fit the last-level
    cache is served from it, so ``kv_mb`` stands beside each figure.
(b) one ``decode_step`` of a BERT-base-sized CausalLM against ``CausalLM.logits`` on the whole prefix (what the model
    offered before the cache) at the same shapes, where the full forward's [B * len, V] logits fit (B * len <=
    ``--full_cap`` tokens; the others are listed as skipped).

One JSON line per shape and part."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dtg  # noqa: E402,F401
from dtg.models import BertConfig, CausalLM, KVCache  # noqa: E402
from dtg.ops import lib, transformer as T  # noqa: E402


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def summarize(r, times):
    for k, v in times.items():
        r[k] = round(statistics.median(v), 1)
        r[k[:-3] + "_range_us"] = [round(min(v), 1), round(max(v), 1)]
    return r


def kernel_part(a, shapes):
    nh, dev = a.nh, "cuda"
    fns = {}
    for B, n in shapes:
        kc = torch.randn(B, nh, n + 1, 64, device=dev).bfloat16()
        vc = torch.randn(B, nh, n + 1, 64, device=dev).bfloat16()
        qkv1 = torch.randn(B, 3 * nh * 64, device=dev).bfloat16()
        lens0 = torch.full((B,), n, dtype=torch.int32, device=dev)
        fns[(B, n)] = lambda q=qkv1, l0=lens0, n=n, kc=kc, vc=vc: T.attn_decode(q, l0, 0, n, kc, vc, a.window)
    times = {s: [] for s in fns}
    for _ in range(a.rounds):
        for s, fn in fns.items():
            times[s].append(timeit(fn, a.iters))
    for (B, n), v in times.items():
        vis = min(n, a.window - 1) if a.window else n
        nbytes = B * nh * vis * 256
        r = summarize({"part": "attn_decode", "B": B, "len": n, "nh": nh, "window": a.window, "rounds": a.rounds,
                       "nsplit": lib().attn_decode_splits(B * nh, n, a.window), "kv_mb": round(nbytes / 2 ** 20, 1)},
                      {"decode_us": v})
        r["kv_tbs"] = round(nbytes / r["decode_us"] * 1e-6, 3)
        r["fraction_of_copy"] = round(r["kv_tbs"] / a.copy_tbs, 3)
        print(json.dumps(r), flush=True)


def model_part(a, shapes):
    cfg = BertConfig(max_position=max(n for _, n in shapes) + 64, window=a.window)
    torch.manual_seed(0)
    model = CausalLM(cfg).cuda().eval()
    for p in model.parameters():
        if p.dim() == 2:
            p.data = p.data.bfloat16()
    for B, n in shapes:
        if B * n > a.full_cap:
            print(json.dumps({"part": "decode_step", "B": B, "len": n, "skipped": "B * len > %d" % a.full_cap}))
            continue
        ids = torch.randint(0, 30000, (B, n), device="cuda")
        cache = KVCache(cfg, B, n + 1, "cuda")
        tok = model.prefill(ids, [n] * B, cache).argmax(-1)

        def step():
            cache.t = 0  # the same position every time: the step appends to row n again
            return model.decode_step(tok, cache)

        def full():
            with torch.no_grad():
                return model.logits(ids)

        times = {"decode_step_us": [], "full_forward_us": []}
        for _ in range(a.rounds):
            times["decode_step_us"].append(timeit(step, a.iters))
            times["full_forward_us"].append(timeit(full, max(1, a.iters // 10)))
        r = summarize({"part": "decode_step", "B": B, "len": n, "layers": cfg.layers, "hidden": cfg.hidden,
                       "window": a.window, "rounds": a.rounds}, times)
        r["full_over_step"] = round(r["full_forward_us"] / r["decode_step_us"], 1)
        print(json.dumps(r), flush=True)
        del cache, ids
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lens", default="512,2048,8192")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--nh", type=int, default=12)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--copy_tbs", type=float, default=5.28, help="device copy bandwidth (profiles/r05_hbm_probe)")
    ap.add_argument("--full_cap", type=int, default=32768, help="largest B * len the full forward is timed at")
    ap.add_argument("--part", choices=["kernel", "model", "both"], default="both")
    a = ap.parse_args()
    shapes = [(int(B), int(n)) for B in a.batches.split(",") for n in a.lens.split(",")]
    if a.part in ("kernel", "both"):
        kernel_part(a, shapes)
    if a.part in ("model", "both"):
        model_part(a, shapes)


if __name__ == "__main__":
    main()
