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

``--cache_dtype fp8`` times the same shapes on the quantised cache (csrc/kernels/attention_decode_fp8.hip), (a) the call
and (b) the step, with the bf16 cache of the same shape alternating in every round.

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


def extend_kernel_part(a, shapes):
    """``--extend`` (a): attn_extend at T = 1, 16, 64 beside attn_decode on the same caches, alternating in a round."""
    nh, dev = a.nh, "cuda"
    fns = {}
    for B, n in shapes:
        kc = torch.randn(B, nh, n + 64, 64, device=dev).bfloat16()
        vc = torch.randn(B, nh, n + 64, 64, device=dev).bfloat16()
        lens0 = torch.full((B,), n, dtype=torch.int32, device=dev)
        q = {Tn: torch.randn(B * Tn, 3 * nh * 64, device=dev).bfloat16() for Tn in (1, 16, 64)}
        fns[(B, n, 0)] = lambda q=q[1], l0=lens0, n=n, kc=kc, vc=vc: T.attn_decode(q, l0, 0, n, kc, vc, a.window)
        for Tn in (1, 16, 64):
            fns[(B, n, Tn)] = lambda q=q[Tn], l0=lens0, n=n, kc=kc, vc=vc, Tn=Tn: T.attn_extend(q, l0, 0, n, kc, vc, Tn,
                                                                                                a.window)
    times = {s: [] for s in fns}
    for _ in range(a.rounds):
        for s, fn in fns.items():
            times[s].append(timeit(fn, a.iters))
    for (B, n, Tn), v in times.items():
        vis = min(n, a.window - 1) if a.window else n
        nbytes = B * nh * vis * 256
        r = summarize({"part": "attn_extend" if Tn else "attn_decode", "B": B, "len": n, "T": Tn or 1, "nh": nh,
                       "window": a.window, "rounds": a.rounds, "nsplit": lib().attn_decode_splits(B * nh, n, a.window),
                       "kv_mb": round(nbytes / 2 ** 20, 1)}, {"call_us": v})
        r["kv_tbs"] = round(nbytes / r["call_us"] * 1e-6, 3)
        r["fraction_of_copy"] = round(r["kv_tbs"] / a.copy_tbs, 3)
        print(json.dumps(r), flush=True)


def extend_model_part(a, shapes):
    """``--extend`` (b): one extend of T = 16 against 16 decode steps and one; (c): prefill(chunk=64) against
    prefill(chunk=0), B * len <= ``--full_cap``."""
    cfg = BertConfig(max_position=max(n for _, n in shapes) + 64, window=a.window)
    torch.manual_seed(0)
    model = CausalLM(cfg).cuda().eval()
    for p in model.parameters():
        if p.dim() == 2:
            p.data = p.data.bfloat16()
    for B, n in shapes:
        if B * n > a.full_cap:
            print(json.dumps({"part": "extend", "B": B, "len": n, "skipped": "B * len > %d" % a.full_cap}))
            continue
        ids = torch.randint(0, 30000, (B, n), device="cuda")
        cache = KVCache(cfg, B, n + 16, "cuda")
        model.prefill(ids, [n] * B, cache)
        new = torch.randint(0, 30000, (B, 16), device="cuda")

        def steps(k):
            cache.t = 0  # the same positions every time
            for i in range(k):
                model.decode_step(new[:, i], cache)

        def extend():
            cache.t = 0
            return model.extend(new, cache)

        fns = {"extend16_us": extend, "decode16_us": lambda: steps(16), "decode1_us": lambda: steps(1),
               "prefill_chunk64_us": lambda: model.prefill(ids, [n] * B, cache, chunk=64),
               "prefill_us": lambda: model.prefill(ids, [n] * B, cache)}
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(timeit(fn, max(1, a.iters // 10)))
        r = summarize({"part": "extend", "B": B, "len": n, "layers": cfg.layers, "hidden": cfg.hidden,
                       "window": a.window, "rounds": a.rounds}, times)
        r["decode16_over_extend16"] = round(r["decode16_us"] / r["extend16_us"], 2)
        r["extend16_over_decode1"] = round(r["extend16_us"] / r["decode1_us"], 2)
        r["chunk64_over_prefill"] = round(r["prefill_chunk64_us"] / r["prefill_us"], 2)
        print(json.dumps(r), flush=True)
        del cache, ids
        torch.cuda.empty_cache()


def fp8_kernel_part(a, shapes):
    """``--cache_dtype fp8`` (a): attn_decode on an FP8 cache beside the bf16 cache of the same shape, alternating in a
    round.  Visible bytes: 68 per row and tensor (64 codes and a scale) against 128."""
    nh, dev = a.nh, "cuda"
    fns = {}
    for B, n in shapes:
        qkv1 = torch.randn(B, 3 * nh * 64, device=dev).bfloat16()
        lens0 = torch.full((B,), n, dtype=torch.int32, device=dev)
        kc, vc = (torch.randn(B, nh, n + 1, 64, device=dev).bfloat16() for _ in range(2))
        (k8, ks), (v8, vs) = T.kv_quantize(kc), T.kv_quantize(vc)
        fns[(B, n, "bf16")] = lambda q=qkv1, l0=lens0, n=n, kc=kc, vc=vc: T.attn_decode(q, l0, 0, n, kc, vc, a.window)
        fns[(B, n, "fp8")] = lambda q=qkv1, l0=lens0, n=n, kc=k8, vc=v8, ks=ks, vs=vs: T.attn_decode(
            q, l0, 0, n, kc, vc, a.window, ks, vs)
    times = {s: [] for s in fns}
    for _ in range(a.rounds):
        for s, fn in fns.items():
            times[s].append(timeit(fn, a.iters))
    for B, n in shapes:
        vis = min(n, a.window - 1) if a.window else n
        nbytes = B * nh * vis * 2 * 68
        r = summarize({"part": "attn_decode_fp8", "B": B, "len": n, "nh": nh, "window": a.window, "rounds": a.rounds,
                       "nsplit": lib().attn_decode_splits(B * nh, n, a.window), "kv_mb": round(nbytes / 2 ** 20, 1),
                       "bf16_kv_mb": round(B * nh * vis * 256 / 2 ** 20, 1)},
                      {"fp8_us": times[(B, n, "fp8")], "bf16_us": times[(B, n, "bf16")]})
        r["fp8_over_bf16"] = round(r["fp8_us"] / r["bf16_us"], 3)
        r["kv_tbs"] = round(nbytes / r["fp8_us"] * 1e-6, 3)
        r["fraction_of_copy"] = round(r["kv_tbs"] / a.copy_tbs, 3)
        print(json.dumps(r), flush=True)


def fp8_model_part(a, shapes):
    """``--cache_dtype fp8`` (b): one decode_step with an FP8 cache beside one with a bf16 cache, B * len <=
    ``--full_cap`` (the prefill's activations)."""
    cfg = BertConfig(max_position=max(n for _, n in shapes) + 64, window=a.window)
    torch.manual_seed(0)
    model = CausalLM(cfg).cuda().eval()
    for p in model.parameters():
        if p.dim() == 2:
            p.data = p.data.bfloat16()
    for B, n in shapes:
        if B * n > a.full_cap:
            print(json.dumps({"part": "decode_step_fp8", "B": B, "len": n, "skipped": "B * len > %d" % a.full_cap}))
            continue
        ids = torch.randint(0, 30000, (B, n), device="cuda")
        caches = {"bf16": KVCache(cfg, B, n + 1, "cuda"), "fp8": KVCache(cfg, B, n + 1, "cuda", torch.float8_e4m3fn)}
        tok = [model.prefill(ids, [n] * B, c).argmax(-1) for c in caches.values()][0]

        def step(cache):
            cache.t = 0  # the same position every time: the step appends to row n again
            return model.decode_step(tok, cache)

        times = {"fp8_step_us": [], "bf16_step_us": []}
        for _ in range(a.rounds):
            for k in ("fp8", "bf16"):
                times[k + "_step_us"].append(timeit(lambda c=caches[k]: step(c), a.iters))
        r = summarize({"part": "decode_step_fp8", "B": B, "len": n, "layers": cfg.layers, "hidden": cfg.hidden,
                       "window": a.window, "rounds": a.rounds}, times)
        r["fp8_over_bf16"] = round(r["fp8_step_us"] / r["bf16_step_us"], 3)
        print(json.dumps(r), flush=True)
        del caches, ids
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache_dtype", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: the same tables on the quantised cache, the bf16 cache alternating in the same run")
    ap.add_argument("--extend", action="store_true", help="time attn_extend / CausalLM.extend / chunked prefill instead")
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
    if a.extend and a.cache_dtype == "fp8":
        ap.error("--extend: attn_extend does not serve the quantised cache")
    fp8 = a.cache_dtype == "fp8"
    if a.part in ("kernel", "both"):
        (extend_kernel_part if a.extend else fp8_kernel_part if fp8 else kernel_part)(a, shapes)
    if a.part in ("model", "both"):
        (extend_model_part if a.extend else fp8_model_part if fp8 else model_part)(a, shapes)


if __name__ == "__main__":
    main()
