#!/usr/bin/env python3
"""Attention microbenchmark at BERT-base heads: the fused kernels (attention.hip at S <= 512, the K/V-streaming
attention_stream.hip above that) and, where it exists (S <= 1024 keys), the unfused path (strided-batched MFMA GEMMs +
softmax kernels).

    python tools/bench_attention.py --shapes 64x512,32x1024,16x2048,8x4096 --rounds 5

One JSON line per shape (B x S): per path the median over the rounds (device events, warm-up before every timing; each
round times every path of every shape once, so the paths alternate) with the rounds' min / max, and the algorithmic
TFLOP/s of the fused kernels from the shape alone: 4 * B * nh * S * S * 64 FLOP forward (QK^T and PV), 10 * ...
backward (recomputed QK^T, dP, dV, dK, dQ) -- not what the kernels execute (softmax, dropout and the backward's second
recomputation of QK^T and dP are not counted).

``--causal``: the causal kernels (attention_causal.hip) against the bidirectional fused kernels at the same shapes, both
backward passes with the QKV bias gradient (``dbias``), and both ``blockIdx.y`` dispatch orders of the causal kernels
(``causal_*``: the heaviest blocks first, the default; ``causal_light_first_*``: the other way round), plus the ratios
causal / bidirectional of the medians.  The unfused path is not timed."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dtg  # noqa: E402,F401
from dtg.ops import lib, transformer as T  # noqa: E402


GEMM_MAX_KEYS = 1024  # the softmax kernels' cap (transformer.hip, attn_max_keys): no unfused path beyond it


def timeit(fn, iters=20):
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


def paths(B, S, nh, p, causal=False):
    """-> {name: callable} of the paths that exist at this shape (their operands are kept alive by the closures)"""
    H = nh * 64
    L = lib()
    qkv = torch.randn(B * S, 3 * H, device="cuda").bfloat16()
    mask = torch.zeros(B, S, device="cuda")
    dout = torch.randn(B * S, H, device="cuda").bfloat16()
    fns = {}
    if causal:
        db = torch.zeros(3 * H, device="cuda")
        out, lse = L.attn_fused_fwd(qkv, mask, B, S, nh, p, 1)
        outc, lsec = L.attn_causal_fwd(qkv, mask, B, S, nh, p, 1)

        def causal_fn(fwd, heavy_first):
            def run():
                L.attn_causal_heavy_first(heavy_first)
                r = (L.attn_causal_fwd(qkv, mask, B, S, nh, p, 1) if fwd else
                     L.attn_causal_bwd(qkv, outc, dout, lsec, mask, B, S, nh, p, 1, db))
                L.attn_causal_heavy_first(True)
                return r
            return run

        fns["fused_fwd_us"] = lambda: L.attn_fused_fwd(qkv, mask, B, S, nh, p, 1)
        fns["fused_bwd_us"] = lambda: L.attn_fused_bwd(qkv, out, dout, lse, mask, B, S, nh, p, 1, db)
        fns["causal_fwd_us"], fns["causal_bwd_us"] = causal_fn(True, True), causal_fn(False, True)
        fns["causal_light_first_fwd_us"] = causal_fn(True, False)
        fns["causal_light_first_bwd_us"] = causal_fn(False, False)
        return fns
    if L.attn_fused_supported(S, 64, True):
        out, lse = L.attn_fused_fwd(qkv, mask, B, S, nh, p, 1)
        fns["fused_fwd_us"] = lambda: L.attn_fused_fwd(qkv, mask, B, S, nh, p, 1)
        fns["fused_bwd_us"] = lambda: L.attn_fused_bwd(qkv, out, dout, lse, mask, B, S, nh, p, 1)
    if S <= GEMM_MAX_KEYS:
        _, P, Pd = T.attention_fwd(qkv, mask, B, S, nh, p, 1)
        dq = torch.empty_like(qkv)
        fns["gemm_fwd_us"] = lambda: T.attention_fwd(qkv, mask, B, S, nh, p, 1)
        fns["gemm_bwd_us"] = lambda: T.attention_bwd(dout, qkv, P, Pd, B, S, nh, dq)
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--S", type=int, default=128)
    ap.add_argument("--shapes", default=None, help="comma-separated BxS list (default: --B x --S)")
    ap.add_argument("--nh", type=int, default=12)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--causal", action="store_true", help="causal against bidirectional fused, both dispatch orders")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")] if a.shapes else [(a.B, a.S)]
    res = []
    for B, S in shapes:  # one shape's operands at a time: the unfused path keeps [B * nh * S, S] tensors
        fns = paths(B, S, a.nh, a.p, a.causal)
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(timeit(fn, a.iters))
        r = {"shape": [B, S, a.nh], "rounds": a.rounds}
        for k, v in times.items():
            r[k] = round(statistics.median(v), 1)
            if a.rounds > 1:
                r[k[:-3] + "_range_us"] = [round(min(v), 1), round(max(v), 1)]
        flop = 4.0 * B * a.nh * S * S * 64
        if "fused_fwd_us" in r:
            r["fused_fwd_tflops"] = round(flop / r["fused_fwd_us"] * 1e-6, 1)
            r["fused_bwd_tflops"] = round(2.5 * flop / r["fused_bwd_us"] * 1e-6, 1)
        if a.causal:
            for k in ("fwd", "bwd"):
                r["causal_over_fused_" + k] = round(r["causal_%s_us" % k] / r["fused_%s_us" % k], 3)
                r["light_first_over_heavy_first_" + k] = round(
                    r["causal_light_first_%s_us" % k] / r["causal_%s_us" % k], 3)
        res.append(r)
        print(json.dumps(r), flush=True)
        del fns
        torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    main()
