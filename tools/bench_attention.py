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
causal / bidirectional of the medians.  The unfused path is not timed.  Then the packed causal kernels
(attention_causal_packed.hip) on records of mixed length (``synthetic_token_set``'s lengths; ``token_ratio`` = T / (B *
S)): ``packed_causal_*`` (both dispatch orders) against the re-padding sequence around the padded causal kernels
(``repad_causal_*``: seq_pad + attn_causal_fwd + seq_unpad; seq_pad(dO) + attn_causal_bwd + seq_unpad), and on
full-length records (``packed_full_*``) against the padded causal kernels themselves.

``--causal --window W[,W..]``: only the sliding-window kernels (attention_window.hip, ``window<W>_*``) against the
causal kernels (``causal_*``) at the same shapes, forward and backward with ``dbias``; beside each measured ratio
``window<W>_over_causal_*`` stands ``window<W>_pair_ratio_*``, the ratio of (block, chunk) pairs the two schedules
visit, computed from the shapes (``chunk_pairs``): the bound the measured ratio cannot go below."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dtg  # noqa: E402,F401
from dtg.data import synthetic_token_set  # noqa: E402
from dtg.ops import lib, seqpack, transformer as T  # noqa: E402


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


def packed_causal_paths(fns, B, S, nh, p, qkv, dout, db, heavy):
    """adds the packed causal paths to fns -> the mixed-length records' T / (B * S)"""
    L, H, dev = lib(), nh * 64, qkv.device
    lens = torch.from_numpy(synthetic_token_set(B, seq=S, vocab_lo=4, vocab_hi=30522, seed=7)["length"].copy())
    pack = seqpack.SeqPack.from_lengths(lens.to(torch.int32).to(dev), lens.numpy(), S)
    full = seqpack.SeqPack.from_lengths(torch.full((B,), S, dtype=torch.int32, device=dev), [S] * B, S)
    cu, Ta = pack.cu, pack.T_alloc
    mask = T.mask_additive((torch.arange(S, device=dev).view(1, S) < pack.lengths.view(B, 1)).float())
    qk, dk = qkv[:Ta].contiguous(), dout[:Ta].contiguous()
    cx, lse = L.attn_packed_causal_fwd(qk, cu, B, S, nh, p, 1)
    qp = seqpack.seq_pad(qk, cu, B, S)
    cp, lp = L.attn_causal_fwd(qp, mask, B, S, nh, p, 1)
    cf, lf = L.attn_packed_causal_fwd(qkv, full.cu, B, S, nh, p, 1)

    def repad_fwd():
        c, _ = L.attn_causal_fwd(seqpack.seq_pad(qk, cu, B, S), mask, B, S, nh, p, 1)
        return seqpack.seq_unpad(c, cu, B, S, Ta)

    def repad_bwd():
        d = L.attn_causal_bwd(qp, cp, seqpack.seq_pad(dk, cu, B, S), lp, mask, B, S, nh, p, 1, db)
        return seqpack.seq_unpad(d, cu, B, S, Ta)

    def pfwd():
        return L.attn_packed_causal_fwd(qk, cu, B, S, nh, p, 1)

    def pbwd():
        return L.attn_packed_causal_bwd(qk, cx, dk, lse, cu, B, S, nh, p, 1, db)

    fns["packed_causal_fwd_us"], fns["repad_causal_fwd_us"] = heavy(pfwd, True), repad_fwd
    fns["packed_causal_bwd_us"], fns["repad_causal_bwd_us"] = heavy(pbwd, True), repad_bwd
    fns["packed_causal_light_first_fwd_us"] = heavy(pfwd, False)
    fns["packed_causal_light_first_bwd_us"] = heavy(pbwd, False)
    fns["packed_full_fwd_us"] = lambda: L.attn_packed_causal_fwd(qkv, full.cu, B, S, nh, p, 1)
    fns["packed_full_bwd_us"] = lambda: L.attn_packed_causal_bwd(qkv, cf, dout, lf, full.cu, B, S, nh, p, 1, db)
    return pack.T / float(B * S)


def chunk_pairs(S, W=0):
    """-> (forward, backward) counts of the (128-row block, 64-row chunk) pairs one head's workgroups visit at
    sequence length S: the causal kernels' (W = 0) or the window kernels' loop bounds, from the shapes alone.  The
    backward is dQ (the forward's bounds) plus dKV."""
    n, w = S // 64, (W // 64 if 0 < W < S else S // 64)
    blocks = range((S + 127) // 128)
    fwd = sum(min(n, 2 * y + 2) - max(0, 2 * y - w) for y in blocks)
    dkv = sum(min(n, 2 * y + 2 + w) - 2 * y for y in blocks)
    return fwd, fwd + dkv


def window_paths(B, S, nh, p, windows):
    """-> {name: callable}: the causal kernels and the window kernels at each W, forward and backward with dbias"""
    H, L = nh * 64, lib()
    qkv = torch.randn(B * S, 3 * H, device="cuda").bfloat16()
    mask = torch.zeros(B, S, device="cuda")
    dout = torch.randn(B * S, H, device="cuda").bfloat16()
    db = torch.zeros(3 * H, device="cuda")
    outc, lsec = L.attn_causal_fwd(qkv, mask, B, S, nh, p, 1)
    fns = {"causal_fwd_us": lambda: L.attn_causal_fwd(qkv, mask, B, S, nh, p, 1),
           "causal_bwd_us": lambda: L.attn_causal_bwd(qkv, outc, dout, lsec, mask, B, S, nh, p, 1, db)}
    for W in windows:
        ow, lw = L.attn_window_fwd(qkv, mask, B, S, nh, W, p, 1)
        fns["window%d_fwd_us" % W] = lambda W=W: L.attn_window_fwd(qkv, mask, B, S, nh, W, p, 1)
        fns["window%d_bwd_us" % W] = (lambda W=W, ow=ow, lw=lw:
                                      L.attn_window_bwd(qkv, ow, dout, lw, mask, B, S, nh, W, p, 1, db))
    return fns


def paths(B, S, nh, p, causal=False):
    """-> {name: callable} of the paths that exist at this shape (their operands are kept alive by the closures);
    causal: the mixed-length records' token ratio under "token_ratio" (a number, not a path)"""
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

        def heavy(fn, on):  # fn under one dispatch order; the switch is left at its default
            def run():
                L.attn_causal_heavy_first(on)
                r = fn()
                L.attn_causal_heavy_first(True)
                return r
            return run

        fns["token_ratio"] = packed_causal_paths(fns, B, S, nh, p, qkv, dout, db, heavy)
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
    ap.add_argument("--window", default=None,
                    help="with --causal: comma-separated windows; the window kernels against the causal kernels only")
    a = ap.parse_args()
    if a.window and not a.causal:
        ap.error("--window needs --causal")
    windows = [int(w) for w in a.window.split(",")] if a.window else []
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")] if a.shapes else [(a.B, a.S)]
    res = []
    for B, S in shapes:  # one shape's operands at a time: the unfused path keeps [B * nh * S, S] tensors
        fns = window_paths(B, S, a.nh, a.p, windows) if windows else paths(B, S, a.nh, a.p, a.causal)
        ratio = fns.pop("token_ratio", None)
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
        for W in windows:  # measured window / causal beside the ratio of pairs visited (the algorithmic bound)
            for i, k in enumerate(("fwd", "bwd")):
                r["window%d_over_causal_%s" % (W, k)] = round(r["window%d_%s_us" % (W, k)] / r["causal_%s_us" % k], 3)
                r["window%d_pair_ratio_%s" % (W, k)] = round(chunk_pairs(S, W)[i] / chunk_pairs(S)[i], 3)
        if a.causal and not windows:
            for k in ("fwd", "bwd"):
                r["causal_over_fused_" + k] = round(r["causal_%s_us" % k] / r["fused_%s_us" % k], 3)
                r["light_first_over_heavy_first_" + k] = round(
                    r["causal_light_first_%s_us" % k] / r["causal_%s_us" % k], 3)
                r["packed_over_repad_" + k] = round(r["packed_causal_%s_us" % k] / r["repad_causal_%s_us" % k], 3)
                r["packed_light_first_over_heavy_first_" + k] = round(
                    r["packed_causal_light_first_%s_us" % k] / r["packed_causal_%s_us" % k], 3)
                r["packed_full_over_causal_" + k] = round(r["packed_full_%s_us" % k] / r["causal_%s_us" % k], 3)
            r["token_ratio"] = round(ratio, 4)
        res.append(r)
        print(json.dumps(r), flush=True)
        del fns
        torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    main()
