#!/usr/bin/env python3
"""BERT-base with and without padding on records of mixed length (dtg.ops.seqpack): what the packed path buys.

BERT-base, batch 256 x 128, batches of ``synthetic_token_set`` records (lengths 8 .. 128, one in eight full) masked by
``mlm_mask``; forward + backward + fused AdamW step.  The padded path (``pack=None``), the packed path with attention
on re-padded rows (``pack=SeqPack``, ``bert_fused._PACKED_ATTN`` off) and the packed path (attention on the packed
rows, attention_packed.hip) alternate over ``--rounds`` rounds on the same batches, the same weights' shapes and the
same build; each measurement is a window of ``--steps`` steps between two device events.  Reported: ms/step of each
(median and the rounds' min..max), the batches' T / (B * S), and the packed step as a share of the padded one -- the
token ratio is the bound, the distance from it is the work that still runs on padded rows (the heads; attention's
whole-record workgroups) or does not shrink with the rows (launches, the optimizer).

The four row kernels are then timed alone at this shape, with their algorithmic bytes against the 5.28 TB/s copy rate
of profiles/r05_hbm_probe (reads of real rows + writes of every output row; the position and type tables and ``cu``
stay in cache and are not counted), and attention alone: ``attn_packed_fwd`` / ``attn_packed_bwd`` (at 128 < S <= 512
their ``attn_packed_long_*`` forms, under the same row names) against the re-padding sequences ``seq_pad + attn_fused_fwd + seq_unpad`` / ``seq_pad + attn_fused_bwd + seq_unpad``.  Needs a GPU.

    python tools/bench_unpad.py [--rounds 5] [--steps 10] [--out profiles/bert_unpad/bench_unpad.md]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dtg  # noqa: E402,F401
from dtg.data import synthetic_token_set  # noqa: E402
from dtg.models import bert, bert_fused  # noqa: E402
from dtg.ops import lib, seqpack  # noqa: E402
from dtg.ops.mlm import count_valid, mlm_mask  # noqa: E402
from dtg.ops.seqpack import SeqPack  # noqa: E402
from dtg.ops.transformer import mask_additive  # noqa: E402
from dtg.optim import FusedAdam  # noqa: E402
from dtg.parallel import FlatParams, overlap  # noqa: E402

COPY_TBS = 5.28  # profiles/r05_hbm_probe
SPECIAL = (0, 1, 2, 3)


def _batches(n, B, S, dev, vocab_hi=30522, P=20):
    f = synthetic_token_set(n * B, seq=S, vocab_lo=4, vocab_hi=vocab_hi, seed=7)
    out = []
    for i in range(n):
        sl = slice(i * B, (i + 1) * B)
        ids, a_len, length = (torch.from_numpy(f[k][sl].copy()) for k in ("input_ids", "a_len", "length"))
        nsp = torch.from_numpy(f["next_sentence_label"][sl].copy())
        index = torch.arange(i * B, (i + 1) * B, dtype=torch.int64)
        masked = mlm_mask(ids.to(dev), a_len.to(dev), length.to(dev), index.to(dev), seed=1, epoch=0, P=P, mask_id=3,
                          vocab_lo=4, vocab_hi=vocab_hi, special_ids=SPECIAL)
        nv = max(1, count_valid(ids.numpy(), length.numpy(), P, 150, SPECIAL))
        pack = SeqPack.from_lengths(length.to(dev), length.numpy(), S)
        out.append(((*masked, nsp.to(dev)), nv, pack))
    return out


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters  # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nbatches", type=int, default=4)
    ap.add_argument("--tiny", action="store_true", help="2-layer model (a quick check of the tool itself)")
    ap.add_argument("--out", default=None, help="also write the markdown here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_unpad needs a GPU (a CPU run measures nothing)")
    if a.rounds < 5 and not a.tiny:
        sys.exit("at least 5 rounds")
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.seq
    cfg = bert.BertConfig(layers=2) if a.tiny else bert.BertConfig.base()
    torch.manual_seed(1234)
    model = bert.BertForPreTraining(cfg).to(dev)
    flat = FlatParams(model, compute_dtype=torch.bfloat16)
    opt = FusedAdam(flat, lr=1e-4, weight_decay=0.01)
    model.train()
    batches = _batches(a.nbatches, B, S, dev)
    ratio = sum(p.T for _, _, p in batches) / (len(batches) * B * S)
    ratio_alloc = sum(p.T_alloc for _, _, p in batches) / (len(batches) * B * S)
    seed = []

    def step(i, packed, packed_attn=True):
        b, nv, pack = batches[i % len(batches)]
        bert_fused._PACKED_ATTN = packed_attn
        loss = model(*b, num_valid=nv, pack=pack if packed else None)
        if not seed:
            seed.append(torch.ones_like(loss))
        loss.backward(seed[0])
        overlap.join()
        opt.step()
        return loss

    paths = {"padded": lambda i: step(i, False), "packed, attention re-padded": lambda i: step(i, True, False),
             "packed": lambda i: step(i, True)}
    for fn in paths.values():
        for i in range(a.warmup):
            fn(i)
    torch.cuda.synchronize()
    t = {k: [] for k in paths}
    for _ in range(a.rounds):
        for k, fn in paths.items():
            t[k].append(_window(fn, a.steps))
    med = {k: statistics.median(v) for k, v in t.items()}
    where = "%s, torch %s, hip %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip)
    share = med["packed"] / med["padded"]
    repad = "packed, attention re-padded"
    lines = ["Measured on: %s (one device, device events, %d rounds alternating the paths, windows of %d steps)"
             % (where, a.rounds, a.steps), "",
             "%s, batch %d x %d, %d batches of synthetic_token_set records: T / (B * S) = %.4f (T_alloc / (B * S) = "
             "%.4f)" % ("BERT-base" if not a.tiny else "2-layer BERT", B, S, len(batches), ratio, ratio_alloc), "",
             "| path | ms/step (min..max) | sequences/s |", "|---|---|---|"]
    for k in paths:
        lines.append("| %s | %.2f (%.2f..%.2f) | %.0f |" % (k, med[k], min(t[k]), max(t[k]), B / med[k] * 1e3))
    lines += ["", "packed / padded = %.4f of the step time; the bound T / (B * S) = %.4f; %.2f ms of the packed step "
              "(%.1f %% of the padded one) lie above the bound" % (share, ratio, med["packed"] - ratio * med["padded"],
                                                                  100 * (share - ratio)),
              "attention on the packed rows: %.2f ms/step below the re-padding path (%.2f -> %.2f; the two paths' own "
              "spreads: %.2f and %.2f ms)" % (med[repad] - med["packed"], med[repad], med["packed"],
                                             max(t[repad]) - min(t[repad]), max(t["packed"]) - min(t["packed"])), ""]
    print(json.dumps({"padded_ms": med["padded"], "packed_ms": med["packed"], "packed_repad_ms": med[repad],
                      "padded_range": [min(t["padded"]), max(t["padded"])],
                      "packed_range": [min(t["packed"]), max(t["packed"])],
                      "packed_repad_range": [min(t[repad]), max(t[repad])], "token_ratio": ratio,
                      "share": share, "where": where}), flush=True)

    # ---- the row kernels alone, at this shape ----
    pack = batches[0][2]
    T, Ta, H = pack.T, pack.T_alloc, cfg.hidden
    ids, tt = batches[0][0][0], batches[0][0][1]
    e = model.emb
    rows = {}
    for W in (3 * H, H):
        x_p = torch.randn(Ta, W, device=dev).bfloat16()
        x_d = torch.randn(B * S, W, device=dev).bfloat16()
        o_d, o_p = torch.empty_like(x_d), torch.empty_like(x_p)
        rows["seq_pad W=%d" % W] = ((lambda x=x_p, o=o_d: seqpack.seq_pad(x, pack.cu, B, S, out=o)),
                                    2 * W * (T + B * S))
        rows["seq_unpad W=%d" % W] = ((lambda x=x_d, o=o_p: seqpack.seq_unpad(x, pack.cu, B, S, Ta, out=o)),
                                      2 * W * (T + Ta))
    o_e = torch.empty(Ta, H, device=dev, dtype=torch.bfloat16)
    rows["emb_fwd_packed H=%d" % H] = ((lambda: seqpack.emb_fwd_packed(ids, tt, e.word, e.pos, e.tok_type, pack.cu, Ta,
                                                                      out=o_e)), 2 * H * (T + Ta) + 16 * T)
    ds = torch.randn(Ta, H, device=dev).bfloat16()
    gp = torch.zeros_like(e.pos)
    rows["emb_pos_bwd_packed H=%d" % H] = ((lambda: seqpack.emb_pos_bwd_packed(ds, pack.cu, B, S, gp)),
                                           2 * H * (T + 2 * S))
    iters = {}
    for k, (fn, _) in rows.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        iters[k] = max(10, int(50.0 / max(_window(lambda i: fn(), 10), 1e-4)))  # ~50 ms windows
    tk = {k: [] for k in rows}
    for _ in range(a.rounds):
        for k, (fn, _) in rows.items():
            tk[k].append(_window(lambda i: fn(), iters[k]))
    lines += ["Row kernels alone (B = %d, S = %d, T = %d, T_alloc = %d):" % (B, S, T, Ta), "",
              "| kernel | us (min..max) | MB | TB/s | of the %.2f TB/s copy rate |" % COPY_TBS, "|---|---|---|---|---|"]
    for k, (_, nbytes) in rows.items():
        m = statistics.median(tk[k])
        rate = nbytes / (m * 1e-3) / 1e12
        lines.append("| %s | %.1f (%.1f..%.1f) | %.1f | %.2f | %.2f |" % (k, m * 1e3, min(tk[k]) * 1e3,
                                                                         max(tk[k]) * 1e3, nbytes / 1e6, rate,
                                                                         rate / COPY_TBS))
        print(json.dumps({"kernel": k, "us": m * 1e3, "bytes": nbytes, "tbs": rate}), flush=True)
    L = cfg.layers
    per_step = L * sum(statistics.median(tk[k]) for k in rows if k.startswith("seq_")) + \
        statistics.median(tk["seq_pad W=%d" % H])
    lines += ["", "Re-padding per step: %d layers x (pad qkv + unpad ctx forward, pad dO + unpad dQKV backward) + one "
              "pad before the heads (its backward unpad not counted) = %.3f ms of kernel time when run alone, %.1f %% "
              "of the packed step with attention re-padded" % (L, per_step, 100 * per_step / med[repad]), ""]

    # ---- attention alone: the packed kernels against pad + padded kernel + unpad ----
    nh, p_a, s_a = cfg.heads, cfg.attn_dropout, 99
    if seqpack.attn_packed_supported(S, 64):
        pfwd, pbwd = seqpack.attn_packed_fwd, seqpack.attn_packed_bwd
    elif seqpack.attn_packed_long_supported(S, 64):  # 128 < S <= 512: the dKV + dQ backward pair
        pfwd, pbwd = seqpack.attn_packed_long_fwd, seqpack.attn_packed_long_bwd
    else:
        pfwd = pbwd = None
    if H == nh * 64 and pfwd is not None:
        L_ = lib()
        cu = pack.cu
        am = (torch.arange(S, device=dev).view(1, S) < pack.lengths.view(B, 1)).float()
        mask = mask_additive(am)
        qkv = torch.randn(Ta, 3 * H, device=dev).bfloat16()
        dcx = torch.randn(Ta, H, device=dev).bfloat16()
        cx, lse = pfwd(qkv, cu, B, S, nh, p_a, s_a)
        qp = seqpack.seq_pad(qkv, cu, B, S)
        cp, lp = L_.attn_fused_fwd(qp, mask, B, S, nh, p_a, s_a)
        db = torch.zeros(3 * H, device=dev)

        def repad_fwd():
            c, _ = L_.attn_fused_fwd(seqpack.seq_pad(qkv, cu, B, S), mask, B, S, nh, p_a, s_a)
            return seqpack.seq_unpad(c, cu, B, S, Ta)

        def repad_bwd():
            d = L_.attn_fused_bwd(qp, cp, seqpack.seq_pad(dcx, cu, B, S), lp, mask, B, S, nh, p_a, s_a, db)
            return seqpack.seq_unpad(d, cu, B, S, Ta)

        att = {"attn_packed_fwd": lambda: pfwd(qkv, cu, B, S, nh, p_a, s_a),
               "seq_pad + attn_fused_fwd + seq_unpad": repad_fwd,
               "attn_packed_bwd": lambda: pbwd(qkv, cx, dcx, lse, cu, B, S, nh, p_a, s_a, dbias=db),
               "seq_pad + attn_fused_bwd + seq_unpad": repad_bwd}
        ia, ta = {}, {k: [] for k in att}
        for k, fn in att.items():
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            ia[k] = max(10, int(50.0 / max(_window(lambda i: fn(), 10), 1e-4)))
        for _ in range(a.rounds):
            for k, fn in att.items():
                ta[k].append(_window(lambda i: fn(), ia[k]))
        ma = {k: statistics.median(v) for k, v in ta.items()}
        lines += ["Attention alone (%d heads, p = %.2f, T / (B * S) = %.4f; one layer's calls):" % (nh, p_a, T / (B * S)),
                  "", "| calls | us (min..max) |", "|---|---|"]
        for k in att:
            lines.append("| %s | %.1f (%.1f..%.1f) |" % (k, ma[k] * 1e3, min(ta[k]) * 1e3, max(ta[k]) * 1e3))
        pk = ma["attn_packed_fwd"] + ma["attn_packed_bwd"]
        rp = ma["seq_pad + attn_fused_fwd + seq_unpad"] + ma["seq_pad + attn_fused_bwd + seq_unpad"]
        lines += ["", "attn_packed_fwd + bwd = %.3f ms against %.3f ms re-padded: ratio %.3f; x %d layers = %.2f ms/step "
                  "less" % (pk, rp, pk / rp, L, L * (rp - pk)), ""]
        print(json.dumps({"attn_packed_ms": pk, "attn_repad_ms": rp, "ratio": pk / rp}), flush=True)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
