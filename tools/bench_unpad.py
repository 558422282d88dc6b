#!/usr/bin/env python3
"""BERT-base with and without padding on records of mixed length (dtg.ops.seqpack): what the packed path buys.

BERT-base, batch 256 x 128, batches of ``synthetic_token_set`` records (lengths 8 .. 128, one in eight full) masked by
``mlm_mask``; forward + backward + fused AdamW step.  The padded path (``pack=None``) and the packed path
(``pack=SeqPack``) alternate over ``--rounds`` rounds on the same batches, the same weights' shapes and the same build;
each measurement is a window of ``--steps`` steps between two device events.  Reported: ms/step of both (median and
the rounds' min..max), the batches' T / (B * S), and the packed step as a share of the padded one -- the token ratio
is the bound, the distance from it is the work that still runs on padded rows (attention, the heads, the re-padding
traffic) or does not shrink with the rows (launches, the optimizer).

The four row kernels are then timed alone at this shape, with their algorithmic bytes against the 5.28 TB/s copy rate
of profiles/r05_hbm_probe (reads of real rows + writes of every output row; the position and type tables and ``cu``
stay in cache and are not counted).  Needs a GPU.

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
from dtg.models import bert  # noqa: E402
from dtg.ops import seqpack  # noqa: E402
from dtg.ops.mlm import count_valid, mlm_mask  # noqa: E402
from dtg.ops.seqpack import SeqPack  # noqa: E402
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

    def step(i, packed):
        b, nv, pack = batches[i % len(batches)]
        loss = model(*b, num_valid=nv, pack=pack if packed else None)
        if not seed:
            seed.append(torch.ones_like(loss))
        loss.backward(seed[0])
        overlap.join()
        opt.step()
        return loss

    paths = {"padded": lambda i: step(i, False), "packed": lambda i: step(i, True)}
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
    lines = ["Measured on: %s (one device, device events, %d rounds alternating padded / packed, windows of %d steps)"
             % (where, a.rounds, a.steps), "",
             "%s, batch %d x %d, %d batches of synthetic_token_set records: T / (B * S) = %.4f (T_alloc / (B * S) = "
             "%.4f)" % ("BERT-base" if not a.tiny else "2-layer BERT", B, S, len(batches), ratio, ratio_alloc), "",
             "| path | ms/step (min..max) | sequences/s |", "|---|---|---|"]
    for k in paths:
        lines.append("| %s | %.2f (%.2f..%.2f) | %.0f |" % (k, med[k], min(t[k]), max(t[k]), B / med[k] * 1e3))
    lines += ["", "packed / padded = %.4f of the step time; the bound T / (B * S) = %.4f; %.2f ms of the packed step "
              "(%.1f %% of the padded one) lie above the bound" % (share, ratio, med["packed"] - ratio * med["padded"],
                                                                  100 * (share - ratio)), ""]
    print(json.dumps({"padded_ms": med["padded"], "packed_ms": med["packed"], "padded_range": [min(t["padded"]),
                      max(t["padded"])], "packed_range": [min(t["packed"]), max(t["packed"])], "token_ratio": ratio,
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
              "of the packed step" % (L, per_step, 100 * per_step / med["packed"]), ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
