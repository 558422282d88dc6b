"""BERT without padding, on the CPU: the PyTorch mirrors of ops/seqpack.py against per-row Python loops, the packed
reference path of the model against the padded one in fp64, ``TokenLoader(pack=True)``, and ``bert_train.py --unpad`` /
``bert_eval.py --unpad`` end to end with a stop/resume and with gradient accumulation."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dtg
from dtg.data import TokenLoader, masking_args, synthetic_token_set, write_token_meta, write_token_shards
from dtg.models import bert
from dtg.ops import seqpack
from dtg.ops.mlm import mlm_mask_ref
from dtg.ops.seqpack import SeqPack

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bert_cases import IDS, make_rows  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = (1, 64, 63, 2, 17)


def _lengths(B, S, kind):
    if kind == "one":
        return [1] * B
    if kind == "full":
        return [S] * B
    return [min(n, S) for n in FIVE[:B]]


def _cases():
    for B in (1, 5):
        for S in (8, 64):
            for kind in ("one", "full", "five"):
                if kind == "five" and B != 5:
                    continue
                for W in (8, 72):
                    yield B, S, kind, W


# ---- the mirrors against per-row loops --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,kind,W", list(_cases()))
def test_mirrors_against_row_loops(B, S, kind, W):
    lens = _lengths(B, S, kind)
    T = sum(lens)
    T_alloc = max(64, -(-T // 64) * 64)
    cu = seqpack.seq_offsets_ref(torch.tensor(lens, dtype=torch.int32), S)
    assert cu.dtype == torch.int32 and cu.tolist() == [0] + np.cumsum(lens).tolist()
    g = torch.Generator().manual_seed(B * 100 + S + W)
    packed = torch.randn(T_alloc, W, generator=g)
    padded = torch.randn(B * S, W, generator=g)
    # pad: row by row
    want = torch.zeros(B * S, W)
    for b in range(B):
        for s in range(lens[b]):
            want[b * S + s] = packed[int(cu[b]) + s]
    got = seqpack.seq_pad_ref(packed, cu, B, S)
    assert torch.equal(got, want)
    # unpad: row by row, zero tail
    want_u = torch.zeros(T_alloc, W)
    for b in range(B):
        for s in range(lens[b]):
            want_u[int(cu[b]) + s] = padded[b * S + s]
    got_u = seqpack.seq_unpad_ref(padded, cu, B, S, T_alloc)
    assert torch.equal(got_u, want_u) and not got_u[T:].any()
    # unpad(pad(x)) == x on the real rows, zeros elsewhere
    back = seqpack.seq_unpad_ref(got, cu, B, S, T_alloc)
    assert torch.equal(back[:T], packed[:T]) and not back[T:].any()
    # ids: the same rows, tail id 0
    ids = torch.randint(1, 50, (B, S), generator=g)
    tt = torch.randint(0, 2, (B, S), generator=g)
    io, to = seqpack.seq_gather_ids_ref(ids, tt, cu, T_alloc)
    for b in range(B):
        assert io[int(cu[b]):int(cu[b + 1])].tolist() == ids[b, :lens[b]].tolist()
        assert to[int(cu[b]):int(cu[b + 1])].tolist() == tt[b, :lens[b]].tolist()
    assert io.shape == (T_alloc,) and not io[T:].any() and not to[T:].any()
    # position gradient: per position, the rows of the sequences that reach it; added into gP
    gP = torch.randn(S + 3, W, generator=g)
    want_p = gP.clone()
    for p in range(S):
        for b in range(B):
            if lens[b] > p:
                want_p[p] += packed[int(cu[b]) + p]
    seqpack.emb_pos_bwd_packed_ref(packed, cu, B, S, gP)
    assert torch.allclose(gP, want_p, rtol=1e-6, atol=1e-6) and torch.equal(gP[S:], want_p[S:])
    # the packed embedding sum: unpad of the padded one
    word, pos, typ = (torch.randn(n, W, generator=g) for n in (50, S, 2))
    e = seqpack.emb_fwd_packed_ref(ids, tt, word, pos, typ, cu, T_alloc)
    for b in range(B):
        for s in range(lens[b]):
            assert torch.equal(e[int(cu[b]) + s], word[ids[b, s]] + (pos[s] + typ[tt[b, s]]))
    assert not e[T:].any()


def test_offsets_clamp_and_overrun_guard():
    S = 16
    lens = torch.tensor([0, S + 5, -3, 7, S, 1], dtype=torch.int32)
    cu = seqpack.seq_offsets_ref(lens, S)
    assert cu.tolist() == [0, 0, 16, 16, 23, 39, 40]
    assert torch.equal(seqpack.seq_offsets(lens, S), cu)  # the op on CPU tensors is the mirror
    # a T_alloc too small for the offsets: the rows beyond it are skipped, nothing fails
    x = torch.arange(6 * S * 8, dtype=torch.float32).view(6 * S, 8)
    short = seqpack.seq_unpad_ref(x, cu, 6, S, 24)
    full = seqpack.seq_unpad_ref(x, cu, 6, S, 64)
    assert short.shape == (24, 8) and torch.equal(short, full[:24])
    back = seqpack.seq_pad_ref(short, cu, 6, S)
    want = seqpack.seq_pad_ref(full, cu, 6, S)
    keep = torch.zeros(6 * S, dtype=torch.bool)
    keep[:2 * S] = True                # records 0 and 1 lie below row 16
    keep[3 * S:3 * S + 7] = True       # record 3: rows 16 .. 22
    keep[4 * S] = True                 # record 4: row 23 only
    assert torch.equal(back[keep], want[keep]) and not back[~keep].any()


def test_pad_unpad_autograd_are_each_others_backward():
    S, lens = 8, [3, 8, 1]
    pack = SeqPack.from_lengths(torch.tensor(lens, dtype=torch.int32), lens, S)
    assert (pack.B, pack.S, pack.T, pack.T_alloc) == (3, 8, 12, 64)
    x = torch.randn(64, 8, dtype=torch.float64, requires_grad=True)
    w = torch.randn(24, 8, dtype=torch.float64)
    (seqpack.pad_rows(x, pack) * w).sum().backward()
    assert torch.equal(x.grad, seqpack.seq_unpad_ref(w, pack.cu, 3, S, 64)) and not x.grad[12:].any()
    y = torch.randn(24, 8, dtype=torch.float64, requires_grad=True)
    v = torch.randn(64, 8, dtype=torch.float64)
    (seqpack.unpad_rows(y, pack) * v).sum().backward()
    assert torch.equal(y.grad, seqpack.seq_pad_ref(v, pack.cu, 3, S))
    with pytest.raises(ValueError):
        seqpack.pad_rows(y, pack)
    with pytest.raises(ValueError):
        pack.chunk(0, 2)  # 3 records do not split in two


# ---- the model: packed reference path == padded reference path --------------------------------------------------------
def test_packed_reference_model_equals_padded_in_fp64():
    """tiny config, dropout 0, batch 6, lengths including 8 and S, fp64: the packed path computes the same function
    of the real rows, so loss and every parameter gradient agree to 1e-9 relative (fp64 rounding of a few hundred
    operations lies orders of magnitude below)."""
    cfg = bert.BertConfig.tiny()
    cfg.dropout = cfg.attn_dropout = 0.0
    S, P = 32, 5
    torch.manual_seed(3)
    model = bert.BertForPreTraining(cfg).double()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    model.train()
    lens = [8, S, 13, 9, S, 20]
    rows = make_rows(6, S, seed=5, lengths=lens)
    ids, tt, am, pos, lab = mlm_mask_ref(*rows, seed=1, epoch=0, P=P, **IDS)
    ids = ids % cfg.vocab_size
    lab = torch.where(lab >= 0, lab % cfg.vocab_size, lab)
    nsp = torch.tensor([0, 1, 1, 0, 1, 0])
    nv = max(1, int((lab >= 0).sum()))
    pack = SeqPack.from_lengths(rows[2], lens, S)
    assert pack.T == sum(lens) and pack.T_alloc == 128 and torch.equal(pack.lengths.long(), am.sum(1))
    out = {}
    for name, pk in (("padded", None), ("packed", pack)):
        model.zero_grad()
        loss = model(ids, tt, am, pos, lab, nsp, num_valid=nv, pack=pk)
        assert loss.dtype == torch.float64
        loss.backward()
        out[name] = (loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()})
    (l0, g0), (l1, g1) = out["padded"], out["packed"]
    rel = abs((l1 - l0) / l0).item()
    worst = max((((g1[n] - g0[n]).norm() / (g0[n].norm() + 1e-300)).item(), n) for n in g0)
    print("[unpad cpu fp64] loss %.12f / %.12f rel %.2e; worst gradient rel %.2e (%s)" % (l0, l1, rel, *worst))
    assert all(g0[n].norm() > 0 for n in g0)
    assert rel <= 1e-9 and worst[0] <= 1e-9
    # set_seq_pack serves callers that cannot pass pack=: the same loss; a pack of another batch shape is refused
    model.set_seq_pack(pack)
    with torch.no_grad():
        assert torch.equal(model(ids, tt, am, pos, lab, nsp, num_valid=nv), l1)
        with pytest.raises(ValueError, match="pack describes"):
            model(ids[:4], tt[:4], am[:4], pos[:4], lab[:4], nsp[:4])
        model.set_seq_pack(None)
        assert torch.equal(model(ids, tt, am, pos, lab, nsp, num_valid=nv), l0)
        # the evaluation forward takes the pack too
        a, b = model.pretraining_logits(ids, tt, am, pos), model.pretraining_logits(ids, tt, am, pos, pack=pack)
    valid = lab.reshape(-1) >= 0
    assert ((a[0][valid] - b[0][valid]).norm() / a[0][valid].norm()).item() <= 1e-9
    assert ((a[1] - b[1]).norm() / a[1].norm()).item() <= 1e-9


# ---- the loader ---------------------------------------------------------------------------------------------------------
VOCAB = 68
META = dict(pad_id=0, cls_id=1, sep_id=2, mask_id=3, vocab_lo=4, vocab_hi=VOCAB)


@pytest.fixture(scope="module")
def token_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tokens_unpad"))
    write_token_shards(d, synthetic_token_set(48, seq=32, vocab_hi=VOCAB, seed=1, strides=(1, 2, 3, 5)), 20)
    write_token_meta(d, **META)
    return d


def test_loader_returns_the_pack(token_dir):
    kw = dict(P=5, seed=2, **masking_args(META))
    with TokenLoader(token_dir, 8, "cpu", pack=True, **kw) as packed, TokenLoader(token_dir, 8, "cpu", **kw) as plain:
        for _ in range(3):
            batch, nv, idx, pack = packed.next()
            ref = plain.next()
            assert len(ref) == 3 and ref[1] == nv and torch.equal(ref[2], idx)  # the default loader: a 3-tuple
            assert all(torch.equal(a, b) for a, b in zip(batch, ref[0]))
            am = batch[2]
            assert isinstance(pack, SeqPack) and (pack.B, pack.S) == tuple(am.shape)
            assert pack.lengths.dtype == torch.int32 and torch.equal(pack.lengths.long(), am.sum(1))
            assert pack.host_lengths.tolist() == am.sum(1).tolist()
            assert pack.T == int(am.sum()) and pack.T_alloc % 64 == 0 and 0 <= pack.T_alloc - pack.T < 64
            assert pack.cu.tolist() == [0] + np.cumsum(am.sum(1).numpy()).tolist()
            for A in (1, 2, 4):
                chunks = [pack.chunk(i, A) for i in range(A)]
                assert sum(c.T for c in chunks) == pack.T and all(c.B == 8 // A and c.T_alloc % 64 == 0 for c in chunks)
                assert torch.equal(torch.cat([c.lengths for c in chunks]), pack.lengths)
                assert all(c.cu.tolist() == [0] + np.cumsum(c.host_lengths).tolist() for c in chunks)
        # nothing in the pack aliases a ring slot: later batches leave it as it was
        kept = (pack.lengths.clone(), pack.cu.clone(), pack.host_lengths.copy())
        for _ in range(4):
            packed.next()
        assert torch.equal(pack.lengths, kept[0]) and torch.equal(pack.cu, kept[1])
        assert (pack.host_lengths == kept[2]).all()
    with TokenLoader(token_dir, 8, "cpu", **kw) as plain:
        with pytest.raises(ValueError, match="pack=True"):
            dtg.data.TokenFeedHook(plain, [None] * 6, None, set_seq_pack=lambda p: None)
        with pytest.raises(ValueError, match="pack=True"):
            dtg.train.BertEvaluator(bert.BertForPreTraining(bert.BertConfig.tiny()), plain, unpad=True)


# ---- the examples, end to end -------------------------------------------------------------------------------------------
def _clean_env():
    e = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DTG_FAULT"):
        e.pop(k, None)
    return e


def _example(script, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "BERT", script), *args], capture_output=True,
                       text=True, timeout=300, env=_clean_env())
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("accum", [1, 2])
def test_bert_example_unpad_trains_resumes_and_evaluates(token_dir, tmp_path, accum):
    ck = str(tmp_path / "ck")
    args = ["--tiny", "--unpad", "--batch", "4", "--accum_steps", str(accum), "--total_steps", "4", "--warmup", "2",
            "--save_every", "2", "--log_every", "1", "--ckpt_dir", ck, "--data_dir", token_dir,
            "--max_predictions", "5", "--eval_dir", token_dir, "--eval_every", "4"]
    first = _example("bert_train.py", "--steps", "2", *args)
    second = _example("bert_train.py", "--steps", "4", *args)
    assert "done at global step 2" in first and "resumed from" not in first, first
    assert "resumed from" in second and "(global step 2)" in second and "done at global step 4" in second, second
    losses = [(int(s), float(v)) for s, v in re.findall(r"^step (\d+) loss ([-\d.naninf]+)", first + second, re.M)]
    assert [s for s, _ in losses] == [1, 2, 3, 4] and all(np.isfinite(v) and v > 0 for _, v in losses), losses
    assert re.search(r"^eval step 4: n=48 mlm_n=\d+ mlm_loss=", second, re.M), second
    if accum == 1:
        out = _example("bert_eval.py", "--tiny", "--unpad", "--ckpt_dir", ck, "--data_dir", token_dir, "--batch", "8",
                       "--max_predictions", "5")
        line = re.search(r"^eval step 4: n=48 mlm_n=(\d+) mlm_loss=([\d.]+) .*nsp_acc=([\d.]+)$", out, re.M)
        assert line and int(line.group(1)) > 0 and np.isfinite(float(line.group(2))), out
        padded = _example("bert_eval.py", "--tiny", "--ckpt_dir", ck, "--data_dir", token_dir, "--batch", "8",
                          "--max_predictions", "5")
        ref = re.search(r"^eval step 4: n=48 mlm_n=(\d+) mlm_loss=([\d.]+) ", padded, re.M)
        assert ref.group(1) == line.group(1) and abs(float(ref.group(2)) - float(line.group(2))) <= 1e-3
