"""BERT without padding, on the GPU: the row kernels of csrc/kernels/seqpack.hip bit for bit against their PyTorch
mirrors inside NaN-filled, sentinel-fenced buffers (with the overrun guard, the clamp and the refusal of unaligned
operands), the packed fused model against the padded one and against the fp32 reference, the evaluator, the GEMM
attention fallback, the refusal of graph capture, and one loader-fed packed training step."""
import os
import sys

import numpy as np
import pytest
import torch

import dtg  # noqa: F401
from dtg.data import TokenLoader, masking_args, synthetic_token_set, write_token_meta, write_token_shards
from dtg.models import bert
from dtg.ops import lib, seqpack
from dtg.ops.mlm import mlm_mask_ref
from dtg.ops.seqpack import SeqPack
from dtg.parallel import FlatParams
from dtg.parallel.graphs import GraphedStep
from dtg.train import BertEvaluator

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bert_cases import IDS, make_rows  # noqa: E402

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
dev0 = torch.device("cuda", 0)
FENCE = 64  # sentinel rows on either side of an output
SENT = 0x4D4D  # the fence's bf16 bit pattern (a finite value no kernel writes)


def _geoms():
    g = torch.Generator().manual_seed(9)
    nine = [128, 8, 1] + torch.randint(1, 129, (6,), generator=g).tolist()
    return {"one": (1, 8, [1]), "five": (5, 64, [1, 64, 63, 2, 17]), "nine": (9, 128, nine)}


GEOMS = _geoms()


def _bits(t):
    return t.view(torch.int16)


def _fenced(rows, W):
    """-> (whole buffer, the [rows, W] view in its middle): fences of SENT, the view filled with NaN"""
    buf = torch.full(((rows + 2 * FENCE) * W,), SENT, dtype=torch.int16, device=dev).view(torch.bfloat16)
    out = buf[FENCE * W:(FENCE + rows) * W].view(rows, W)
    out.fill_(float("nan"))
    return buf, out


def _fences_intact(buf, rows, W):
    b = _bits(buf)
    return bool((b[:FENCE * W] == SENT).all()) and bool((b[(FENCE + rows) * W:] == SENT).all())


def _pack(B, S, lens):
    return SeqPack.from_lengths(torch.tensor(lens, dtype=torch.int32, device=dev), lens, S)


# ---- the row kernels == the mirrors ---------------------------------------------------------------------------------
# W: one 16-byte chunk; exactly one pass of the 64 lanes; one lane into a second pass; several passes
@pytest.mark.parametrize("W", [8, 512, 520, 2304])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_pad_unpad_equal_mirrors(W, geom):
    B, S, lens = GEOMS[geom]
    pk = _pack(B, S, lens)
    T, Ta = pk.T, pk.T_alloc
    assert pk.cu.tolist() == [0] + np.cumsum(lens).tolist()
    if geom == "five":
        assert (T, Ta) == (147, 192)  # no multiple of the 4 rows of a workgroup
    g = torch.Generator().manual_seed(W + B)
    packed = torch.randn(Ta, W, generator=g).bfloat16().to(dev)
    padded = torch.randn(B * S, W, generator=g).bfloat16().to(dev)
    # pad
    buf, out = _fenced(B * S, W)
    res = seqpack.seq_pad(packed, pk.cu, B, S, out=out)
    want = seqpack.seq_pad_ref(packed, pk.cu, B, S)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr() and torch.equal(_bits(out), _bits(want)) and _fences_intact(buf, B * S, W)
    real = torch.zeros(B, S, dtype=torch.bool)
    for b, n in enumerate(lens):
        real[b, :n] = True
    assert not _bits(out)[~real.reshape(-1).to(dev)].any()  # padding rows: exactly zero (+0)
    assert torch.equal(_bits(seqpack.seq_pad(packed, pk.cu, B, S)), _bits(want))  # the allocating form
    # unpad
    buf, out = _fenced(Ta, W)
    seqpack.seq_unpad(padded, pk.cu, B, S, Ta, out=out)
    want = seqpack.seq_unpad_ref(padded, pk.cu, B, S, Ta)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want)) and _fences_intact(buf, Ta, W)
    assert not _bits(out)[T:].any()  # tail rows: exactly zero
    # round trip
    back = seqpack.seq_unpad(seqpack.seq_pad(packed, pk.cu, B, S), pk.cu, B, S, Ta)
    assert torch.equal(_bits(back[:T]), _bits(packed[:T])) and not _bits(back[T:]).any()
    # the overrun guard: T_alloc 64 too small -> the rows beyond it are neither read nor written, the call returns
    if Ta > 64:
        small = Ta - 64
        buf, out = _fenced(small, W)
        seqpack.seq_unpad(padded, pk.cu, B, S, small, out=out)
        torch.cuda.synchronize()
        assert _fences_intact(buf, small, W)
        assert torch.equal(_bits(out), _bits(seqpack.seq_unpad_ref(padded, pk.cu, B, S, small)))
        assert torch.equal(_bits(out), _bits(want[:small]))
        cut, src = _fenced(small, W)  # the source ends in a fence of its own: reading past it would show
        src.copy_(packed[:small])
        buf, out = _fenced(B * S, W)
        seqpack.seq_pad(src, pk.cu, B, S, out=out)
        torch.cuda.synchronize()
        w2 = seqpack.seq_pad_ref(packed[:small], pk.cu, B, S)
        assert torch.equal(_bits(out), _bits(w2)) and _fences_intact(buf, B * S, W)
        assert not (_bits(out) == SENT).all(1).any()


def test_out_of_range_lengths_are_clamped():
    S, W = 16, 72
    lens = torch.tensor([0, S + 5, -3, 7, S, 1], dtype=torch.int32, device=dev)
    cu = seqpack.seq_offsets(lens, S)
    assert cu.tolist() == [0, 0, 16, 16, 23, 39, 40] and torch.equal(cu.cpu(), seqpack.seq_offsets_ref(lens.cpu(), S))
    pk = SeqPack.from_lengths(lens, lens.tolist(), S)
    assert (pk.T, pk.T_alloc) == (40, 64)
    g = torch.Generator().manual_seed(1)
    packed = torch.randn(64, W, generator=g).bfloat16().to(dev)
    padded = torch.randn(6 * S, W, generator=g).bfloat16().to(dev)
    assert torch.equal(_bits(seqpack.seq_pad(packed, cu, 6, S)), _bits(seqpack.seq_pad_ref(packed, cu, 6, S)))
    buf, out = _fenced(64, W)
    seqpack.seq_unpad(padded, cu, 6, S, 64, out=out)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(seqpack.seq_unpad_ref(padded, cu, 6, S, 64))) and _fences_intact(buf, 64, W)
    # offsets that do not come from seq_offsets (a record longer than S, a negative one): clamped where they are used
    bad = torch.tensor([0, S + 9, S + 4, 60], dtype=torch.int32, device=dev)
    buf, out = _fenced(3 * S, W)
    seqpack.seq_pad(packed, bad, 3, S, out=out)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(seqpack.seq_pad_ref(packed, bad, 3, S))) and _fences_intact(buf, 3 * S, W)
    assert torch.equal(_bits(out[:S]), _bits(packed[:S])) and not _bits(out[S:2 * S]).any()


def test_unaligned_operands_are_refused():
    """the documented choice (ops/seqpack.py, seqpack_ops.cc): no scalar path; a width that is no multiple of 8, a base
    that is not 16-byte aligned or a non-contiguous view raises with a message that names the reason"""
    B, S, lens = GEOMS["five"]
    pk = _pack(B, S, lens)
    flat = torch.zeros(pk.T_alloc * 16 + 8, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        seqpack.seq_pad(flat[1:1 + pk.T_alloc * 16].view(pk.T_alloc, 16), pk.cu, B, S)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        seqpack.seq_pad(torch.zeros(pk.T_alloc, 12, dtype=torch.bfloat16, device=dev), pk.cu, B, S)
    with pytest.raises(RuntimeError, match="contiguous"):
        seqpack.seq_unpad(torch.zeros(B * S, 16, dtype=torch.bfloat16, device=dev)[:, :8], pk.cu, B, S, pk.T_alloc)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        seqpack.seq_unpad(torch.zeros(B * S, 16, dtype=torch.bfloat16, device=dev), pk.cu, B, S, pk.T_alloc,
                          out=flat[3:3 + pk.T_alloc * 16].view(pk.T_alloc, 16))
    torch.cuda.synchronize()
    # the autograd forms make their operand contiguous first, so a strided view works through them
    x = torch.randn(pk.T_alloc, 16, device=dev).bfloat16()
    assert torch.equal(seqpack.pad_rows(x[:, :8], pk), seqpack.seq_pad_ref(x[:, :8].contiguous(), pk.cu, B, S))


@pytest.mark.parametrize("B", [1, 64, 65, 257, 1025])
def test_seq_offsets_against_cumsum(B):
    S = 128
    g = torch.Generator().manual_seed(B)
    lens = torch.randint(-4, S + 6, (B,), generator=g, dtype=torch.int32)
    cu = seqpack.seq_offsets(lens.to(dev), S)
    want = np.concatenate([[0], np.cumsum(np.clip(lens.numpy().astype(np.int64), 0, S))])
    assert cu.dtype == torch.int32 and cu.shape == (B + 1,) and cu.cpu().tolist() == want.tolist()


@pytest.mark.parametrize("geom,H", [("one", 8), ("five", 520), ("nine", 128), ("nine", 2304)])
def test_packed_embeddings_and_ids(geom, H):
    """emb_fwd_packed == seq_unpad(emb_fwd(padded)) bit for bit (the same sum in the same order), with and without
    token types; seq_gather_ids == its mirror, tail id 0"""
    B, S, lens = GEOMS[geom]
    pk = _pack(B, S, lens)
    g = torch.Generator().manual_seed(H + B)
    word, pos, typ = (torch.randn(n, H, generator=g).bfloat16().to(dev) for n in (300, S + 2, 2))
    ids = torch.randint(0, 300, (B, S), generator=g).to(dev)
    tt = torch.randint(0, 2, (B, S), generator=g).to(dev)
    for t in (tt, None):
        padded = lib().emb_fwd(ids.reshape(-1), None if t is None else t.reshape(-1), word, pos, typ, S)
        want = seqpack.seq_unpad(padded, pk.cu, B, S, pk.T_alloc)
        buf, out = _fenced(pk.T_alloc, H)
        seqpack.emb_fwd_packed(ids, t, word, pos, typ, pk.cu, pk.T_alloc, out=out)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want)) and _fences_intact(buf, pk.T_alloc, H)
        assert not _bits(out)[pk.T:].any()
        assert torch.equal(_bits(out), _bits(seqpack.emb_fwd_packed_ref(ids, t, word, pos, typ, pk.cu, pk.T_alloc)))
    io, to = seqpack.seq_gather_ids(ids, tt, pk.cu, pk.T_alloc)
    wi, wt = seqpack.seq_gather_ids_ref(ids.cpu(), tt.cpu(), pk.cu.cpu(), pk.T_alloc)
    assert torch.equal(io.cpu(), wi) and torch.equal(to.cpu(), wt) and not io[pk.T:].any()
    assert seqpack.seq_gather_ids(ids, None, pk.cu, pk.T_alloc)[1] is None
    if pk.T_alloc > 64:  # the guard
        small = pk.T_alloc - 64
        i2, _ = seqpack.seq_gather_ids(ids, tt, pk.cu, small)
        assert torch.equal(i2.cpu(), seqpack.seq_gather_ids_ref(ids.cpu(), tt.cpu(), pk.cu.cpu(), small)[0])
        buf, out = _fenced(small, H)
        seqpack.emb_fwd_packed(ids, tt, word, pos, typ, pk.cu, small, out=out)
        torch.cuda.synchronize()
        assert _fences_intact(buf, small, H)
        assert torch.equal(_bits(out), _bits(seqpack.emb_fwd_packed_ref(ids, tt, word, pos, typ, pk.cu, small)))


@pytest.mark.parametrize("geom,H", [("one", 8), ("five", 520), ("nine", 128), ("nine", 2304)])
def test_packed_position_gradient(geom, H):
    """gP[p] += sum over the records that reach p, against an fp64 sum per position.  The bound, per element: the
    kernel adds n = (records reaching p) + 1 terms (the rows and gP's old value) in fp32 in some fixed order, so its
    fp32 sum s obeys |s - exact| <= gamma * sum|terms| with gamma = (n - 1) u / (1 - (n - 1) u), u = 2^-24 (Higham,
    Accuracy and Stability, eq. 4.4: any order); the store rounds s to bf16 once, |bf(s) - s| <= 2^-8 |s|.  Hence
    |got - exact| <= 2^-8 (|exact| + e1) + e1 with e1 = gamma * sum|terms|."""
    B, S, lens = GEOMS[geom]
    pk = _pack(B, S, lens)
    g = torch.Generator().manual_seed(H * 3 + B)
    ds = torch.randn(pk.T_alloc, H, generator=g).bfloat16().to(dev)
    for prefill in (False, True):
        buf, gP = _fenced(S + 3, H)
        gP.copy_(torch.randn(S + 3, H, generator=g).bfloat16() if prefill else torch.zeros(S + 3, H))
        old = gP.clone()
        seqpack.emb_pos_bwd_packed(ds, pk.cu, B, S, gP)
        torch.cuda.synchronize()
        assert _fences_intact(buf, S + 3, H) and torch.equal(_bits(gP[S:]), _bits(old[S:]))
        rows = seqpack.seq_pad_ref(ds.cpu().double(), pk.cu.cpu(), B, S).view(B, S, H)
        exact = old[:S].cpu().double() + rows.sum(0)
        mag = old[:S].cpu().double().abs() + rows.abs().sum(0)
        n = torch.tensor([sum(1 for m in lens if m > p) + 1 for p in range(S)], dtype=torch.float64).view(S, 1)
        u = 2.0 ** -24
        e1 = (n - 1) * u / (1 - (n - 1) * u) * mag
        bound = 2.0 ** -8 * (exact.abs() + e1) + e1
        err = (gP[:S].cpu().double() - exact).abs()
        print("[emb_pos_bwd_packed] %s H=%d prefill=%s: worst err / bound %.3f" % (
            geom, H, prefill, (err / bound.clamp(min=1e-300)).max().item()))
        assert bool((err <= bound).all())
        # no record reaches the position: the old value, untouched
        none = [p for p in range(S) if all(m <= p for m in lens)]
        assert torch.equal(_bits(gP[none]), _bits(old[none]))
        # a second launch on the same inputs: the order over b is fixed, so the bits repeat
        again = old.clone()
        seqpack.emb_pos_bwd_packed(ds, pk.cu, B, S, again)
        assert torch.equal(_bits(again), _bits(gP))


# ---- the model ------------------------------------------------------------------------------------------------------
PRED = 10
CFG = dict(vocab_size=1024, hidden=128, layers=2, heads=2, intermediate=512, max_position=128)
_rel = lambda a, b: ((a - b).norm() / (b.norm() + 1e-12)).item()  # noqa: E731


def _model(seed=0, **over):
    torch.manual_seed(seed)
    model = bert.BertForPreTraining(bert.BertConfig(**dict(CFG, **over))).to(dev)
    with torch.no_grad():  # biases and LayerNorm parameters away from (0, 1): an omitted one would show
        for n, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    return model, FlatParams(model)


def _ref_model(model, noise=0.0, seed=11):
    """the reference path in fp32 on the CPU with the weights as the bf16 mirror holds them; noise: relative weight
    noise, the matrices rounded to bf16 again"""
    g = torch.Generator().manual_seed(seed)
    ref = bert.BertForPreTraining(bert.BertConfig(**{k: getattr(model.cfg, k) for k in (
        "vocab_size", "hidden", "layers", "heads", "intermediate", "max_position", "dropout", "attn_dropout")}))
    state = {}
    for n, p in model.named_parameters():
        t = p.detach().float().cpu().clone()
        if noise:
            t = t * (1 + noise * torch.randn(t.shape, generator=g))
            t = t.bfloat16().float() if p.dim() > 1 else t
        state[n] = t
    ref.load_state_dict(state)
    return ref.train()


def _batch(B, S, lens, seed):
    rows = make_rows(B, S, seed=seed, lengths=lens)
    ids, tt, am, pos, lab = mlm_mask_ref(*rows, seed=1, epoch=0, P=PRED, **IDS)
    nsp = torch.tensor([(b * 7 + seed) % 2 for b in range(B)])
    return (ids, tt, am, pos, lab, nsp), max(1, int((lab >= 0).sum())), rows[2]


def _step(model, flat, batch, nv, pack, step=5):
    """forward + backward -> (loss fp32, flat gradient fp32 in named_parameters order)"""
    model._step = step
    if flat is not None:
        flat.zero_grad()
    else:
        model.zero_grad()
    loss = model(*batch, num_valid=nv, pack=pack)
    loss.backward()
    if batch[0].is_cuda:
        torch.cuda.synchronize()
    return loss.detach().float().cpu().clone(), torch.cat([p.grad.detach().float().reshape(-1).cpu()
                                                           for _, p in model.named_parameters()])


@pytest.mark.parametrize("S", [128, 64])
def test_full_lengths_packed_equals_padded_bitwise(S):
    """all lengths S, dropout on, fixed ``_step``: the packed rows ARE the padded rows (T_alloc = B * S, the same M,
    the same dropout indices) and the forward has no atomics, so the loss is the same bits; the gradients agree up to
    the order of the atomic sums (one bf16 rounding, 2^-8: the bound of
    test_bert_data_gpu.py::test_training_step_fed_by_the_loader)"""
    model, flat = _model(seed=2)
    model.train()
    batch, nv, lengths = _batch(8, S, [S] * 8, seed=3)
    batch = tuple(t.to(dev) for t in batch)
    pack = SeqPack.from_lengths(lengths.to(dev), lengths.tolist(), S)
    assert model.fused_ok(batch[0]) and model.cfg.dropout > 0 and (pack.T, pack.T_alloc) == (8 * S, 8 * S)
    l0, g0 = _step(model, flat, batch, nv, None)
    l1, g1 = _step(model, flat, batch, nv, pack)
    e = _rel(g1, g0)
    print("[unpad full lengths] S=%d loss %.6f / %.6f, grad rel diff %.3e, |grad| %.4f" % (S, l0, l1, e, g0.norm()))
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all() and g0.norm() > 0
    assert torch.equal(l0, l1)
    assert e <= 2.0 ** -8


MIXED = [8, 128, 77, 128, 9, 50, 101, 33]


@pytest.fixture(scope="module")
def mixed():
    """mixed lengths including 8 and S, dropout 0: the batch, the fused model, and the fp32 padded reference's loss
    and gradient with and without 2^-9 relative weight noise (computed once, shared)"""
    model, flat = _model(seed=4, dropout=0.0, attn_dropout=0.0)
    model.train()
    batch, nv, lengths = _batch(8, 128, MIXED, seed=6)
    ref = _step(_ref_model(model), None, batch, nv, None)
    noisy = _step(_ref_model(model, noise=2 ** -9), None, batch, nv, None)
    return model, flat, batch, nv, lengths, ref, noisy


def test_mixed_lengths_match_fp32_reference(mixed):
    """loss and flat gradient of the packed fused path against the fp32 PADDED reference model, under the project's
    noise-floor rule: within 1.6 x the reference's own movement under 2^-9 relative weight noise, plus 0.02.  A wrong
    offset, a missed zero row or a dropped tail moves the gradient by its own size."""
    model, flat, batch, nv, lengths, (rl, rg), (nl, ng) = mixed
    d = tuple(t.to(dev) for t in batch)
    pack = SeqPack.from_lengths(lengths.to(dev), lengths.tolist(), 128)
    assert model.fused_ok(d[0]) and pack.T == sum(MIXED) and pack.T_alloc == 576
    pl, pg = _step(model, flat, d, nv, pack)
    dl, dg = _step(model, flat, d, nv, None)
    e_l, e_g = abs((pl - rl) / rl).item(), _rel(pg, rg)
    n_l, n_g = abs((nl - rl) / rl).item(), _rel(ng, rg)
    print("[unpad mixed] loss: packed %.6f padded fused %.6f fp32 ref %.6f; rel err packed %.5f, padded fused %.5f, "
          "ref under noise %.5f (bound %.5f)" % (pl, dl, rl, e_l, abs((dl - rl) / rl).item(), n_l, 1.6 * n_l + 0.02))
    print("[unpad mixed] gradient: rel err packed %.4f, padded fused %.4f, ref under noise %.4f (bound %.4f); packed "
          "against padded fused %.4f" % (e_g, _rel(dg, rg), n_g, 1.6 * n_g + 0.02, _rel(pg, dg)))
    assert torch.isfinite(pg).all() and e_l <= 1.6 * n_l + 0.02 and e_g <= 1.6 * n_g + 0.02
    # and per parameter, so that a small tensor (a bias, the position table) cannot hide in the flat norm
    o = 0
    for (name, p) in model.named_parameters():
        n = p.numel()
        a, r, z = pg[o:o + n], rg[o:o + n], ng[o:o + n]
        o += n
        assert _rel(a, r) <= 1.6 * _rel(z, r) + 0.02, (name, _rel(a, r), _rel(z, r))
    # the reference path takes the pack too: on the card in fp32 it is the padded reference up to fp32 rounding
    ref32 = _ref_model(model).to(dev)
    ql, qg = _step(ref32, None, d, nv, pack)
    assert abs((ql - rl) / rl).item() <= 1e-4 and _rel(qg, rg) <= 1e-3


def test_pretraining_logits_packed(mixed):
    model, flat, batch, nv, lengths, _, _ = mixed
    ids, tt, am, pos = batch[:4]
    d = [t.to(dev) for t in (ids, tt, am, pos)]
    pack = SeqPack.from_lengths(lengths.to(dev), lengths.tolist(), 128)
    step = model._step
    with torch.no_grad():
        got = model.pretraining_logits(*d, pack=pack)
        padded = model.pretraining_logits(*d)
        ref = _ref_model(model).pretraining_logits(ids, tt, am, pos)
        noisy = _ref_model(model, noise=2 ** -9).pretraining_logits(ids, tt, am, pos)
    torch.cuda.synchronize()
    assert model._step == step and got[0].shape == (8 * PRED, 1024) and got[1].shape == (8, 2)
    for name, a, p, r, z in zip(("mlm", "nsp"), got, padded, ref, noisy):
        e, e_pad, e_noise = _rel(a.float().cpu(), r), _rel(p.float().cpu(), r), _rel(z, r)
        print("[unpad eval logits] %s: rel err packed %.4f, padded fused %.4f; fp32 reference under 2^-9 weight noise "
              "%.4f (bound %.4f)" % (name, e, e_pad, e_noise, 1.6 * e_noise + 0.02))
        assert torch.isfinite(a.float()).all() and e <= 1.6 * e_noise + 0.02


def test_gemm_attention_fallback_runs_packed():
    """head dim 32: no fused attention, the batched-GEMM attention runs between the pad and the unpad; same rule"""
    model, flat = _model(seed=5, hidden=64, heads=2, intermediate=256, dropout=0.0, attn_dropout=0.0)
    model.train()
    S, lens = 64, [8, 64, 30, 64, 1, 17, 45, 2]
    batch, nv, lengths = _batch(8, S, lens, seed=8)
    d = tuple(t.to(dev) for t in batch)
    assert model.fused_ok(d[0]) and not lib().attn_fused_supported(S, 32, True)
    pack = SeqPack.from_lengths(lengths.to(dev), lens, S)
    pl, pg = _step(model, flat, d, nv, pack)
    rl, rg = _step(_ref_model(model), None, batch, nv, None)
    nl, ng = _step(_ref_model(model, noise=2 ** -9), None, batch, nv, None)
    e_l, e_g, n_l, n_g = abs((pl - rl) / rl).item(), _rel(pg, rg), abs((nl - rl) / rl).item(), _rel(ng, rg)
    print("[unpad gemm attention] loss %.6f ref %.6f; rel err loss %.5f (noise %.5f) gradient %.4f (noise %.4f)" % (
        pl, rl, e_l, n_l, e_g, n_g))
    assert torch.isfinite(pg).all() and e_l <= 1.6 * n_l + 0.02 and e_g <= 1.6 * n_g + 0.02


def test_graphed_step_refuses_a_packed_step(mixed):
    model, flat, batch, nv, lengths, _, _ = mixed
    d = tuple(t.to(dev) for t in batch)
    pack = SeqPack.from_lengths(lengths.to(dev), lengths.tolist(), 128)
    with pytest.raises(RuntimeError, match="packed step"):
        GraphedStep(lambda: model(*d, num_valid=nv, pack=pack)).capture()
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.isfinite(model(*d, num_valid=nv, pack=pack).float())  # eager: still fine afterwards


# ---- loader and evaluator ---------------------------------------------------------------------------------------------
SEQ, VOCAB = 64, 1000
META = dict(pad_id=0, cls_id=1, sep_id=2, mask_id=3, vocab_lo=4, vocab_hi=VOCAB)


@pytest.fixture(scope="module")
def token_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("tokens_unpad_gpu")
    write_token_shards(str(d), synthetic_token_set(70, seq=SEQ, vocab_hi=VOCAB, seed=4), 32)
    write_token_meta(str(d), **META)
    return str(d)


def _loader(d, batch, device, **kw):
    return TokenLoader(d, batch, device, P=PRED, **masking_args(META), **kw)


def test_evaluator_unpad_scores_the_same_records(token_dir):
    """70 records at batch 8: the packed pass scores the same records and the same predictions (n, mlm_n, bad labels
    and non-finite rows are equal), with logits that differ from the padded pass in rounding only -- so a verdict
    (is the label among the top k; is the pair class right) may flip where two logits tie within a rounding.  The cap
    on the rows whose verdict the packed pass may take out of (or add to) a count: 2 % of the rows scored."""
    model, _ = _model(seed=1)
    ks = (1, 5)
    res = {}
    for unpad in (False, True):
        with _loader(token_dir, 8, dev0, train=False, drop_last=False, eval_seed=3, pack=unpad) as loader:
            res[unpad] = BertEvaluator(model, loader, ks=ks, unpad=unpad).run()
    a, b = res[False], res[True]
    print("[unpad evaluator] padded %s\n[unpad evaluator] packed %s" % (
        {k: v for k, v in a.items() if "sec" not in k}, {k: v for k, v in b.items() if "sec" not in k}))
    assert a["n"] == b["n"] == 70 and a["mlm_n"] == b["mlm_n"] > 70
    assert a["bad_labels"] == b["bad_labels"] == 0 and a["nonfinite"] == b["nonfinite"] == 0
    for k in ks:
        assert abs(a["mlm_top%d_count" % k] - b["mlm_top%d_count" % k]) <= 0.02 * a["mlm_n"]
    assert abs(a["nsp_correct"] - b["nsp_correct"]) <= 0.02 * a["n"]
    assert np.isfinite(b["mlm_loss"]) and np.isfinite(b["nsp_loss"])


def test_packed_training_step_fed_by_the_loader(token_dir):
    """one forward + backward on a ``TokenLoader(pack=True)`` batch on the card: finite, and the same loss bits as the
    step fed with the CPU loader's tensors and pack (the same inputs; the forward has no atomics)"""
    model, flat = _model(seed=2)
    model.train()
    with _loader(token_dir, 8, dev0, seed=9, pack=True) as gpu, _loader(token_dir, 8, "cpu", seed=9, pack=True) as cpu:
        gpu.seek(2)
        cpu.seek(2)
        batch, nv, idx, pack = gpu.next()
        mirror, nv_c, idx_c, pack_c = cpu.next()
    assert nv == nv_c and torch.equal(idx, idx_c) and pack.cu.is_cuda and pack.lengths.is_cuda
    assert (pack.T, pack.T_alloc) == (pack_c.T, pack_c.T_alloc) and pack.T < 8 * SEQ
    assert torch.equal(pack.cu.cpu(), pack_c.cu) and torch.equal(pack.lengths.cpu(), pack_c.lengths)
    assert torch.equal(pack.lengths.long(), batch[2].sum(1))
    moved = SeqPack.from_lengths(pack_c.lengths.to(dev), pack_c.host_lengths, SEQ)
    l0, g0 = _step(model, flat, batch, nv, pack)
    l1, g1 = _step(model, flat, tuple(t.to(dev) for t in mirror), nv, moved)
    e = _rel(g0, g1)
    print("[unpad loader step] T %d of %d rows (T_alloc %d), loss %.6f / %.6f, grad rel diff %.3e" % (
        pack.T, 8 * SEQ, pack.T_alloc, l0, l1, e))
    assert torch.isfinite(l0).all() and torch.isfinite(g0).all() and g0.norm() > 0
    assert torch.equal(l0, l1) and e <= 2.0 ** -8
    # micro-batches: the chunks' packs drive two half-batch steps
    for i in range(2):
        half = tuple(t[i * 4:(i + 1) * 4] for t in batch)
        li, _ = _step(model, flat, half, nv / 2, pack.chunk(i, 2))
        assert torch.isfinite(li).all()
