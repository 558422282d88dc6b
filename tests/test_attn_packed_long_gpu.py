"""Fused attention on packed rows at 128 < S <= 512, on the GPU (csrc/kernels/attention_packed.hip, the long entry
points: the forward over ceil(S/128) query blocks, the dKV + dQ backward pair): forward, backward and the bias gradient
bit for bit against the padded kernels fed the re-padded operands, inside NaN-filled, sentinel-fenced buffers; the
overrun guard; the refusals; and the model's switch (bert_fused._PACKED_ATTN) at S = 256: the same loss bits, the same
gradient up to the order of the atomic sums, and no re-padding launches around attention.

All kernel tests: nh = 2 (H = 128), B = 8, randn inputs in bf16 at unit scale (|score| < 100, so a masked key's
probability exp(x - 10000 - m) is exactly 0 in fp32).  Length sets (at S = 192: clipped to 192):
  M1  at S = 256: T = 1103, T_alloc = 1152: a tail exists
  M2  the 128-block, 32-query and 64-key edges from both sides
  M3  at S = 256: T = 1024 = T_alloc: no tail, the last record ends on the buffer's last row; two records are empty
  M4  S = 512 only: the 147 KB LDS configuration, an empty record, a record of one row
S = 192: the last 128-block of a record is half empty; S = 256: the first with two full blocks.
"""
import functools
import os
import sys

import pytest
import torch

import dtg  # noqa: F401
from dtg.models import bert, bert_fused
from dtg.ops import lib, seqpack
from dtg.ops.mlm import mlm_mask_ref
from dtg.ops.seqpack import SeqPack
from dtg.ops.transformer import mask_additive
from dtg.parallel import FlatParams

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bert_cases import IDS, make_rows  # noqa: E402

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
FENCE = 64  # sentinel rows on either side of an output
SENT = 0x4D4D  # the fence's bf16 bit pattern (a finite value no kernel writes)
NH, B = 2, 8
H = NH * 64
SEED = 77
SETS = {"M1": [256, 129, 8, 200, 77, 128, 255, 50], "M2": [1, 127, 128, 129, 159, 161, 193, 256],
        "M3": [256, 0, 130, 256, 64, 191, 0, 127], "M4": [512, 300, 0, 65, 511, 129, 384, 1]}
GRID = [(n, S, p) for n in ("M1", "M2", "M3") for S in (192, 256) for p in (0.0, 0.1)] + [("M4", 512, 0.1)]


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _fenced(rows, W):
    """-> (whole buffer, the [rows, W] view in its middle): fences of SENT, the view filled with NaN"""
    buf = torch.full(((rows + 2 * FENCE) * W,), SENT, dtype=torch.int16, device=dev).view(torch.bfloat16)
    out = buf[FENCE * W:(FENCE + rows) * W].view(rows, W)
    out.fill_(float("nan"))
    return buf, out


def _fences_intact(buf, rows, W):
    b = _bits(buf)
    return bool((b[:FENCE * W] == SENT).all()) and bool((b[(FENCE + rows) * W:] == SENT).all())


@functools.lru_cache(maxsize=None)
def _case(name, S):
    """-> (lens, pack, qkv [T_alloc, 3H] and dout [T_alloc, H]: random on every row, the tail rows included)"""
    lens = [min(n, S) for n in SETS[name]]
    pack = SeqPack.from_lengths(torch.tensor(lens, dtype=torch.int32, device=dev), lens, S)
    g = torch.Generator().manual_seed(S + len(name) + sum(lens))
    qkv = torch.randn(pack.T_alloc, 3 * H, generator=g).bfloat16().to(dev)
    dout = torch.randn(pack.T_alloc, H, generator=g).bfloat16().to(dev)
    return lens, pack, qkv, dout


@functools.lru_cache(maxsize=None)
def _padded(name, S, p):
    """the padded kernels on the re-padded operands, computed once per case and shared (read only):
    -> (ctx [T_alloc, H], lse [nh, T_alloc] (0 where no record has a row), dqkv [T_alloc, 3H])"""
    lens, pack, qkv, dout = _case(name, S)
    cu, Ta = pack.cu, pack.T_alloc
    am = (torch.arange(S).view(1, S) < torch.tensor(lens).view(B, 1)).float().to(dev)
    mask = mask_additive(am)
    qp = seqpack.seq_pad(qkv, cu, B, S)
    cp, lp = lib().attn_fused_fwd(qp, mask, B, S, NH, p, SEED)
    dq = lib().attn_fused_bwd(qp, cp, seqpack.seq_pad(dout, cu, B, S), lp, mask, B, S, NH, p, SEED)
    # padded lse entry [b * nh + h][q] -> packed [h][cu[b] + q]
    lse = seqpack.seq_unpad_ref(lp.view(B, NH, S).permute(0, 2, 1).reshape(B * S, NH), cu, B, S, Ta).t().contiguous()
    torch.cuda.synchronize()
    return seqpack.seq_unpad(cp, cu, B, S, Ta), lse, seqpack.seq_unpad(dq, cu, B, S, Ta)


def _geometry(name, S, pack):
    if (name, S) == ("M1", 256):
        assert (pack.T, pack.T_alloc) == (1103, 1152)
    if (name, S) == ("M3", 256):
        assert pack.T == pack.T_alloc == 1024


# ---- 1: forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,p", GRID)
def test_forward_equals_padded_kernel_bitwise(name, S, p):
    lens, pack, qkv, _ = _case(name, S)
    T, Ta = pack.T, pack.T_alloc
    _geometry(name, S, pack)
    want_ctx, want_lse, _ = _padded(name, S, p)
    ctx, lse = seqpack.attn_packed_long_fwd(qkv, pack.cu, B, S, NH, p, SEED)
    torch.cuda.synchronize()
    assert ctx.shape == (Ta, H) and lse.shape == (NH, Ta) and lse.dtype == torch.float32
    assert torch.equal(_bits(ctx), _bits(want_ctx))  # real rows: the padded kernel's bits; tail rows: zeros
    assert torch.equal(_bits(lse[:, :T]), _bits(want_lse[:, :T]))
    # the output buffer: a NaN-filled view between fences -- a wrong index shows in a fence and cannot fault
    buf, out = _fenced(Ta, H)
    res, _ = seqpack.attn_packed_long_fwd(qkv, pack.cu, B, S, NH, p, SEED, out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr() and _fences_intact(buf, Ta, H)
    assert not _bits(out)[T:].any()  # tail rows: exactly zero
    assert torch.isfinite(out[:T].float()).all() and torch.equal(_bits(out), _bits(ctx))


# ---- 2: backward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,p", GRID)
def test_backward_equals_padded_kernel_bitwise(name, S, p):
    """dout is random on the tail rows too: it must not leak.  Twice on the same inputs: without dbias the kernels have
    no atomics, the bits repeat."""
    lens, pack, qkv, dout = _case(name, S)
    T, Ta = pack.T, pack.T_alloc
    _geometry(name, S, pack)
    _, _, want = _padded(name, S, p)
    ctx, lse = seqpack.attn_packed_long_fwd(qkv, pack.cu, B, S, NH, p, SEED)
    assert Ta == T or bool(dout[T:].float().abs().sum() > 0)
    buf, out = _fenced(Ta, 3 * H)
    res = seqpack.attn_packed_long_bwd(qkv, ctx, dout, lse, pack.cu, B, S, NH, p, SEED, out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr() and _fences_intact(buf, Ta, 3 * H)
    assert not _bits(out)[T:].any()  # tail rows: exactly zero
    assert torch.isfinite(out.float()).all()
    assert torch.equal(_bits(out), _bits(want))
    again = seqpack.attn_packed_long_bwd(qkv, ctx, dout, lse, pack.cu, B, S, NH, p, SEED)
    assert torch.equal(_bits(again), _bits(out))


# ---- 3: the bias gradient --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,p", GRID)
def test_dbias_adds_the_packed_column_sums(name, S, p):
    """dbias is pre-filled (an add, not a store) and compared with the fp64 column sums of the kernels' own dqkv over
    rows 0 .. T - 1.  Bound per column: 2^-8 sum|x| (the kernels sum the fp32 accumulators BEFORE their bf16 rounding)
    + (T - 1) 2^-24 sum|x| (fp32 sums in an order the atomics choose)."""
    lens, pack, qkv, dout = _case(name, S)
    T = pack.T
    ctx, lse = seqpack.attn_packed_long_fwd(qkv, pack.cu, B, S, NH, p, SEED)
    pre = torch.randn(3 * H, generator=torch.Generator().manual_seed(5)).to(dev)
    db = pre.clone()
    dq = seqpack.attn_packed_long_bwd(qkv, ctx, dout, lse, pack.cu, B, S, NH, p, SEED, dbias=db)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dq), _bits(_padded(name, S, p)[2]))  # the epilogues do not disturb dqkv
    x = dq[:T].double()
    exact, mag = x.sum(0), x.abs().sum(0)
    bound = 2.0 ** -8 * mag + (T - 1) * 2.0 ** -24 * mag
    err = ((db.double() - pre.double()) - exact).abs()
    print("[attn_packed_long dbias] %s S=%d p=%.1f: worst err / bound %.4f (min bound %.3e)" % (
        name, S, p, (err / bound.clamp(min=1e-300)).max().item(), bound.min().item()))
    assert bool((mag > 0).all()) and bool((err <= bound).all())


# ---- 4: the overrun guard --------------------------------------------------------------------------------------------
def test_cu_beyond_the_buffer_is_clamped():
    """S = 256: the last record's end lies 15 rows beyond T_alloc: its rows beyond the buffer are neither read nor
    written (qkv, ctx and dqkv each end in a fence of their own), the other records' rows are those of the full run,
    and everything written is finite."""
    S, p = 256, 0.0
    lens, pack, qkv, dout = _case("M1", S)
    small = pack.T_alloc - 64
    cu = pack.cu
    assert int(cu[B - 1]) < small < int(cu[B])
    full_ctx, _, full_dq = _padded("M1", S, p)
    sbuf, src = _fenced(small, 3 * H)
    src.copy_(qkv[:small])
    buf, out = _fenced(small, H)
    ctx, lse = seqpack.attn_packed_long_fwd(src, cu, B, S, NH, p, SEED, out=out)
    torch.cuda.synchronize()
    assert _fences_intact(buf, small, H) and _fences_intact(sbuf, small, 3 * H)
    keep = int(cu[B - 1])  # rows of the records that fit
    assert torch.equal(_bits(out[:keep]), _bits(full_ctx[:keep])) and torch.isfinite(out.float()).all()
    assert torch.isfinite(lse[:, :small]).all()
    dbuf, dq = _fenced(small, 3 * H)
    seqpack.attn_packed_long_bwd(src, ctx, dout[:small].contiguous(), lse, cu, B, S, NH, p, SEED, out=dq)
    torch.cuda.synchronize()
    assert _fences_intact(dbuf, small, 3 * H) and _fences_intact(sbuf, small, 3 * H) and _fences_intact(buf, small, H)
    assert torch.equal(_bits(dq[:keep]), _bits(full_dq[:keep])) and torch.isfinite(dq.float()).all()
    # a cu that starts beyond the buffer, and a negative one: those records are empty
    bad = cu.clone()
    bad[B - 1:] += 4096
    bad[0] = -5
    a, b = int(cu[1]), int(cu[B - 2])
    buf, out = _fenced(small, H)
    _, lse2 = seqpack.attn_packed_long_fwd(src, bad, B, S, NH, p, SEED, out=out)
    torch.cuda.synchronize()
    assert _fences_intact(buf, small, H)
    assert torch.equal(_bits(out[a:b]), _bits(full_ctx[a:b]))
    assert bool(torch.isnan(out[:a].float()).all())  # record 0 (negative start): nothing written
    assert bool(torch.isnan(out[int(cu[B - 1]) + 1:].float()).all())  # record B - 1 (beyond the buffer): nothing
    dbuf, dq = _fenced(small, 3 * H)
    seqpack.attn_packed_long_bwd(src, out, dout[:small].contiguous(), lse2, bad, B, S, NH, p, SEED, out=dq)
    torch.cuda.synchronize()
    assert _fences_intact(dbuf, small, 3 * H) and _fences_intact(sbuf, small, 3 * H)
    assert torch.equal(_bits(dq[a:b]), _bits(full_dq[a:b]))
    assert bool(torch.isnan(dq[:a].float()).all()) and bool(torch.isnan(dq[int(cu[B - 1]) + 1:].float()).all())


# ---- 5: refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_the_operand():
    S = 256
    lens, pack, qkv, dout = _case("M1", S)
    Ta, cu = pack.T_alloc, pack.cu
    wide = torch.zeros(Ta, 6 * H, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="qkv must be contiguous"):
        seqpack.attn_packed_long_fwd(wide[:, :3 * H], cu, B, S, NH, 0.0, 0)
    with pytest.raises(RuntimeError, match="qkv: the row width must be 3 \\* nh \\* 64"):
        seqpack.attn_packed_long_fwd(torch.zeros(Ta, 3 * NH * 32, dtype=torch.bfloat16, device=dev), cu, B, S, NH, 0.0,
                                     0)
    for bad_s in (128, 576, 200):
        with pytest.raises(RuntimeError, match="S: long packed attention takes a multiple of 64 with 128 < S <= 512, "
                                               "got %d" % bad_s):
            seqpack.attn_packed_long_fwd(qkv, cu, B, bad_s, NH, 0.0, 0)
    with pytest.raises(RuntimeError, match="S: long packed attention takes"):
        lib().attn_packed_long_bwd(qkv, dout, dout, torch.zeros(NH, Ta, device=dev), cu, B, 128, NH, 0.0, 0)
    with pytest.raises(RuntimeError, match="cu must be a contiguous int32"):
        seqpack.attn_packed_long_fwd(qkv, cu.long(), B, S, NH, 0.0, 0)
    with pytest.raises(RuntimeError, match="cu must be a contiguous int32"):
        seqpack.attn_packed_long_fwd(qkv, cu[:B], B, S, NH, 0.0, 0)
    with pytest.raises(RuntimeError, match="qkv must be a 2-D bf16"):
        lib().attn_packed_long_bwd(qkv.float(), dout, dout, torch.zeros(NH, Ta, device=dev), cu, B, S, NH, 0.0, 0)
    with pytest.raises(RuntimeError, match="T_alloc"):
        seqpack.attn_packed_long_fwd(qkv[:Ta - 4], cu, B, S, NH, 0.0, 0)
    with pytest.raises(RuntimeError, match="dout must be"):
        lib().attn_packed_long_bwd(qkv, dout, dout[:Ta - 8], torch.zeros(NH, Ta, device=dev), cu, B, S, NH, 0.0, 0)
    with pytest.raises(RuntimeError, match="lse must be"):
        lib().attn_packed_long_bwd(qkv, dout, dout, torch.zeros(NH, Ta - 1, device=dev), cu, B, S, NH, 0.0, 0)
    for ok in (192, 256, 512):
        assert seqpack.attn_packed_long_supported(ok, 64)
    for no in (128, 576, 200):
        assert not seqpack.attn_packed_long_supported(no, 64)
    assert not seqpack.attn_packed_long_supported(256, 32)
    torch.cuda.synchronize()


# ---- 6: the model ----------------------------------------------------------------------------------------------------
PRED = 10
CFG = dict(vocab_size=1024, hidden=128, layers=2, heads=2, intermediate=512, max_position=256)
_rel = lambda a, b: ((a - b).norm() / (b.norm() + 1e-12)).item()  # noqa: E731


def _model(seed=0, **over):
    torch.manual_seed(seed)
    model = bert.BertForPreTraining(bert.BertConfig(**dict(CFG, **over))).to(dev)
    with torch.no_grad():  # biases and LayerNorm parameters away from (0, 1): an omitted one would show
        for n, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    return model, FlatParams(model)


def _batch(Bn, S, lens, seed):
    rows = make_rows(Bn, S, seed=seed, lengths=lens)
    ids, tt, am, pos, lab = mlm_mask_ref(*rows, seed=1, epoch=0, P=PRED, **IDS)
    nsp = torch.tensor([(b * 7 + seed) % 2 for b in range(Bn)])
    return (ids, tt, am, pos, lab, nsp), max(1, int((lab >= 0).sum())), rows[2]


def _step(model, flat, batch, nv, pack, step=5):
    """forward + backward -> (loss fp32, flat gradient fp32 in named_parameters order)"""
    model._step = step
    flat.zero_grad()
    loss = model(*batch, num_valid=nv, pack=pack)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().float().cpu().clone(), torch.cat([p.grad.detach().float().reshape(-1).cpu()
                                                           for _, p in model.named_parameters()])


@pytest.fixture(scope="module")
def small_model():
    """the 2-layer model, dropout on, with an M1 batch at S = 256 and its pack on the device"""
    model, flat = _model(seed=2)
    model.train()
    batch, nv, lengths = _batch(B, 256, SETS["M1"], seed=3)
    d = tuple(t.to(dev) for t in batch)
    pack = SeqPack.from_lengths(lengths.to(dev), lengths.tolist(), 256)
    assert model.fused_ok(d[0]) and model.cfg.dropout > 0 and model.cfg.attn_dropout > 0
    assert (pack.T, pack.T_alloc) == (1103, 1152)
    return model, flat, d, nv, pack


def test_model_switch_same_loss_bits_same_gradient(small_model, monkeypatch):
    """_PACKED_ATTN on against off at S = 256, p = 0.1, fixed ``_step``: the forward has no atomics, so the loss is the
    same bits; the gradients agree up to the order of the atomic sums (2^-8: the bound of
    test_attn_packed_gpu.py::test_model_switch_same_loss_bits_same_gradient), flat and per parameter"""
    model, flat, d, nv, pack = small_model
    assert bert_fused._PACKED_ATTN is True and bert_fused._ATTN == "fused"
    l1, g1 = _step(model, flat, d, nv, pack)
    monkeypatch.setattr(bert_fused, "_PACKED_ATTN", False)
    l0, g0 = _step(model, flat, d, nv, pack)
    e = _rel(g1, g0)
    print("[attn_packed_long model] loss %.6f / %.6f, grad rel diff %.3e, |grad| %.4f" % (l0, l1, e, g0.norm()))
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all() and g0.norm() > 0
    assert torch.equal(l0, l1)
    assert e <= 2.0 ** -8
    o = 0
    for name, prm in model.named_parameters():
        n = prm.numel()
        a, r = g1[o:o + n], g0[o:o + n]
        o += n
        if r.norm() > 0:
            assert _rel(a, r) <= 2.0 ** -8, (name, _rel(a, r))
        else:
            assert not a.any(), name


def test_no_repadding_launches_around_attention(small_model, monkeypatch):
    """one training step of the 2-layer model at S = 256: with the switch on, seq_pad and seq_unpad run once each (the
    heads' pad_rows and its backward); off, 5 times each (+ 2 per layer and pass)"""
    model, flat, d, nv, pack = small_model
    calls = {"pad": 0, "unpad": 0}
    pad, unpad = seqpack.seq_pad, seqpack.seq_unpad

    def count_pad(*a, **k):
        calls["pad"] += 1
        return pad(*a, **k)

    def count_unpad(*a, **k):
        calls["unpad"] += 1
        return unpad(*a, **k)

    monkeypatch.setattr(seqpack, "seq_pad", count_pad)
    monkeypatch.setattr(seqpack, "seq_unpad", count_unpad)
    for switch, want in ((True, 1), (False, 5)):
        monkeypatch.setattr(bert_fused, "_PACKED_ATTN", switch)
        calls["pad"] = calls["unpad"] = 0
        loss, _ = _step(model, flat, d, nv, pack)
        assert torch.isfinite(loss).all()
        assert (calls["pad"], calls["unpad"]) == (want, want), (switch, calls)


def test_pretraining_logits_same_bits(small_model, monkeypatch):
    model, flat, d, nv, pack = small_model
    ids, tt, am, pos = d[:4]
    with torch.no_grad():
        on = model.pretraining_logits(ids, tt, am, pos, pack=pack)
        monkeypatch.setattr(bert_fused, "_PACKED_ATTN", False)
        off = model.pretraining_logits(ids, tt, am, pos, pack=pack)
    torch.cuda.synchronize()
    assert on[0].shape == (B * PRED, 1024) and on[1].shape == (B, 2)
    for a, b in zip(on, off):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
