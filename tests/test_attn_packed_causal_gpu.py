"""Causal fused attention on packed rows, on the GPU (csrc/kernels/attention_causal_packed.hip): against the plain fp64
causal attention (bounds: those test_attn_causal_gpu.py holds the padded causal kernels to) and, bit for bit, against
the padded causal kernels fed the re-padded operands and the length mask; isolation; the overrun guard; the refusals;
the model's switch (bert_fused._PACKED_ATTN) on a CausalLM.  nh = 2; randn inputs in bf16, qkv scaled by 1.5.  Sets:
  A  S = 192: a tail of 57 rows; ends one row into a 128-block, a 64-chunk, a 16-row fragment; a one-row, an empty record
  B  S = 640: crosses 512; 9 and 10 chunks          C  S = 64: the smallest S, no tail, the last record is empty
"""
import functools
import os
import sys

import pytest
import torch

import dtg  # noqa: F401
from dtg.models import CausalLM, bert, bert_fused
from dtg.ops import lib, seqpack
from dtg.ops.seqpack import SeqPack
from dtg.ops.transformer import mask_additive

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_attn_packed_long_gpu import _batch, _model, _rel, _step  # noqa: E402  (the tiny 2-layer model)

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
NH = 2
H = NH * 64
SEED = 1234
SETS = {"A": (192, [192, 1, 129, 65, 0, 17, 127, 180], (711, 768)),  # name: (S, lengths, (T, T_alloc))
        "B": (640, [640, 513, 0, 577, 65], (1795, 1856)), "C": (64, [64, 1, 33, 64, 30, 0], (192, 192))}


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (S, B, lens, pack, qkv [T_alloc, 3H], dout [T_alloc, H]: random on every row, the tail rows included)"""
    S, lens, geom = SETS[name]
    pack = SeqPack.from_lengths(torch.tensor(lens, dtype=torch.int32, device=dev), lens, S)
    assert (pack.T, pack.T_alloc) == geom
    g = torch.Generator().manual_seed(6 + S)
    qkv = (torch.randn(pack.T_alloc, 3 * H, generator=g) * 1.5).bfloat16().to(dev)
    dout = torch.randn(pack.T_alloc, H, generator=g).bfloat16().to(dev)
    return S, len(lens), lens, pack, qkv, dout


@functools.lru_cache(maxsize=None)
def _packed(name, p):
    """the packed causal kernels, computed once per case and shared (read only): -> (ctx, lse, dqkv)"""
    S, B, lens, pack, qkv, dout = _case(name)
    ctx, lse = seqpack.attn_packed_causal_fwd(qkv, pack.cu, B, S, NH, p, SEED)
    return ctx, lse, seqpack.attn_packed_causal_bwd(qkv, ctx, dout, lse, pack.cu, B, S, NH, p, SEED)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_against_fp64_reference(name, p):
    S, B, lens, pack, qkv, dout = _case(name)
    cu, T, Ta = pack.cu, pack.T, pack.T_alloc
    ctx, lse, dqkv = _packed(name, p)
    db = torch.full((3 * H,), 0.5, device=dev)
    dqkv2 = seqpack.attn_packed_causal_bwd(qkv, ctx, dout, lse, cu, B, S, NH, p, SEED, dbias=db)
    assert ctx.shape == (Ta, H) and lse.shape == (NH, Ta) and lse.dtype == torch.float32 and dqkv.shape == (Ta, 3 * H)
    qr = qkv.double().requires_grad_()
    ref = seqpack.attn_packed_ref(qr, cu, B, S, NH, p, SEED, causal=True)
    ref.backward(dout.double())
    q, k, _ = seqpack.seq_pad_ref(qkv.double(), cu, B, S).view(B, S, 3, NH, 64).permute(2, 0, 3, 1, 4)
    pos = torch.arange(S, device=dev)
    seen = (pos.view(1, S) <= pos.view(S, 1)) & (pos.view(1, 1, 1, S) < torch.tensor(lens, device=dev).view(B, 1, 1, 1))
    ref_lse = torch.logsumexp(((q @ k.transpose(-1, -2)) / 8.0).masked_fill(~seen, -1e300), -1)  # [B, nh, S]
    ref_lse = seqpack.seq_unpad_ref(ref_lse.permute(0, 2, 1).reshape(B * S, NH), cu, B, S, Ta).t()
    e_out, e_lse = rel(ctx, ref), (lse[:, :T].double() - ref_lse[:, :T]).abs().max().item()
    e_g = [rel(dqkv[:, i * H:(i + 1) * H], qr.grad[:, i * H:(i + 1) * H]) for i in range(3)]
    e_db = rel(db, qr.grad.sum(0) + 0.5)
    print("[attn packed causal] %s S=%d p=%.1f rel out %.4f, max |dLSE| %.4f, rel dQ %.4f dK %.4f dV %.4f dbias %.4f"
          % (name, S, p, e_out, e_lse, *e_g, e_db))
    for t in (ctx, lse[:, :T], dqkv, db):
        assert torch.isfinite(t).all()
    assert e_out < 1.5e-2
    assert e_lse <= 2e-2
    assert max(e_g) < 3e-2, e_g
    assert e_db < 2e-2
    assert torch.equal(_bits(dqkv2), _bits(dqkv))  # the bias gradient is added on the side: the same dQKV bits
    assert not _bits(ctx)[T:].any() and not _bits(dqkv)[T:].any()  # tail rows: exactly zero
    # rows < T: the padded causal kernels on the re-padded operands with the length mask, bit for bit
    mask = mask_additive((torch.arange(S).view(1, S) < torch.tensor(lens).view(B, 1)).float().to(dev))
    qp = seqpack.seq_pad(qkv, cu, B, S)
    cp, lp = lib().attn_causal_fwd(qp, mask, B, S, NH, p, SEED)
    dq = lib().attn_causal_bwd(qp, cp, seqpack.seq_pad(dout, cu, B, S), lp, mask, B, S, NH, p, SEED)
    want_lse = seqpack.seq_unpad_ref(lp.view(B, NH, S).permute(0, 2, 1).reshape(B * S, NH), cu, B, S, Ta).t()
    assert torch.equal(_bits(ctx[:T]), _bits(seqpack.seq_unpad(cp, cu, B, S, Ta)[:T]))
    assert torch.equal(_bits(lse[:, :T]), _bits(want_lse[:, :T].contiguous()))
    assert torch.equal(_bits(dqkv[:T]), _bits(seqpack.seq_unpad(dq, cu, B, S, Ta)[:T]))


def test_no_row_outside_the_record_and_no_later_key_is_seen():
    """Set A, p = 0: NaN on every qkv row outside record 2 (129 rows), the tail included, except record 0's rows
    < 70.  Record 2 and record 0's rows < 70 keep their out and LSE bits; record 2 keeps its dQKV bits."""
    S, B, lens, pack, qkv, dout = _case("A")
    cu = pack.cu
    ctx, lse, dqkv = _packed("A", 0.0)
    a, b = int(cu[2]), int(cu[3])
    bad = torch.full_like(qkv, float("nan"))
    bad[a:b], bad[:70] = qkv[a:b], qkv[:70]
    ctx2, lse2 = seqpack.attn_packed_causal_fwd(bad, cu, B, S, NH, 0.0, SEED)
    dqkv2 = seqpack.attn_packed_causal_bwd(bad, ctx2, dout, lse2, cu, B, S, NH, 0.0, SEED)
    for lo, hi in ((a, b), (0, 70)):
        assert torch.isfinite(ctx2[lo:hi].float()).all() and torch.isfinite(lse2[:, lo:hi]).all()
        assert torch.equal(_bits(ctx2[lo:hi]), _bits(ctx[lo:hi]))
        assert torch.equal(_bits(lse2[:, lo:hi].contiguous()), _bits(lse[:, lo:hi].contiguous()))
    assert torch.equal(_bits(dqkv2[a:b]), _bits(dqkv[a:b]))


def test_cu_beyond_the_buffer_is_clamped():
    """Set A in a buffer 64 rows short, every operand and output a row view framed by NaN: the records that fit keep
    the full run's bits, nothing around the views is written, everything written is finite."""
    S, B, lens, pack, qkv, dout = _case("A")
    p, cu, small, F = 0.0, pack.cu, pack.T_alloc - 64, 64
    keep = int(cu[B - 1])  # rows of the records that fit
    assert keep < small < int(cu[B])
    full_ctx, _, full_dq = _packed("A", p)

    def framed(W, fill=None):
        whole = torch.full((small + 2 * F, W), float("nan"), dtype=torch.bfloat16, device=dev)
        view = whole[F:F + small]
        if fill is not None:
            view.copy_(fill[:small])
        return whole, view

    def frame_untouched(whole):
        return bool(torch.isnan(whole[:F].float()).all()) and bool(torch.isnan(whole[F + small:].float()).all())

    (_, src), (_, dsrc) = framed(3 * H, qkv), framed(H, dout)
    wc, out = framed(H)
    _, lse = seqpack.attn_packed_causal_fwd(src, cu, B, S, NH, p, SEED, out=out)
    wd, dq = framed(3 * H)
    seqpack.attn_packed_causal_bwd(src, out, dsrc, lse, cu, B, S, NH, p, SEED, out=dq)
    torch.cuda.synchronize()
    assert frame_untouched(wc) and frame_untouched(wd)
    assert torch.equal(_bits(out[:keep]), _bits(full_ctx[:keep]))
    assert torch.equal(_bits(dq[:keep]), _bits(full_dq[:keep]))
    assert torch.isfinite(out.float()).all() and torch.isfinite(dq.float()).all()
    assert torch.isfinite(lse[:, :small]).all()


def test_refusals_name_the_operand():
    S, B, lens, pack, qkv, dout = _case("A")
    Ta, cu, cap = pack.T_alloc, pack.cu, lib().attn_stream_max_s()
    wide = torch.zeros(Ta, 6 * H, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="qkv must be contiguous"):
        seqpack.attn_packed_causal_fwd(wide[:, :3 * H], cu, B, S, NH, 0.0, 0)
    with pytest.raises(RuntimeError, match="qkv: the row width must be 3 \\* nh \\* 64"):
        seqpack.attn_packed_causal_fwd(torch.zeros(Ta, 3 * NH * 32, dtype=torch.bfloat16, device=dev), cu, B, S, NH,
                                       0.0, 0)
    for bad_s in (600, cap + 64):
        with pytest.raises(RuntimeError, match="S: causal packed attention takes a multiple of 64 with 64 <= S <= "
                                               "%d, got %d" % (cap, bad_s)):
            seqpack.attn_packed_causal_fwd(qkv, cu, B, bad_s, NH, 0.0, 0)
        with pytest.raises(RuntimeError, match="S: causal packed attention takes"):
            lib().attn_packed_causal_bwd(qkv, dout, dout, torch.zeros(NH, Ta, device=dev), cu, B, bad_s, NH, 0.0, 0)
    with pytest.raises(RuntimeError, match="cu must be a contiguous int32"):
        seqpack.attn_packed_causal_fwd(qkv, cu.long(), B, S, NH, 0.0, 0)
    for ok in (64, 192, cap):
        assert seqpack.attn_packed_causal_supported(ok, 64)
    for no in (600, cap + 64):
        assert not seqpack.attn_packed_causal_supported(no, 64)
    assert not seqpack.attn_packed_causal_supported(192, 32)
    torch.cuda.synchronize()


def test_model_switch_at_192(monkeypatch):
    """A 2-layer CausalLM (hidden 128), dropout on, mixed lengths, fixed ``_step``: _PACKED_ATTN on against off.  The
    same loss bits (no atomics in the forward); gradients within 2^-8 (the order of the atomic sums), flat and per
    parameter; seq_pad / seq_unpad once each on (the head's pad_rows and its backward), 5 times each off."""
    S, lens = 192, [192, 65, 1, 129, 100, 17]
    monkeypatch.setattr(bert, "BertForPreTraining", CausalLM)  # what _model builds
    model, flat = _model(seed=2, max_position=S)
    model.train()
    batch, _, lengths = _batch(len(lens), S, lens, seed=3)
    d = (batch[0].to(dev), batch[2].to(dev))  # ids, attention mask
    nv = int((CausalLM.next_token_labels(*d) >= 0).sum())
    pack = SeqPack.from_lengths(lengths.to(dev), lengths.tolist(), S)
    assert isinstance(model, CausalLM) and model.cfg.causal and model.fused_ok(d[0]) and model.cfg.attn_dropout > 0
    calls = {"pad": 0, "unpad": 0}

    def counted(key, fn):
        def call(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return call

    monkeypatch.setattr(seqpack, "seq_pad", counted("pad", seqpack.seq_pad))
    monkeypatch.setattr(seqpack, "seq_unpad", counted("unpad", seqpack.seq_unpad))
    l1, g1 = _step(model, flat, d, nv, pack)
    assert (calls["pad"], calls["unpad"]) == (1, 1), calls
    monkeypatch.setattr(bert_fused, "_PACKED_ATTN", False)
    calls["pad"] = calls["unpad"] = 0
    l0, g0 = _step(model, flat, d, nv, pack)
    assert (calls["pad"], calls["unpad"]) == (5, 5), calls
    e = _rel(g1, g0)
    print("[attn packed causal model] loss %.6f / %.6f, grad rel diff %.3e, |grad| %.4f" % (l0, l1, e, g0.norm()))
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
