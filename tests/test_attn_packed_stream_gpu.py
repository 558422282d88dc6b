"""Streaming fused attention on packed rows at 512 < S <= 8192, on the GPU (csrc/kernels/attention_stream_packed.hip):
against the plain fp64 attention (bounds: those test_attn_stream_gpu.py holds the padded streaming kernels to) and, bit
for bit, against the padded streaming kernels fed the re-padded operands; the overrun guard; the refusals; and the
model's switch (bert_fused._PACKED_ATTN) at S = 576.

nh = 2; randn inputs in bf16, qkv scaled by 1.5.  Length sets:
  A  S = 640:  T = 2523, T_alloc = 2560: a tail of 37 rows; 9 and 10 chunks; records ending 1 row into a 128-block,
     a 64-chunk and a 16-row fragment; a one-row and an empty record; neighbours starting on the row after such an end
  B  S = 576:  T = 1536 = T_alloc: no tail, the last record is empty
  C  S = 1088: 17 chunks; T = 1788, T_alloc = 1792: a tail that an empty last record must zero
"""
import functools
import os
import sys

import pytest
import torch

import dtg  # noqa: F401
from dtg.models import bert_fused
from dtg.ops import lib, seqpack
from dtg.ops.seqpack import SeqPack
from dtg.ops.transformer import mask_additive

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_attn_packed_long_gpu import _batch, _model, _rel, _step  # noqa: E402  (the tiny 2-layer BERT)

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
NH = 2
H = NH * 64
SEED = 1234
SETS = {"A": (640, [640, 1, 513, 65, 0, 577, 127, 600], (2523, 2560)),  # name: (S, lengths, (T, T_alloc))
        "B": (576, [576, 64, 0, 576, 320, 0], (1536, 1536)), "C": (1088, [1088, 700, 0], (1788, 1792))}


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
def _padded(name, p):
    """the padded streaming kernels on the re-padded operands, computed once per case and shared (read only):
    -> (ctx [T_alloc, H], lse [nh, T_alloc] (0 where no record has a row), dqkv [T_alloc, 3H])"""
    S, B, lens, pack, qkv, dout = _case(name)
    cu, Ta = pack.cu, pack.T_alloc
    mask = mask_additive((torch.arange(S).view(1, S) < torch.tensor(lens).view(B, 1)).float().to(dev))
    qp = seqpack.seq_pad(qkv, cu, B, S)
    cp, lp = lib().attn_fused_fwd(qp, mask, B, S, NH, p, SEED)
    dq = lib().attn_fused_bwd(qp, cp, seqpack.seq_pad(dout, cu, B, S), lp, mask, B, S, NH, p, SEED)
    # padded lse entry [b * nh + h][q] -> packed [h][cu[b] + q]
    lse = seqpack.seq_unpad_ref(lp.view(B, NH, S).permute(0, 2, 1).reshape(B * S, NH), cu, B, S, Ta).t().contiguous()
    return seqpack.seq_unpad(cp, cu, B, S, Ta), lse, seqpack.seq_unpad(dq, cu, B, S, Ta)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_packed_stream_fwd_bwd(name, p):
    S, B, lens, pack, qkv, dout = _case(name)
    cu, T, Ta = pack.cu, pack.T, pack.T_alloc
    assert Ta == T or bool(dout[T:].float().abs().sum() > 0)
    ctx, lse = seqpack.attn_packed_stream_fwd(qkv, cu, B, S, NH, p, SEED)
    dqkv = seqpack.attn_packed_stream_bwd(qkv, ctx, dout, lse, cu, B, S, NH, p, SEED)
    db = torch.full((3 * H,), 0.5, device=dev)
    dqkv2 = seqpack.attn_packed_stream_bwd(qkv, ctx, dout, lse, cu, B, S, NH, p, SEED, dbias=db)
    assert ctx.shape == (Ta, H) and lse.shape == (NH, Ta) and lse.dtype == torch.float32 and dqkv.shape == (Ta, 3 * H)
    # the plain fp64 attention on the same rows, the same seed: a wrong dropout index is a gross error
    qr = qkv.double().requires_grad_()
    ref = seqpack.attn_packed_ref(qr, cu, B, S, NH, p, SEED)
    ref.backward(dout.double())
    q, k, _ = seqpack.seq_pad_ref(qkv.double(), cu, B, S).view(B, S, 3, NH, 64).permute(2, 0, 3, 1, 4)
    keys = torch.arange(S, device=dev).view(1, 1, 1, S) < torch.tensor(lens, device=dev).view(B, 1, 1, 1)
    ref_lse = torch.logsumexp(((q @ k.transpose(-1, -2)) / 8.0).masked_fill(~keys, -1e4), -1)  # [B, nh, S]
    ref_lse = seqpack.seq_unpad_ref(ref_lse.permute(0, 2, 1).reshape(B * S, NH), cu, B, S, Ta).t()
    e_out, e_lse = rel(ctx, ref), (lse[:, :T].double() - ref_lse[:, :T]).abs().max().item()
    e_g = [rel(dqkv[:, i * H:(i + 1) * H], qr.grad[:, i * H:(i + 1) * H]) for i in range(3)]
    e_db = rel(db, qr.grad.sum(0) + 0.5)
    print("[attn packed stream] %s S=%d p=%.1f rel out %.4f, max |dLSE| %.4f, rel dQ %.4f dK %.4f dV %.4f dbias %.4f"
          % (name, S, p, e_out, e_lse, *e_g, e_db))
    for t in (ctx, lse[:, :T], dqkv, db):
        assert torch.isfinite(t).all()
    assert e_out < 1.5e-2
    assert e_lse <= 2e-2
    assert max(e_g) < 3e-2, e_g
    assert e_db < 2e-2
    assert torch.equal(_bits(dqkv2), _bits(dqkv))  # the bias gradient is added on the side: the same dQKV bits
    assert not _bits(ctx)[T:].any() and not _bits(dqkv)[T:].any()  # tail rows: exactly zero
    # the padded streaming kernels on the re-padded operands: the same bits
    want_ctx, want_lse, want_dqkv = _padded(name, p)
    assert torch.equal(_bits(ctx), _bits(want_ctx))
    assert torch.equal(_bits(lse[:, :T]), _bits(want_lse[:, :T]))
    assert torch.equal(_bits(dqkv), _bits(want_dqkv))


def test_cu_beyond_the_buffer_is_clamped():
    """Set A in a buffer 64 rows short: the last record's end lies beyond it.  Every operand and output is a row view
    in the middle of a larger tensor, NaN outside the operands' rows and in the outputs: rows of the records that fit
    carry the full run's bits, nothing around the views is written, everything written is finite.  Then a cu with a
    negative first entry and a last record starting beyond the buffer: those two records are empty."""
    S, B, lens, pack, qkv, dout = _case("A")
    p, cu, small, F = 0.0, pack.cu, pack.T_alloc - 64, 64
    keep = int(cu[B - 1])  # rows of the records that fit
    assert keep < small < int(cu[B])
    full_ctx, _, full_dq = _padded("A", p)

    def framed(W, fill=None):
        whole = torch.full((small + 2 * F, W), float("nan"), dtype=torch.bfloat16, device=dev)
        view = whole[F:F + small]
        if fill is not None:
            view.copy_(fill[:small])
        return whole, view

    def frame_untouched(whole):
        return bool(torch.isnan(whole[:F].float()).all()) and bool(torch.isnan(whole[F + small:].float()).all())

    bad = cu.clone()
    bad[B - 1:] += 4096
    bad[0] = -5
    a, b = int(cu[1]), int(cu[B - 2])
    (_, src), (_, dsrc) = framed(3 * H, qkv), framed(H, dout)
    for c, lo, hi in ((cu, 0, keep), (bad, a, b)):
        wc, out = framed(H)
        _, lse = seqpack.attn_packed_stream_fwd(src, c, B, S, NH, p, SEED, out=out)
        wd, dq = framed(3 * H)
        seqpack.attn_packed_stream_bwd(src, out, dsrc, lse, c, B, S, NH, p, SEED, out=dq)
        torch.cuda.synchronize()
        assert frame_untouched(wc) and frame_untouched(wd)
        assert torch.equal(_bits(out[lo:hi]), _bits(full_ctx[lo:hi]))
        assert torch.equal(_bits(dq[lo:hi]), _bits(full_dq[lo:hi]))
        if c is cu:  # the clamped last record reaches the buffer's end: every row is written
            assert torch.isfinite(out.float()).all() and torch.isfinite(dq.float()).all()
            assert torch.isfinite(lse[:, :small]).all()
        else:        # record 0 (negative start) and record B - 1 (beyond the buffer): nothing written; record B - 2
            end = min(b + S, small)  # now ends at cu[B - 1] + 4096: S rows of it are taken
            for t in (out, dq):
                assert bool(torch.isnan(t[:a].float()).all()) and bool(torch.isnan(t[end:].float()).all())
                assert torch.isfinite(t[a:end].float()).all()


def test_refusals_name_the_operand():
    S, B, lens, pack, qkv, dout = _case("A")
    Ta, cu, cap = pack.T_alloc, pack.cu, lib().attn_stream_max_s()
    wide = torch.zeros(Ta, 6 * H, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="qkv must be contiguous"):
        seqpack.attn_packed_stream_fwd(wide[:, :3 * H], cu, B, S, NH, 0.0, 0)
    with pytest.raises(RuntimeError, match="qkv: the row width must be 3 \\* nh \\* 64"):
        seqpack.attn_packed_stream_fwd(torch.zeros(Ta, 3 * NH * 32, dtype=torch.bfloat16, device=dev), cu, B, S, NH,
                                       0.0, 0)
    for bad_s in (512, 600, cap + 64):
        with pytest.raises(RuntimeError, match="S: streaming packed attention takes a multiple of 64 with 512 < S <= "
                                               "%d, got %d" % (cap, bad_s)):
            seqpack.attn_packed_stream_fwd(qkv, cu, B, bad_s, NH, 0.0, 0)
        with pytest.raises(RuntimeError, match="S: streaming packed attention takes"):
            lib().attn_packed_stream_bwd(qkv, dout, dout, torch.zeros(NH, Ta, device=dev), cu, B, bad_s, NH, 0.0, 0)
    with pytest.raises(RuntimeError, match="cu must be a contiguous int32"):
        seqpack.attn_packed_stream_fwd(qkv, cu.long(), B, S, NH, 0.0, 0)
    with pytest.raises(RuntimeError, match="qkv must be a 2-D bf16"):
        lib().attn_packed_stream_bwd(qkv.float(), dout, dout, torch.zeros(NH, Ta, device=dev), cu, B, S, NH, 0.0, 0)
    for ok in (576, 1088, cap):
        assert seqpack.attn_packed_stream_supported(ok, 64)
    for no in (512, 600, cap + 64):
        assert not seqpack.attn_packed_stream_supported(no, 64)
    assert not seqpack.attn_packed_stream_supported(576, 32)
    assert not seqpack.attn_packed_long_supported(576, 64)
    torch.cuda.synchronize()


def test_model_switch_at_576(monkeypatch):
    """The 2-layer model, dropout on, a mixed-length batch at S = 576, fixed ``_step``: _PACKED_ATTN on against off.
    The forward has no atomics, so the loss is the same bits; the gradients agree up to the order of the atomic sums
    (2^-8, the bound of the two earlier packed model tests), flat and per parameter; seq_pad / seq_unpad run once each
    with the switch on (the heads' pad_rows and its backward) and 5 times each off (+ 2 per layer and pass)."""
    S, lens = 576, [576, 65, 1, 513, 320, 129]
    model, flat = _model(seed=2, max_position=S)
    model.train()
    batch, nv, lengths = _batch(len(lens), S, lens, seed=3)
    d = tuple(t.to(dev) for t in batch)
    pack = SeqPack.from_lengths(lengths.to(dev), lengths.tolist(), S)
    assert model.fused_ok(d[0]) and model.cfg.attn_dropout > 0 and bert_fused._PACKED_ATTN is True
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
    print("[attn packed stream model] loss %.6f / %.6f, grad rel diff %.3e, |grad| %.4f" % (l0, l1, e, g0.norm()))
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
