"""The causal packed attention mirror and entry points of ops/seqpack.py on CPU tensors (set A of the GPU test, nh = 1),
and the model's choice of kernel pair (bert_fused._packed_attn) with the extension stubbed."""
import math

import pytest
import torch

import dtg  # noqa: F401
from dtg.models import bert_fused
from dtg.ops import seqpack

S, NH, LENS = 192, 1, [192, 1, 129, 65, 0, 17, 127, 180]
B, H = len(LENS), NH * 64


def _case(dtype):
    cu = seqpack.seq_offsets(torch.tensor(LENS, dtype=torch.int32), S)
    T = int(cu[B])
    Ta = -(-T // 64) * 64
    assert (T, Ta) == (711, 768)
    g = torch.Generator().manual_seed(3)
    return cu, T, Ta, torch.randn(Ta, 3 * H, generator=g, dtype=dtype), torch.randn(Ta, H, generator=g, dtype=dtype)


def test_causal_mirror_is_a_softmax_over_the_records_earlier_keys():
    cu, T, Ta, qkv, _ = _case(torch.float64)
    got = seqpack.attn_packed_ref(qkv, cu, B, S, NH, causal=True)
    assert got.shape == (Ta, H) and not got[T:].any()
    for b, n in enumerate(LENS):
        base = int(cu[b])
        for q in range(n):
            w = [math.exp(float(qkv[base + q, :64] @ qkv[base + k, 64:128]) / 8.0) for k in range(q + 1)]
            want = sum(wk * qkv[base + k, 128:] for k, wk in enumerate(w)) / sum(w)
            assert torch.allclose(got[base + q], want, rtol=1e-9, atol=1e-12), (b, q)


def test_default_is_unchanged():
    cu, T, Ta, qkv, _ = _case(torch.float32)
    valid = seqpack._coords(cu, B, S, Ta)[1]
    for p in (0.0, 0.1):
        want = seqpack.seq_unpad_ref(seqpack.attention_ref(seqpack.seq_pad_ref(qkv, cu, B, S),
                                                           (1.0 - valid.float()) * -10000.0, B, S, NH, p, 9),
                                     cu, B, S, Ta)
        assert torch.equal(seqpack.attn_packed_ref(qkv, cu, B, S, NH, p, 9), want)
        assert torch.equal(seqpack.attn_packed_ref(qkv, cu, B, S, NH, p, 9, causal=False), want)
        assert not torch.equal(seqpack.attn_packed_ref(qkv, cu, B, S, NH, p, 9, causal=True), want)


def test_cpu_tensors_reach_the_mirror():
    cu, T, Ta, qkv, dout = _case(torch.float32)
    for p in (0.0, 0.1):
        ctx, lse = seqpack.attn_packed_causal_fwd(qkv, cu, B, S, NH, p, 9)
        x = qkv.clone().requires_grad_()
        want = seqpack.attn_packed_ref(x, cu, B, S, NH, p, 9, causal=True)
        assert lse is None and torch.equal(ctx, want.detach()) and not ctx[T:].any()
        (gx,) = torch.autograd.grad(want, x, dout)
        db = torch.full((3 * H,), 0.5)
        dqkv = seqpack.attn_packed_causal_bwd(qkv, ctx, dout, None, cu, B, S, NH, p, 9, dbias=db)
        assert torch.equal(dqkv, gx) and not dqkv[T:].any() and gx.abs().sum() > 0
        assert torch.allclose(db, gx.sum(0) + 0.5, rtol=0, atol=1e-5 * gx.abs().sum(0).max().item())


class _Lib:
    """the extension's shape predicates (lo < S <= hi) and, as entry points, their own names"""
    RANGE = {"attn_packed_causal_supported": (63, 8192), "attn_packed_supported": (63, 128),
             "attn_packed_long_supported": (128, 512), "attn_packed_stream_supported": (512, 8192)}

    def __getattr__(self, name):
        if name in self.RANGE:
            lo, hi = self.RANGE[name]
            return lambda S, dh: dh == 64 and S % 64 == 0 and lo < S <= hi
        return name


@pytest.mark.parametrize("S_,causal,on,want", [
    (192, True, True, ("attn_packed_causal_fwd", "attn_packed_causal_bwd")), (192, True, False, False),
    (64, True, True, ("attn_packed_causal_fwd", "attn_packed_causal_bwd")), (600, True, True, False),
    (192, False, True, ("attn_packed_long_fwd", "attn_packed_long_bwd")), (192, False, False, False),
    (128, False, True, ("attn_packed_fwd", "attn_packed_bwd")),
    (1024, False, True, ("attn_packed_stream_fwd", "attn_packed_stream_bwd"))])
def test_the_layer_picks_the_pair(monkeypatch, S_, causal, on, want):
    monkeypatch.setattr(bert_fused, "lib", _Lib)
    monkeypatch.setattr(bert_fused, "_PACKED_ATTN", on)
    assert bert_fused._packed_attn(object(), S_, 3 * 2 * 64, 2, causal) == want
    assert bert_fused._packed_attn(None, S_, 3 * 2 * 64, 2, causal) is False
    assert bert_fused._packed_attn(object(), S_, 3 * 2 * 32, 2, causal) is False
