"""Attention on packed rows, the mirror (ops/seqpack.py ``attn_packed_ref``): against a per-record loop in fp64 in
which each record attends alone over its own keys with no mask at all -- values and autograd gradients --, zeros on the
tail rows, nothing from an empty record, and the dropout keep-mask at the PADDED index."""
import math

import pytest
import torch

import dtg  # noqa: F401
from dtg.ops import seqpack
from dtg.ops.transformer import attn_dropout_keep

NH, B = 2, 8
H = NH * 64
L1 = [8, 128, 77, 128, 9, 50, 101, 33]
L2 = [1, 16, 17, 31, 32, 33, 63, 64]
L3 = [65, 127, 128, 0, 15, 128, 64, 49]
SETS = {"L1": L1, "L2": L2, "L3": L3}


def _case(name, S, seed=0):
    lens = [min(n, S) for n in SETS[name]]
    T = sum(lens)
    Ta = max(64, -(-T // 64) * 64)
    cu = seqpack.seq_offsets_ref(torch.tensor(lens, dtype=torch.int32), S)
    g = torch.Generator().manual_seed(seed + S + len(name))
    qkv = torch.randn(Ta, 3 * H, generator=g, dtype=torch.float64)
    return lens, T, Ta, cu, qkv


def _per_record(qkv, lens, keep=None):
    """each record alone: softmax(Q K^T / 8) V over its own n keys, no mask; keep [B, nh, S, S] bool or None (p = 0.1)"""
    out = qkv.new_zeros(qkv.shape[0], H)
    t = 0
    for b, n in enumerate(lens):
        for h in range(NH):
            q, k, v = (qkv[t:t + n, i * H + h * 64:i * H + (h + 1) * 64] for i in range(3))
            pr = torch.softmax(q @ k.T / math.sqrt(64), -1)
            if keep is not None:
                pr = torch.where(keep[b, h, :n, :n], pr / 0.9, torch.zeros((), dtype=pr.dtype))
            out[t:t + n, h * 64:(h + 1) * 64] = pr @ v
        t += n
    return out


@pytest.mark.parametrize("S", [128, 64])
@pytest.mark.parametrize("name", list(SETS))
def test_mirror_equals_per_record_loop(name, S):
    lens, T, Ta, cu, qkv = _case(name, S)
    if name == "L1" and S == 128:
        assert (T, Ta) == (534, 576)
    if name == "L3" and S == 128:
        assert T == Ta == 576 and 0 in lens
    x = qkv.clone().requires_grad_(True)
    got = seqpack.attn_packed_ref(x, cu, B, S, NH)
    y = qkv.clone().requires_grad_(True)
    want = _per_record(y, lens)
    assert got.shape == (Ta, H) and (got - want).abs().max().item() <= 1e-9
    assert not got[T:].any()  # the tail rows: exactly zero
    w = torch.randn(Ta, H, generator=torch.Generator().manual_seed(1), dtype=torch.float64)  # random on the tail too
    (gx,) = torch.autograd.grad(got, x, w)
    (gy,) = torch.autograd.grad(want, y, w)
    assert (gx - gy).abs().max().item() <= 1e-9
    assert not gx[T:].any()  # nothing flows into (or out of) the tail rows
    # the op's CPU path is the mirror, its backward autograd through it
    ctx, lse = seqpack.attn_packed_fwd(qkv, cu, B, S, NH, 0.0, 0)
    assert lse is None and torch.equal(ctx, got.detach())
    db = torch.ones(3 * H, dtype=torch.float64)
    dq = seqpack.attn_packed_bwd(qkv, ctx, w, None, cu, B, S, NH, 0.0, 0, dbias=db)
    assert torch.equal(dq, gx) and (db - 1 - gx.sum(0)).abs().max().item() <= 1e-9


def test_empty_record_contributes_nothing():
    """L3 has a record of length 0: dropping it from the batch leaves the output and the gradient where they were"""
    S = 128
    lens, T, Ta, cu, qkv = _case("L3", S)
    e = lens.index(0)
    rest = lens[:e] + lens[e + 1:]
    cu2 = seqpack.seq_offsets_ref(torch.tensor(rest, dtype=torch.int32), S)
    x = qkv.clone().requires_grad_(True)
    y = qkv.clone().requires_grad_(True)
    a = seqpack.attn_packed_ref(x, cu, B, S, NH)
    b = seqpack.attn_packed_ref(y, cu2, B - 1, S, NH)
    assert torch.equal(a, b)
    w = torch.randn(Ta, H, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    assert torch.equal(torch.autograd.grad(a, x, w)[0], torch.autograd.grad(b, y, w)[0])


@pytest.mark.parametrize("S", [128, 64])
def test_dropout_mask_is_at_the_padded_index(S):
    """p = 0.1: row (b, h, q) keeps the keys that attn_dropout_keep keeps at ((b * nh + h) * S + q) * S + key"""
    lens, T, Ta, cu, qkv = _case("L1", S, seed=3)
    seed = 1234
    keep = attn_dropout_keep(seed, B * NH * S * S, 0.1).view(B, NH, S, S)
    assert 0.85 < keep.float().mean().item() < 0.95
    got = seqpack.attn_packed_ref(qkv, cu, B, S, NH, 0.1, seed)
    want = _per_record(qkv, lens, keep)
    assert (got - want).abs().max().item() <= 1e-9
    # and it matters: without the mask, or with the mask at packed coordinates, the result is another one
    assert (got - _per_record(qkv, lens)).abs().max().item() > 1e-3
