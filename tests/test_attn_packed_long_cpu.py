"""Attention on packed rows at 128 < S <= 512, the CPU path of the long wrappers (ops/seqpack.py
``attn_packed_long_fwd`` / ``attn_packed_long_bwd``): they take the mirror ``attn_packed_ref``, checked at S = 192 and
S = 256 against a per-record loop in fp64 in which each record attends alone over its own keys with no mask at all --
values and gradients --; zeros on the tail rows, the bias gradient added, nothing from an empty record."""
import math

import pytest
import torch

import dtg  # noqa: F401
from dtg.ops import seqpack

NH, B = 2, 8
H = NH * 64
SETS = {"M1": [256, 129, 8, 200, 77, 128, 255, 50], "M2": [1, 127, 128, 129, 159, 161, 193, 256],
        "M3": [256, 0, 130, 256, 64, 191, 0, 127]}


def _case(name, S, seed=0):
    lens = [min(n, S) for n in SETS[name]]
    T = sum(lens)
    Ta = max(64, -(-T // 64) * 64)
    cu = seqpack.seq_offsets_ref(torch.tensor(lens, dtype=torch.int32), S)
    g = torch.Generator().manual_seed(seed + S + len(name))
    qkv = torch.randn(Ta, 3 * H, generator=g, dtype=torch.float64)
    return lens, T, Ta, cu, qkv


def _per_record(qkv, lens):
    """each record alone: softmax(Q K^T / 8) V over its own n keys, no mask"""
    out = qkv.new_zeros(qkv.shape[0], H)
    t = 0
    for n in lens:
        for h in range(NH):
            q, k, v = (qkv[t:t + n, i * H + h * 64:i * H + (h + 1) * 64] for i in range(3))
            out[t:t + n, h * 64:(h + 1) * 64] = torch.softmax(q @ k.T / math.sqrt(64), -1) @ v
        t += n
    return out


@pytest.mark.parametrize("S", [192, 256])
@pytest.mark.parametrize("name", list(SETS))
def test_long_wrappers_take_the_mirror(name, S):
    lens, T, Ta, cu, qkv = _case(name, S)
    if name == "M1" and S == 256:
        assert (T, Ta) == (1103, 1152)
    if name == "M3" and S == 256:
        assert T == Ta == 1024 and 0 in lens
    ctx, lse = seqpack.attn_packed_long_fwd(qkv, cu, B, S, NH, 0.0, 0)
    assert lse is None and ctx.shape == (Ta, H)
    assert torch.equal(ctx, seqpack.attn_packed_ref(qkv, cu, B, S, NH))
    y = qkv.clone().requires_grad_(True)
    want = _per_record(y, lens)
    assert (ctx - want).abs().max().item() <= 1e-9
    assert not ctx[T:].any()  # the tail rows: exactly zero
    w = torch.randn(Ta, H, generator=torch.Generator().manual_seed(1), dtype=torch.float64)  # random on the tail too
    (gy,) = torch.autograd.grad(want, y, w)
    db = torch.ones(3 * H, dtype=torch.float64)
    dq = seqpack.attn_packed_long_bwd(qkv, ctx, w, None, cu, B, S, NH, 0.0, 0, dbias=db)
    assert dq.shape == (Ta, 3 * H) and (dq - gy).abs().max().item() <= 1e-9
    assert not dq[T:].any()  # nothing flows into (or out of) the tail rows
    assert (db - 1 - gy.sum(0)).abs().max().item() <= 1e-9  # added, not stored
    out = torch.full((Ta, 3 * H), float("nan"), dtype=torch.float64)
    res = seqpack.attn_packed_long_bwd(qkv, ctx, w, None, cu, B, S, NH, 0.0, 0, out=out)
    assert res is out and torch.equal(out, dq)


def test_empty_record_contributes_nothing():
    """M3 has two records of length 0: dropping them from the batch leaves the output and the gradient where they were
    (to 1e-9, the file's fp64 bound: the batched products of B and of B - 2 records may be blocked differently)"""
    S = 256
    lens, T, Ta, cu, qkv = _case("M3", S)
    rest = [n for n in lens if n]
    assert len(rest) == B - 2
    cu2 = seqpack.seq_offsets_ref(torch.tensor(rest, dtype=torch.int32), S)
    a, _ = seqpack.attn_packed_long_fwd(qkv, cu, B, S, NH, 0.1, 9)
    b, _ = seqpack.attn_packed_long_fwd(qkv, cu2, B - 2, S, NH, 0.0, 0)
    a0, _ = seqpack.attn_packed_long_fwd(qkv, cu, B, S, NH, 0.0, 0)
    assert (a0 - b).abs().max().item() <= 1e-9
    assert (a - a0).abs().max().item() > 1e-3  # (dropout is live in the wrapper)
    w = torch.randn(Ta, H, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    ga = seqpack.attn_packed_long_bwd(qkv, a0, w, None, cu, B, S, NH, 0.0, 0)
    gb = seqpack.attn_packed_long_bwd(qkv, b, w, None, cu2, B - 2, S, NH, 0.0, 0)
    assert (ga - gb).abs().max().item() <= 1e-9 and ga.abs().max().item() > 1e-3
