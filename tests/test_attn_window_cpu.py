"""The window option of the attention mirror, the CPU route of the window entry points, and the training script's
refusal of --window without --causal."""
import importlib.util
import math
import os
import sys

import pytest
import torch

import dtg  # noqa: F401
from dtg.ops import transformer as T


def _qkv(B, S, nh, dh=8):
    torch.manual_seed(3)
    mask = torch.zeros(B, S)
    mask[1, S - 2:] = -10000.0
    return torch.randn(B * S, 3 * nh * dh, dtype=torch.float64), mask


def test_attention_ref_window_matches_a_per_row_softmax():
    B, S, nh, dh, W = 2, 8, 2, 8, 3  # (the mirror has none of the kernels' constraints on W)
    qkv, mask = _qkv(B, S, nh)
    out = T.attention_ref(qkv, mask, B, S, nh, causal=True, window=W)
    x = qkv.view(B, S, 3, nh, dh)
    for b in range(B):
        for h in range(nh):
            for q in range(S):
                keys = range(max(0, q - W + 1), q + 1)  # W keys, q itself included
                w = [math.exp(float(x[b, q, 0, h] @ x[b, k, 1, h]) / math.sqrt(dh) + float(mask[b, k])) for k in keys]
                row = sum(wk / sum(w) * x[b, k, 2, h] for k, wk in zip(keys, w))
                assert torch.allclose(out[b * S + q, h * dh:(h + 1) * dh], row, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("causal", [False, True])
def test_window_0_is_the_mirror_as_it_was(p, causal):
    B, S, nh, dh = 2, 8, 2, 8
    qkv, mask = _qkv(B, S, nh)
    q, k, v = qkv.view(B, S, 3, nh, dh).permute(2, 0, 3, 1, 4)
    sc = (q @ k.transpose(-1, -2)) / math.sqrt(dh) + mask.view(B, 1, 1, S)
    if causal:
        sc = sc.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    pr = T.attn_dropout_ref(torch.softmax(sc, dim=-1).reshape(-1, S), p, 5).view(B, nh, S, S)
    old = (pr @ v).permute(0, 2, 1, 3).reshape(B * S, nh * dh)  # the function's body before the keyword
    assert torch.equal(T.attention_ref(qkv, mask, B, S, nh, p, 5, causal=causal), old)
    assert torch.equal(T.attention_ref(qkv, mask, B, S, nh, p, 5, causal=causal, window=0), old)
    if causal:  # and a window that covers every key <= q changes nothing
        assert torch.equal(T.attention_ref(qkv, mask, B, S, nh, p, 5, causal=True, window=S), old)


def test_window_without_causal_raises():
    qkv, mask = _qkv(2, 8, 2)
    with pytest.raises(ValueError, match="needs causal=True"):
        T.attention_ref(qkv, mask, 2, 8, 2, window=3)


def test_window_entry_points_on_cpu_are_the_mirror():
    B, S, nh, W = 2, 8, 2, 3
    qkv, mask = _qkv(B, S, nh)
    out, lse = T.attn_window_fwd(qkv, mask, B, S, nh, W, 0.1, 5)
    x = qkv.clone().requires_grad_()
    ref = T.attention_ref(x, mask, B, S, nh, 0.1, 5, causal=True, window=W)
    assert torch.equal(out, ref) and lse.shape == (B * nh * S,) and torch.isfinite(lse).all()
    assert not torch.equal(out, T.attn_causal_fwd(qkv, mask, B, S, nh, 0.1, 5)[0])
    dout = torch.randn_like(out)
    ref.backward(dout)
    db = torch.full((qkv.shape[1],), 0.5, dtype=torch.float64)
    assert torch.equal(T.attn_window_bwd(qkv, out, dout, lse, mask, B, S, nh, W, 0.1, 5, db), x.grad)
    assert torch.allclose(db, x.grad.sum(0) + 0.5)


def test_bert_train_refuses_window_without_causal(capsys, monkeypatch):
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "BERT")
    monkeypatch.syspath_prepend(here)  # the script's ``import _path``
    spec = importlib.util.spec_from_file_location("bert_train_window", os.path.join(here, "bert_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules.pop("_path", None)
    with pytest.raises(SystemExit):
        mod.parse_args(["--window", "64"])
    assert "--window needs --causal" in capsys.readouterr().err
    assert mod.model_config(mod.parse_args(["--causal", "--window", "64"])).window == 64
    assert mod.model_config(mod.parse_args([])).window == 0
