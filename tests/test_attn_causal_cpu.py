"""The causal option of the attention mirror, the CPU route of the causal entry points, and CausalLM's causality."""
import math

import pytest
import torch

import dtg  # noqa: F401
from dtg.models import BertConfig, CausalLM
from dtg.ops import transformer as T


def _qkv(B, S, nh, dh=8):
    torch.manual_seed(3)
    mask = torch.zeros(B, S)
    mask[1, S - 2:] = -10000.0
    return torch.randn(B * S, 3 * nh * dh, dtype=torch.float64), mask


def test_attention_ref_causal_matches_a_per_row_softmax():
    B, S, nh, dh = 2, 8, 2, 8
    qkv, mask = _qkv(B, S, nh)
    out = T.attention_ref(qkv, mask, B, S, nh, causal=True)
    x = qkv.view(B, S, 3, nh, dh)
    for b in range(B):
        for h in range(nh):
            for q in range(S):
                w = [math.exp(float(x[b, q, 0, h] @ x[b, k, 1, h]) / math.sqrt(dh) + float(mask[b, k]))
                     for k in range(q + 1)]
                row = sum(wk / sum(w) * x[b, k, 2, h] for k, wk in enumerate(w))
                assert torch.allclose(out[b * S + q, h * dh:(h + 1) * dh], row, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_ref_default_is_unchanged(p):
    B, S, nh, dh = 2, 8, 2, 8
    qkv, mask = _qkv(B, S, nh)
    q, k, v = qkv.view(B, S, 3, nh, dh).permute(2, 0, 3, 1, 4)
    pr = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(dh) + mask.view(B, 1, 1, S), dim=-1)
    pr = T.attn_dropout_ref(pr.reshape(-1, S), p, 5).view(B, nh, S, S)
    old = (pr @ v).permute(0, 2, 1, 3).reshape(B * S, nh * dh)  # the function's body before the keyword
    assert torch.equal(T.attention_ref(qkv, mask, B, S, nh, p, 5), old)
    assert torch.equal(T.attention_ref(qkv, mask, B, S, nh, p, 5, causal=False), old)


def test_causal_entry_points_on_cpu_are_the_mirror():
    B, S, nh = 2, 8, 2
    qkv, mask = _qkv(B, S, nh)
    out, lse = T.attn_causal_fwd(qkv, mask, B, S, nh, 0.1, 5)
    x = qkv.clone().requires_grad_()
    ref = T.attention_ref(x, mask, B, S, nh, 0.1, 5, causal=True)
    assert torch.equal(out, ref) and lse.shape == (B * nh * S,) and torch.isfinite(lse).all()
    dout = torch.randn_like(out)
    ref.backward(dout)
    db = torch.full((qkv.shape[1],), 0.5, dtype=torch.float64)
    assert torch.equal(T.attn_causal_bwd(qkv, out, dout, lse, mask, B, S, nh, 0.1, 5, db), x.grad)
    assert torch.allclose(db, x.grad.sum(0) + 0.5)


def test_causal_lm_logits_ignore_later_tokens():
    cfg = BertConfig.tiny()
    torch.manual_seed(0)
    model = CausalLM(cfg).eval()
    B, S, t = 2, 16, 9
    ids = torch.randint(0, cfg.vocab_size, (B, S))
    ids2 = ids.clone()
    ids2[:, t + 1:] = torch.randint(0, cfg.vocab_size, (B, S - t - 1))
    with torch.no_grad():
        a, b = model.logits(ids).view(B, S, -1), model.logits(ids2).view(B, S, -1)
        assert torch.equal(a[:, :t + 1], b[:, :t + 1]) and not torch.equal(a[:, t + 1:], b[:, t + 1:])
        labels = CausalLM.next_token_labels(ids, (torch.arange(S) < 12).long().expand(B, S))
        assert torch.equal(labels[:, :11], ids[:, 1:12]) and (labels[:, 11:] == -1).all()
        assert torch.isfinite(model(ids))
