"""The torch mirror of attn_extend against a per-row softmax, and CausalLM.extend / chunked prefill on the CPU (fp32,
the mirrors) against decode_step and the one-shot prefill."""
import math

import pytest
import torch

import dtg  # noqa: F401
from dtg.models import BertConfig, CausalLM, KVCache
from dtg.ops import transformer as T


@pytest.mark.parametrize("W", [0, 2, 5])  # 2: the window cuts inside the new block
def test_attn_extend_mirror_matches_a_per_row_softmax(W):
    torch.manual_seed(3)
    B, nh, dh, S_max, Tn, t = 3, 2, 8, 12, 4, 1
    lens0 = torch.tensor([4, -1, 1], dtype=torch.int32)  # len = 5, 0 (an empty cache) and 2
    n_new = torch.tensor([4, 3, 0], dtype=torch.int32)
    kc, vc = torch.randn(B, nh, S_max, dh, dtype=torch.float64), torch.randn(B, nh, S_max, dh, dtype=torch.float64)
    k0, v0 = kc.clone(), vc.clone()
    qkvT = torch.randn(B * Tn, 3 * nh * dh, dtype=torch.float64)
    ctx, lse = T.attn_extend(qkvT, lens0, t, 5, kc, vc, Tn, W, n_new)
    q, k, v = qkvT.view(B, Tn, 3, nh, dh).unbind(2)
    for b, (L, n) in enumerate(zip([5, 0, 2], n_new.tolist())):
        assert torch.equal(kc[b, :, L:L + n], k[b, :n].transpose(0, 1))  # the append, and nothing else
        assert torch.equal(vc[b, :, L:L + n], v[b, :n].transpose(0, 1))
        keep = (torch.arange(S_max) < L) | (torch.arange(S_max) >= L + n)
        assert torch.equal(kc[b][:, keep], k0[b][:, keep]) and torch.equal(vc[b][:, keep], v0[b][:, keep])
        assert (ctx.view(B, Tn, -1)[b, n:] == 0).all() and (lse[b, :, n:] == 0).all()
        for i in range(n):
            for h in range(nh):
                keys = range(max(0, L + i + 1 - W) if W else 0, L + i + 1)
                w = [math.exp(float(q[b, i, h] @ kc[b, h, j]) / math.sqrt(dh)) for j in keys]
                row = sum(wj / sum(w) * vc[b, h, j] for j, wj in zip(keys, w))
                assert torch.allclose(ctx.view(B, Tn, nh, dh)[b, i, h], row, rtol=1e-10, atol=1e-12)
                assert abs(float(lse[b, h, i]) - math.log(sum(w))) < 1e-5
    for bad_T, max_len, msg in ((0, 5, "T <= 64"), (65, 5, "T <= 64"), (Tn, S_max - Tn + 1, "cache is full")):
        with pytest.raises(ValueError, match=msg):
            T.attn_extend(qkvT, lens0, t, max_len, kc, vc, bad_T, W)


def _model(window, max_position=100):
    cfg = BertConfig(vocab_size=512, hidden=64, layers=2, heads=2, intermediate=256, max_position=max_position,
                     window=window)
    torch.manual_seed(1)
    return CausalLM(cfg).eval(), cfg


@pytest.mark.parametrize("window", [0, 4])
def test_extend_is_decode_steps_and_chunked_prefill_is_prefill(window):
    model, cfg = _model(window, max_position=128)  # the one-shot prefill pads 70 tokens to 128
    lengths, Tn = [3, 70, 41], 6
    ids = torch.randint(0, 512, (3, 70 + Tn))
    nxt = torch.stack([ids[b, n:n + Tn] for b, n in enumerate(lengths)])
    c0, c1, c2 = (KVCache(cfg, 3, 90, dtype=torch.float32) for _ in range(3))
    first = model.prefill(ids[:, :70], lengths, c0)
    for chunk, c in ((16, c1), (64, c2)):  # mixed lengths: records end in different pieces
        assert torch.allclose(model.prefill(ids[:, :70], lengths, c, chunk=chunk), first, atol=1e-5)
        assert c.max_len == 70 and c.t == 0 and c.lens0.tolist() == lengths
    steps = torch.stack([model.decode_step(nxt[:, i], c0) for i in range(Tn)], 1)
    assert torch.allclose(model.extend(nxt, c1), steps, atol=1e-5)
    assert c1.max_len == c0.max_len == 70 + Tn
    for b, n in enumerate(lengths):
        assert torch.allclose(c1.k[1][b, :, :n + Tn], c0.k[1][b, :, :n + Tn], atol=1e-5)
    with pytest.raises(ValueError, match="beyond the cache"):
        model.extend(ids[:, :15], c1)


def test_a_prompt_of_max_position_tokens_and_generate():
    model, cfg = _model(0, max_position=100)  # 100 is no multiple of 64: the one-shot prefill pads to 128 and refuses
    ids = torch.randint(0, 512, (2, 100))
    cache = KVCache(cfg, 2, 100, dtype=torch.float32)
    with pytest.raises(ValueError, match="position table"):
        model.prefill(ids, [100, 37], cache)
    got = model.prefill(ids, [100, 37], cache, chunk=48)
    with torch.no_grad():
        want = torch.stack([model.logits(ids[b:b + 1, :n])[-1] for b, n in enumerate([100, 37])])
    assert torch.allclose(got, want, atol=1e-4)
    model.train()
    before = [p.detach().clone() for p in model.parameters()]
    out = model.generate(ids[:, :60], [60, 37], 4, prefill_chunk=16)
    assert torch.equal(out, model.generate(ids[:, :60], [60, 37], 4))
    assert model.training and all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
