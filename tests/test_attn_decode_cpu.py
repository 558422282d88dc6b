"""The torch mirror of attn_decode against a per-row softmax, and CausalLM.generate on the CPU (fp32, the mirrors)
against the loop the model offered before it: argmax of ``logits(prefix)[last]``, append."""
import math

import pytest
import torch

import dtg  # noqa: F401
from dtg.models import BertConfig, CausalLM
from dtg.ops import transformer as T


def test_attn_decode_mirror_matches_a_per_row_softmax():
    torch.manual_seed(2)
    B, nh, dh, S_max, W, t = 2, 2, 8, 8, 3, 1
    lens0 = torch.tensor([4, 1], dtype=torch.int32)  # len = 5 and 2: a window that cuts, and one that does not
    kc, vc = torch.randn(B, nh, S_max, dh, dtype=torch.float64), torch.randn(B, nh, S_max, dh, dtype=torch.float64)
    k0, v0 = kc.clone(), vc.clone()
    qkv1 = torch.randn(B, 3 * nh * dh, dtype=torch.float64)
    ctx, lse = T.attn_decode(qkv1, lens0, t, 5, kc, vc, W)
    q, k, v = qkv1.view(B, 3, nh, dh).unbind(1)
    for b, n in enumerate([5, 2]):
        assert torch.equal(kc[b, :, n], k[b]) and torch.equal(vc[b, :, n], v[b])  # the append, and nothing else
        keep = torch.arange(S_max) != n
        assert torch.equal(kc[b][:, keep], k0[b][:, keep]) and torch.equal(vc[b][:, keep], v0[b][:, keep])
        for h in range(nh):
            keys = range(max(0, n + 1 - W), n + 1)  # W keys, the token's own (position n) included
            w = [math.exp(float(q[b, h] @ kc[b, h, j]) / math.sqrt(dh)) for j in keys]
            row = sum(wj / sum(w) * vc[b, h, j] for j, wj in zip(keys, w))
            assert torch.allclose(ctx[b, h * dh:(h + 1) * dh], row, rtol=1e-10, atol=1e-12)
            assert abs(float(lse[b, h]) - math.log(sum(w))) < 1e-5
    with pytest.raises(ValueError, match="cache is full"):
        T.attn_decode(qkv1, lens0, t, S_max, kc, vc, W)


@pytest.mark.parametrize("window", [0, 4])
def test_generate_is_the_full_forward_loop(window):
    cfg = BertConfig(vocab_size=512, hidden=64, layers=2, heads=2, intermediate=256, max_position=64, window=window)
    torch.manual_seed(1)
    model = CausalLM(cfg)  # fp32 on the CPU: every step runs the mirrors; training mode, which generate must restore
    before = [p.detach().clone() for p in model.parameters()]
    lengths, new = [3, 7, 5], 6
    ids = torch.randint(0, 512, (3, 7))
    out = model.generate(ids, lengths, new)
    assert out.shape == (3, new) and out.dtype == torch.int64
    assert model.training and all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
    model.eval()
    want = []
    with torch.no_grad():
        for b, n in enumerate(lengths):
            seq = ids[b, :n]
            for _ in range(new):
                seq = torch.cat([seq, model.logits(seq.unsqueeze(0))[-1].argmax().view(1)])
            want.append(seq[n:])
    want = torch.stack(want)
    assert torch.equal(out, want)
    eos = int(want[0, 1])  # record 0 ends after two tokens; the others where they happen to produce it, if at all
    ended = (want == eos).cumsum(1) > 0
    assert ended[0, 1:].all() and not ended[0, 0]
    assert torch.equal(model.generate(ids, lengths, new, eos_id=eos), torch.where(ended, eos, want))


@pytest.mark.parametrize("lengths,new,msg", [([3, 0, 5], 4, "lengths in"), ([3, 7, 5], 58, "max_position")])
def test_generate_refusals(lengths, new, msg):
    model = CausalLM(BertConfig.tiny())
    with pytest.raises(ValueError, match=msg):
        model.generate(torch.zeros(3, 7, dtype=torch.int64), lengths, new)
