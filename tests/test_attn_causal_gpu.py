"""Causal fused attention (csrc/kernels/attention_causal.hip) against the plain fp64 attention, its causality bit for
bit, its refusals, and CausalLM fused against its fp32 reference model.  Bounds: those test_attn_stream_gpu.py holds the
streaming kernels to."""
import pytest
import torch

import dtg  # noqa: F401
from dtg.models import BertConfig, CausalLM
from dtg.ops import lib, transformer as T
from dtg.ops.seqpack import SeqPack

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


# 64: one diagonal chunk, waves 4..7 beyond S; 192: an odd chunk count, a half-idle last block, 3- and 1-chunk dKV
# loops; 640: five blocks, every loop length from 2 to 10
@pytest.mark.parametrize("S", [64, 192, 640])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_causal_attention_fwd_bwd(S, p):
    torch.manual_seed(6)
    B, nh = 3, 2
    H = nh * 64
    qkv = (torch.randn(B * S, 3 * H, device=dev) * 1.5).bfloat16()
    am = torch.ones(B, S, device=dev)
    am[1, S - 9:] = 0
    am[2, S // 2 + 6:] = 0
    mask = T.mask_additive(am)
    out, lse = T.attn_causal_fwd(qkv, mask, B, S, nh, p, 1234)
    qr = qkv.double().requires_grad_()
    ref = T.attention_ref(qr, mask, B, S, nh, p, 1234, causal=True)  # the same seed: a wrong dropout index is gross
    q, k, _ = qkv.double().view(B, S, 3, nh, 64).permute(2, 0, 3, 1, 4)
    sc = (q @ k.transpose(-1, -2)) / 8.0 + mask.view(B, 1, 1, S)
    ref_lse = torch.logsumexp(sc.masked_fill(torch.ones(S, S, dtype=torch.bool, device=dev).triu(1), -1e300), -1)
    dout = torch.randn(B * S, H, device=dev).bfloat16()
    ref.backward(dout.double())
    dqkv = T.attn_causal_bwd(qkv, out, dout, lse, mask, B, S, nh, p, 1234)
    db = torch.full((3 * H,), 0.5, device=dev)
    dqkv2 = T.attn_causal_bwd(qkv, out, dout, lse, mask, B, S, nh, p, 1234, db)
    e_out, e_lse = rel(out, ref), (lse.view(B, nh, S).double() - ref_lse).abs().max().item()
    e_g = [rel(dqkv[:, i * H:(i + 1) * H], qr.grad[:, i * H:(i + 1) * H]) for i in range(3)]
    e_db = rel(db, qr.grad.sum(0) + 0.5)
    print("[attn causal] S=%d p=%.1f rel out %.4f, max |dLSE| %.4f, rel dQ %.4f dK %.4f dV %.4f dbias %.4f" % (
        S, p, e_out, e_lse, *e_g, e_db))
    for t in (out, lse, dqkv, db):
        assert torch.isfinite(t).all()
    assert e_out < 1.5e-2
    assert e_lse <= 2e-2
    assert max(e_g) < 3e-2, e_g
    assert torch.equal(dqkv2, dqkv)  # the bias gradient is added on the side: the same dQKV bits
    assert e_db < 2e-2


@pytest.mark.parametrize("fill", ["random", "nan"])
def test_future_keys_do_not_reach_earlier_rows(fill):
    """Rows < 70 of a record (a boundary inside a 16-row fragment and inside a chunk) keep their out and LSE bits
    whatever K and V hold on rows >= 70: an excluded element is excluded, not multiplied by zero."""
    torch.manual_seed(7)
    B, S, nh, cut = 2, 192, 2, 70
    H = nh * 64
    qkv = (torch.randn(B * S, 3 * H, device=dev) * 1.5).bfloat16()
    out, lse = lib().attn_causal_fwd(qkv, None, B, S, nh, 0.1, 99)
    qkv2 = qkv.clone()
    kv = qkv2[S + cut:2 * S, H:]  # record 1, rows >= cut, the K and V segments
    kv.copy_(torch.randn_like(kv) * 2 if fill == "random" else torch.full_like(kv, float("nan")))
    out2, lse2 = lib().attn_causal_fwd(qkv2, None, B, S, nh, 0.1, 99)
    assert torch.isfinite(out2[S:S + cut]).all() and torch.isfinite(lse2.view(B, nh, S)[1, :, :cut]).all()
    assert torch.equal(out2[:S + cut], out[:S + cut])
    assert torch.equal(lse2.view(B, nh, S)[1, :, :cut], lse.view(B, nh, S)[1, :, :cut])
    assert torch.equal(lse2.view(B, nh, S)[0], lse.view(B, nh, S)[0])


@pytest.mark.parametrize("S,width,msg", [(600, 192, r"S % 64 == 0 and 64 <= S <= "), ("cap + 64", 192, r"64 <= S <= "),
                                         (128, 160, r"\[B\*S, 3\*nh\*64\]")])
def test_unsupported_shapes_are_refused(S, width, msg):
    S = lib().attn_stream_max_s() + 64 if S == "cap + 64" else S
    assert lib().attn_causal_supported(128, 64) and (width != 192 or not lib().attn_causal_supported(S, 64))
    qkv = torch.zeros(S, width, device=dev, dtype=torch.bfloat16)
    out = torch.zeros(S, 64, device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(S, device=dev)
    with pytest.raises(RuntimeError, match=msg):
        lib().attn_causal_fwd(qkv, None, 1, S, 1, 0.0, 0)
    with pytest.raises(RuntimeError, match=msg):
        lib().attn_causal_bwd(qkv, out, out, lse, None, 1, S, 1, 0.0, 0)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "repadded-pack"])
def test_causal_lm_matches_reference(packed):
    S, B, lengths = 192, 2, [192, 131]
    cfg = BertConfig(vocab_size=1024, hidden=128, layers=2, heads=2, intermediate=512, max_position=S)
    torch.manual_seed(0)
    fused = CausalLM(cfg).to(dev)
    for prm in fused.parameters():
        if prm.dim() == 2:
            prm.data = prm.data.bfloat16()
    ref = CausalLM(cfg).to(dev)
    ref.load_state_dict({k: v.float() for k, v in fused.state_dict().items()})
    ref.fused = False
    ids = torch.randint(0, 1000, (B, S), device=dev)
    ln = torch.tensor(lengths, dtype=torch.int32, device=dev)
    am = (torch.arange(S, device=dev).unsqueeze(0) < ln.unsqueeze(1)).long()
    pack = SeqPack.from_lengths(ln, lengths, S) if packed else None
    assert fused.fused_ok(ids) and fused.cfg.causal and fused.training
    lf, lr = fused(ids, am, pack=pack), ref(ids, am, pack=pack)
    print("[causal lm] loss fused %.5f reference %.5f" % (lf.item(), lr.item()))
    assert abs(lf.item() - lr.item()) < 2e-2 * abs(lr.item())
    lf.backward()
    lr.backward()
    for (n, pf), pr in zip(fused.named_parameters(), ref.parameters()):
        assert (pf.grad is None) == (pr.grad is None), n  # the pooler / NSP weights: in neither
        if pr.grad is not None:
            assert rel(pf.grad, pr.grad) < 5e-2, n
