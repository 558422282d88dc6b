"""Streaming fused attention (csrc/kernels/attention_stream.hip, 512 < S <= attn_stream_max_s) against the plain
fp64 attention, and the fused BERT at S = 1088 against its fp32 reference model.  Bounds: those of
test_transformer_gpu.py::test_fused_attention_fwd_bwd, which holds the resident kernels to them at S = 512."""
import pytest
import torch

import dtg  # noqa: F401
from dtg.models.bert import BertConfig, BertForPreTraining, synthetic_batch
from dtg.ops import lib, transformer as T
from dtg.ops.seqpack import SeqPack

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


@pytest.mark.parametrize("S", [576, 640, 1088])  # 9, 10, 17 chunks: odd and even ring parity, a half-idle last block
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_stream_attention_fwd_bwd(S, p):
    torch.manual_seed(6)
    B, nh = 3, 2
    H = nh * 64
    qkv = (torch.randn(B * S, 3 * H, device=dev) * 1.5).bfloat16()
    am = torch.ones(B, S, device=dev)
    am[0, :64] = 0      # the first chunk all masked
    am[1, S - 9:] = 0   # a partial last chunk
    am[2, 70:] = 0      # every chunk after the second all masked
    mask = T.mask_additive(am)
    out, lse = lib().attn_fused_fwd(qkv, mask, B, S, nh, p, 1234)
    qr = qkv.double().requires_grad_()
    ref = T.attention_ref(qr, mask, B, S, nh, p, 1234)  # the same seed: a wrong dropout index is a gross error
    q, k, _ = qkv.double().view(B, S, 3, nh, 64).permute(2, 0, 3, 1, 4)
    ref_lse = torch.logsumexp((q @ k.transpose(-1, -2)) / 8.0 + mask.view(B, 1, 1, S), -1)
    dout = torch.randn(B * S, H, device=dev).bfloat16()
    ref.backward(dout.double())
    dqkv = lib().attn_fused_bwd(qkv, out, dout, lse, mask, B, S, nh, p, 1234)
    db = torch.full((3 * H,), 0.5, device=dev)
    dqkv2 = lib().attn_fused_bwd(qkv, out, dout, lse, mask, B, S, nh, p, 1234, db)
    e_out, e_lse = rel(out, ref), (lse.view(B, nh, S).double() - ref_lse).abs().max().item()
    e_g = [rel(dqkv[:, i * H:(i + 1) * H], qr.grad[:, i * H:(i + 1) * H]) for i in range(3)]
    e_db = rel(db, qr.grad.sum(0) + 0.5)
    print("[attn stream] S=%d p=%.1f rel out %.4f, max |dLSE| %.4f, rel dQ %.4f dK %.4f dV %.4f dbias %.4f" % (
        S, p, e_out, e_lse, *e_g, e_db))
    for t in (out, lse, dqkv, db):
        assert torch.isfinite(t).all()
    assert e_out < 1.5e-2
    assert e_lse <= 2e-2
    assert max(e_g) < 3e-2, e_g
    assert torch.equal(dqkv2, dqkv)  # the bias gradient is added on the side: the same dQKV bits
    assert e_db < 2e-2


@pytest.mark.parametrize("lengths", [None, [1088, 700]], ids=["padded", "repadded-pack"])
def test_bert_at_1088_matches_reference(lengths):
    """Beyond the unfused path's 1024 keys.  With a pack the encoder runs on packed rows and re-pads around the
    streaming attention; the reference model takes the same pack."""
    S, B = 1088, 2
    assert lib().attn_fused_supported(S, 64, True)
    cfg = BertConfig(vocab_size=1024, hidden=128, layers=2, heads=2, intermediate=512, max_position=S)
    torch.manual_seed(0)
    fused = BertForPreTraining(cfg).to(dev)
    for prm in fused.parameters():
        if prm.dim() == 2:
            prm.data = prm.data.bfloat16()
    ref = BertForPreTraining(cfg).to(dev)
    ref.load_state_dict({k: v.float() for k, v in fused.state_dict().items()})
    ref.fused = False
    ids, tt, am, pos, lab, nsp = synthetic_batch(B, S, cfg, dev, max_predictions=8, seed=5)
    pack = None
    if lengths is not None:
        ln = torch.tensor(lengths, dtype=torch.int32, device=dev)
        am = (torch.arange(S, device=dev).unsqueeze(0) < ln.unsqueeze(1)).long()
        pos = pos % (ln.long().unsqueeze(1) - 1) + 1  # predictions on real tokens
        pack = SeqPack.from_lengths(ln, lengths, S)
    batch = (ids, tt, am, pos, lab, nsp)
    assert fused.fused_ok(ids)
    lf, lr = fused(*batch, pack=pack), ref(*batch, pack=pack)
    assert abs(lf.item() - lr.item()) < 2e-2 * abs(lr.item())
    lf.backward()
    lr.backward()
    for (n, pf), pr in zip(fused.named_parameters(), ref.parameters()):
        assert rel(pf.grad, pr.grad) < 5e-2, n


@pytest.mark.parametrize("S", [600, "cap + 64"])
def test_unsupported_lengths_are_refused(S):
    S = lib().attn_stream_max_s() + 64 if S == "cap + 64" else S
    assert lib().attn_stream_max_s() >= 4096 and not lib().attn_fused_supported(S, 64, True)
    qkv = torch.zeros(S, 192, device=dev, dtype=torch.bfloat16)
    out = torch.zeros(S, 64, device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(S, device=dev)
    msg = r"S % 64 == 0 and 64 <= S <= {}".format(lib().attn_stream_max_s())
    with pytest.raises(RuntimeError, match=msg):
        lib().attn_fused_fwd(qkv, None, 1, S, 1, 0.0, 0)
    with pytest.raises(RuntimeError, match=msg):
        lib().attn_fused_bwd(qkv, out, out, lse, None, 1, S, 1, 0.0, 0)
