"""Sliding-window causal fused attention (csrc/kernels/attention_window.hip) against the plain fp64 attention, its
exclusion at both edges bit for bit, W >= S against the causal kernels, its refusals, and a CausalLM with a window
fused against its fp32 reference model.  Bounds: those test_attn_causal_gpu.py holds the causal kernels to."""
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


# (192, 64): an odd first chunk, the edge chunk next to the diagonal one, a half-idle last block; (640, 128): an even
# first chunk, dKV loops cut at both ends; (640, 320): odd W/64, blocks without and with a lower edge
@pytest.mark.parametrize("S,W", [(192, 64), (640, 128), (640, 320)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_window_attention_fwd_bwd(S, W, p):
    torch.manual_seed(6)
    B, nh = 3, 2
    H = nh * 64
    qkv = (torch.randn(B * S, 3 * H, device=dev) * 1.5).bfloat16()
    am = torch.ones(B, S, device=dev)
    am[1, S - 9:] = 0
    am[2, S // 2 + 6:] = 0
    mask = T.mask_additive(am)
    out, lse = T.attn_window_fwd(qkv, mask, B, S, nh, W, p, 1234)
    qr = qkv.double().requires_grad_()
    ref = T.attention_ref(qr, mask, B, S, nh, p, 1234, causal=True, window=W)  # the same seed, the [S, S] draw
    q, k, _ = qkv.double().view(B, S, 3, nh, 64).permute(2, 0, 3, 1, 4)
    sc = (q @ k.transpose(-1, -2)) / 8.0 + mask.view(B, 1, 1, S)
    d = torch.arange(S, device=dev).view(S, 1) - torch.arange(S, device=dev).view(1, S)  # q - key
    ref_lse = torch.logsumexp(sc.masked_fill((d < 0) | (d >= W), -1e300), -1)
    dout = torch.randn(B * S, H, device=dev).bfloat16()
    ref.backward(dout.double())
    dqkv = T.attn_window_bwd(qkv, out, dout, lse, mask, B, S, nh, W, p, 1234)
    db = torch.full((3 * H,), 0.5, device=dev)
    dqkv2 = T.attn_window_bwd(qkv, out, dout, lse, mask, B, S, nh, W, p, 1234, db)
    e_out, e_lse = rel(out, ref), (lse.view(B, nh, S).double() - ref_lse).abs().max().item()
    e_g = [rel(dqkv[:, i * H:(i + 1) * H], qr.grad[:, i * H:(i + 1) * H]) for i in range(3)]
    e_db = rel(db, qr.grad.sum(0) + 0.5)
    print("[attn window] S=%d W=%d p=%.1f rel out %.4f, max |dLSE| %.4f, rel dQ %.4f dK %.4f dV %.4f dbias %.4f" % (
        S, W, p, e_out, e_lse, *e_g, e_db))
    for t in (out, lse, dqkv, db):
        assert torch.isfinite(t).all()
    assert e_out < 1.5e-2
    assert e_lse <= 2e-2
    assert max(e_g) < 3e-2, e_g
    assert torch.equal(dqkv2, dqkv)  # the bias gradient is added on the side: the same dQKV bits
    assert e_db < 2e-2


# rows 0 .. 99 are below the window of rows >= 227 (227 - 128 = 99: a boundary inside a 16-row fragment and a chunk);
# rows >= 250 are the future of rows < 250
@pytest.mark.parametrize("lo,hi,keep,fill", [(0, 100, (227, 320), "random"), (250, 320, (0, 250), "nan"),
                                             (0, 100, (227, 320), "nan")],
                         ids=["below-random", "above-nan", "below-nan"])
def test_keys_outside_the_window_do_not_reach_a_row(lo, hi, keep, fill):
    """out and LSE of record 1's rows ``keep`` (and all of record 0) keep their bits whatever K and V hold on its rows
    lo .. hi - 1: an excluded element is excluded, not multiplied by zero -- in the forward at both edges."""
    torch.manual_seed(7)
    B, S, W, nh = 2, 320, 128, 2
    H = nh * 64
    qkv = (torch.randn(B * S, 3 * H, device=dev) * 1.5).bfloat16()
    out, lse = lib().attn_window_fwd(qkv, None, B, S, nh, W, 0.1, 99)
    qkv2 = qkv.clone()
    kv = qkv2[S + lo:S + hi, H:]  # record 1, the K and V segments
    kv.copy_(torch.randn_like(kv) * 2 if fill == "random" else torch.full_like(kv, float("nan")))
    out2, lse2 = lib().attn_window_fwd(qkv2, None, B, S, nh, W, 0.1, 99)
    rows = slice(S + keep[0], S + keep[1])
    l1, l2 = lse.view(B, nh, S), lse2.view(B, nh, S)
    assert torch.isfinite(out2[rows]).all() and torch.isfinite(l2[1, :, keep[0]:keep[1]]).all()
    assert torch.equal(out2[rows], out[rows]) and torch.equal(out2[:S], out[:S])
    assert torch.equal(l2[1, :, keep[0]:keep[1]], l1[1, :, keep[0]:keep[1]]) and torch.equal(l2[0], l1[0])


@pytest.mark.parametrize("W", [192, 256])
def test_a_window_of_the_whole_sequence_is_causal_attention(W):
    torch.manual_seed(8)
    B, S, nh = 2, 192, 2
    qkv = (torch.randn(B * S, 3 * nh * 64, device=dev) * 1.5).bfloat16()
    dout = torch.randn(B * S, nh * 64, device=dev).bfloat16()
    mask = T.mask_additive((torch.arange(S, device=dev).view(1, S) < torch.tensor([[S], [150]], device=dev)).float())
    out, lse = T.attn_window_fwd(qkv, mask, B, S, nh, W, 0.1, 5)
    outc, lsec = T.attn_causal_fwd(qkv, mask, B, S, nh, 0.1, 5)
    assert torch.equal(out, outc) and torch.equal(lse, lsec)
    assert torch.equal(T.attn_window_bwd(qkv, out, dout, lse, mask, B, S, nh, W, 0.1, 5),
                       T.attn_causal_bwd(qkv, outc, dout, lsec, mask, B, S, nh, 0.1, 5))


@pytest.mark.parametrize("S,W,width,msg", [(128, 96, 192, r"window % 64 == 0 and window >= 64"),
                                           (128, 0, 192, r"window % 64 == 0 and window >= 64"),
                                           (600, 64, 192, r"S % 64 == 0, 64 <= S <= "),
                                           (128, 64, 160, r"\[B\*S, 3\*nh\*64\]")])
def test_unsupported_shapes_are_refused(S, W, width, msg):
    assert lib().attn_window_supported(128, 64, 64) and (width != 192 or not lib().attn_window_supported(S, W, 64))
    qkv = torch.zeros(S, width, device=dev, dtype=torch.bfloat16)
    out = torch.zeros(S, 64, device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(S, device=dev)
    with pytest.raises(RuntimeError, match=msg):
        lib().attn_window_fwd(qkv, None, 1, S, 1, W, 0.0, 0)
    with pytest.raises(RuntimeError, match=msg):
        lib().attn_window_bwd(qkv, out, out, lse, None, 1, S, 1, W, 0.0, 0)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "repadded-pack"])
def test_window_lm_matches_reference(packed):
    S, B, lengths = 192, 2, [192, 131]
    cfg = BertConfig(vocab_size=1024, hidden=128, layers=2, heads=2, intermediate=512, max_position=S, window=64)
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
    assert fused.fused_ok(ids) and fused.cfg.causal and fused.cfg.window == 64 and fused.training
    lf, lr = fused(ids, am, pack=pack), ref(ids, am, pack=pack)
    print("[window lm] loss fused %.5f reference %.5f" % (lf.item(), lr.item()))
    assert abs(lf.item() - lr.item()) < 2e-2 * abs(lr.item())
    lf.backward()
    lr.backward()
    for (n, pf), pr in zip(fused.named_parameters(), ref.parameters()):
        assert (pf.grad is None) == (pr.grad is None), n  # the pooler / NSP weights: in neither
        if pr.grad is not None:
            assert rel(pf.grad, pr.grad) < 5e-2, n
    if not packed:  # the window is in effect in the fused layers: two of them reach 2 * 63 tokens back and no further
        ids2 = ids.clone()
        ids2[:, :65] = (ids[:, :65] + 1) % 1000
        with torch.no_grad():
            a, b = fused.logits(ids).view(B, S, -1), fused.logits(ids2).view(B, S, -1)
        assert torch.equal(a[:, 191], b[:, 191]) and not torch.equal(a[:, 190], b[:, 190])
