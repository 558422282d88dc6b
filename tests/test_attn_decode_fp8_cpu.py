"""The FP8 KV cache's torch mirrors: the quantiser, attn_decode against a per-row softmax, KVCache, generate."""
import math

import pytest
import torch

import dtg  # noqa: F401
from dtg.models import BertConfig, CausalLM, KVCache
from dtg.ops import transformer as T

FP8 = torch.float8_e4m3fn


def test_quantiser_round_trips_within_half_an_ulp():
    """Half an e4m3 ulp: 2^-4 |c| at most for a normal code, 2^-10 below 2^-6; the row's largest element lands on 448"""
    torch.manual_seed(0)
    x = (torch.randn(40, 64) * torch.logspace(-3, 3, 40).unsqueeze(1)).bfloat16()
    x[3] = 0
    x[5, 1:] *= 1e-4  # one large element: the others fall into the subnormal codes and to zero
    codes, scale = T.kv_quantize(x)
    assert codes.dtype == FP8 and scale.dtype == torch.float32 and scale[3] == 1 and (codes[3].float() == 0).all()
    ratio = (x.float() / scale.unsqueeze(1)).abs()
    err = (T.kv_dequantize(codes, scale) - x.float()).abs()
    assert (err <= scale.unsqueeze(1) * 2.0 ** -4 * ratio.clamp_min(2.0 ** -6)).all()
    assert (codes.float().abs().amax(1)[torch.arange(40) != 3] == 448).all()


def test_attn_decode_mirror_with_an_fp8_cache_matches_a_per_row_softmax():
    torch.manual_seed(2)
    B, nh, dh, S_max, W, t = 2, 2, 8, 8, 3, 1
    lens0 = torch.tensor([4, 1], dtype=torch.int32)  # len = 5 and 2: a window that cuts, and one that does not
    (kc, ks), (vc, vs) = (T.kv_quantize(torch.randn(B, nh, S_max, dh)) for _ in range(2))
    kd, vd = T.kv_dequantize(kc, ks), T.kv_dequantize(vc, vs)
    qkv1 = torch.randn(B, 3 * nh * dh)
    ctx, lse = T.attn_decode(qkv1, lens0, t, 5, kc, vc, W, ks, vs)
    q, k, v = qkv1.view(B, 3, nh, dh).unbind(1)
    for b, n in enumerate([5, 2]):
        for x, new in zip((kc, ks, vc, vs), T.kv_quantize(k[b]) + T.kv_quantize(v[b])):  # the append
            assert torch.equal(x[b, :, n].float(), new.float())
        kd[b, :, n], vd[b, :, n] = k[b], v[b]  # the token itself: unquantised in this step
        for h in range(nh):
            keys = range(max(0, n + 1 - W), n + 1)
            w = [math.exp(float(q[b, h] @ kd[b, h, j]) / math.sqrt(dh)) for j in keys]
            row = sum(wj / sum(w) * vd[b, h, j] for j, wj in zip(keys, w))
            assert torch.allclose(ctx[b, h * dh:(h + 1) * dh], row, rtol=1e-5, atol=1e-6)
            assert abs(float(lse[b, h]) - math.log(sum(w))) < 1e-5
    for c, s, msg in ((kc, None, "needs its kscale / vscale"), (kd, vs, "takes no kscale")):
        with pytest.raises(ValueError, match=msg):
            T.attn_decode(qkv1, lens0, t, 5, c, c.clone(), W, ks, s)


def test_kv_cache_scales_and_generate_with_an_fp8_cache():
    cfg = BertConfig(vocab_size=512, hidden=64, layers=2, heads=2, intermediate=256, max_position=64)
    c = KVCache(cfg, 3, 16, dtype=FP8)
    for x, s in zip(c.k + c.v, c.k_scale + c.v_scale):
        assert x.dtype == FP8 and s.dtype == torch.float32 and s.shape == x.shape[:3]
    for dt in (torch.bfloat16, torch.float32):
        assert KVCache(cfg, 3, 16, dtype=dt).k_scale == KVCache(cfg, 3, 16, dtype=dt).v_scale == [None] * cfg.layers
    torch.manual_seed(1)
    model = CausalLM(cfg)  # fp32 on the CPU, training mode, which generate must restore
    before = [p.detach().clone() for p in model.parameters()]
    ids = torch.randint(0, 512, (3, 7))
    out = model.generate(ids, [3, 7, 5], 6, cache_dtype=FP8)
    assert out.shape == (3, 6) and out.dtype == torch.int64 and ((out >= 0) & (out < 512)).all()
    assert model.training and all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
    with pytest.raises(ValueError, match="prefill_chunk"):
        model.generate(ids, [3, 7, 5], 6, prefill_chunk=4, cache_dtype=FP8)
