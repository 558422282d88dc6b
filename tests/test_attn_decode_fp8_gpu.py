"""The FP8 KV cache (csrc/kernels/attention_decode_fp8.hip) against fp64 over the dequantised rows (quantisation is on
both sides: the bounds are tests/test_attn_decode_gpu.py's) and, bit for bit, against the torch quantiser run on the
CPU.  Measured values: profiles/attn_decode_fp8/test_errors.txt."""
import functools

import pytest
import torch

import dtg  # noqa: F401
from dtg.models import BertConfig, CausalLM, KVCache
from dtg.ops import lib, transformer as T

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
NH, H, FP8 = 3, 192, torch.float8_e4m3fn
LENS = {300: [0, 1, 15, 16, 17, 63, 64], 1100: [65, 127, 640, 1099]}  # a batch per cache size; a load is 16 rows
u8 = lambda x: x.view(torch.uint8)  # noqa: E731


@functools.lru_cache(None)
def _case(S_max):
    """-> rows [B, S_max, 3H] (row len_b is the new token), qkv1, lens0, t, (kc, ks, vc, vs): every row quantised"""
    lens = LENS[S_max]
    B, t = len(lens), min(lens)
    rows = (torch.randn(B, S_max, 3 * H, generator=torch.Generator().manual_seed(S_max)) * 1.5).bfloat16()
    x = rows.view(B, S_max, 3, NH, 64)
    cache = T.kv_quantize(x[:, :, 1].transpose(1, 2)) + T.kv_quantize(x[:, :, 2].transpose(1, 2))
    qkv1 = torch.stack([rows[b, n] for b, n in enumerate(lens)])
    ln = torch.tensor(lens, dtype=torch.int32)
    return rows.to(dev), qkv1.to(dev), (ln - t).to(dev), t, tuple(c.contiguous().to(dev) for c in cache)


@functools.lru_cache(None)
def _reference(S_max, window):
    """fp64 (ctx [B, H], lse [B, NH]) of the new token of each record over the dequantised rows"""
    rows, _, _, _, (kc, ks, vc, vs) = _case(S_max)
    ctx, lse = [], []
    for b, n in enumerate(LENS[S_max]):
        seq = rows[b, :n + 1].double()
        seq[:n, H:2 * H] = T.kv_dequantize(kc[b, :, :n], ks[b, :, :n]).double().transpose(0, 1).reshape(n, H)
        seq[:n, 2 * H:] = T.kv_dequantize(vc[b, :, :n], vs[b, :, :n]).double().transpose(0, 1).reshape(n, H)
        ctx.append(T.attention_ref(seq, None, 1, n + 1, NH, causal=True, window=window)[-1])
        lo = max(0, n + 1 - window) if window else 0
        q, k = seq[-1, :H].view(NH, 1, 64), seq[lo:, H:2 * H].view(-1, NH, 64).transpose(0, 1)
        lse.append(torch.logsumexp((q @ k.transpose(1, 2)).squeeze(1) / 8.0, -1))
    return torch.stack(ctx), torch.stack(lse)


def _decode(S_max, window, nsplit, cache=None):
    _, qkv1, lens0, t, cache0 = _case(S_max)
    kc, ks, vc, vs = cache = cache or tuple(c.clone() for c in cache0)
    lib().attn_decode_force_splits(nsplit)
    try:
        ctx, lse = T.attn_decode(qkv1, lens0, t, max(LENS[S_max]), kc, vc, window, ks, vs)
    finally:
        lib().attn_decode_force_splits(0)
    return ctx, lse, cache


@pytest.mark.parametrize("nsplit", [0, 1, 5])  # the launcher's choice, no combine, empty splits
@pytest.mark.parametrize("window", [0, 64, 200])
@pytest.mark.parametrize("S_max", [300, 1100])
def test_attn_decode_fp8_against_fp64_and_append(S_max, window, nsplit):
    _, qkv1, _, _, cache0 = _case(S_max)
    ctx, lse, cache = _decode(S_max, window, nsplit)
    ref, ref_lse = _reference(S_max, window)
    e_out = ((ctx.double() - ref).norm() / ref.norm()).item()
    e_lse = (lse.double() - ref_lse).abs().max().item()
    print("[attn decode fp8] S_max=%d W=%d nsplit=%d out %.2e, |dLSE| %.2e" % (S_max, window, nsplit, e_out, e_lse))
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    assert e_out < 1.5e-2 and e_lse <= 2e-2
    k, v = qkv1.cpu().view(-1, 3, NH, 64)[:, 1], qkv1.cpu().view(-1, 3, NH, 64)[:, 2]
    want = [w.to(dev) for w in T.kv_quantize(k) + T.kv_quantize(v)]  # the CPU quantiser: codes, scale, codes, scale
    for b, n in enumerate(LENS[S_max]):  # rows < len and > len as they were, row len the token's codes and scales
        for c, c0, w in zip(cache, cache0, want):
            c, c0, w = (u8(x) if x.dtype == FP8 else x.view(torch.int32) for x in (c, c0, w))
            assert torch.equal(c[b, :, :n], c0[b, :, :n]) and torch.equal(c[b, :, n + 1:], c0[b, :, n + 1:])
            assert torch.equal(c[b, :, n], w[b])


@pytest.mark.parametrize("window,fill", [(64, "random"), (64, "nan"), (64, "inf"), (0, "nan"), (0, "inf")])
def test_excluded_rows_and_scales_never_reach_the_result(window, fill):
    """window 64: rows < 577 of record 2 (len 640) may hold anything (NaN code 0x7f); window 0: rows > len of each"""
    ctx, lse, _ = _decode(1100, window, 5)
    cache = tuple(c.clone() for c in _case(1100)[4])
    spans = [(2, slice(0, 577))] if window else [(b, slice(n + 1, None)) for b, n in enumerate(LENS[1100])]
    for b, rows in spans:
        for c in cache:
            if c.dtype == FP8:
                u8(c)[b, :, rows] = torch.randint_like(u8(c)[b, :, rows], 0, 127) if fill == "random" else 0x7f
            else:
                c[b, :, rows] = torch.randn_like(c[b, :, rows]) * 9 if fill == "random" else float(fill)
    ctx2, lse2, _ = _decode(1100, window, 5, cache)
    assert torch.isfinite(ctx2).all() and torch.equal(ctx2, ctx) and torch.equal(lse2, lse)


@pytest.mark.parametrize("window", [0, 200])
def test_split_invariance(window):
    """Forced 1 against 5, within the bound tests/test_attn_decode_gpu.py derives from the combine"""
    vmax = T.kv_dequantize(*_case(1100)[4][2:]).abs().max().item()
    ctx, lse, _ = _decode(1100, window, 1)
    ctx2, lse2, _ = _decode(1100, window, 5)
    d = (ctx2.float() - ctx.float()).abs()
    assert (d <= 2.0 ** -7 * ctx.float().abs() + 64 * 2.0 ** -24 * vmax).all(), d.max().item()
    assert (lse2 - lse).abs().max().item() <= 1e-5


@pytest.mark.parametrize("S_max", [200, 66])  # above S0, and below it: record 3 is cut at 66 rows
def test_kv_cache_fill_fp8_is_the_quantiser(S_max):
    B, S0, lens = 4, 128, [0, 5, 64, 70]
    qkv = torch.randn(B * S0, 3 * H, generator=torch.Generator().manual_seed(3)).bfloat16()
    x = qkv.view(B, S0, 3, NH, 64)
    x[1, 2, 1:, 0] = 0  # an all-zero K row and V row: scale 1, codes 0
    kc = torch.full((B, NH, S_max, 64), 0x55, dtype=torch.uint8, device=dev).view(FP8)
    ks = torch.full((B, NH, S_max), 7.0, device=dev)
    vc, vs = kc.clone(), ks.clone()
    T.kv_cache_fill(qkv.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), kc, vc, B, S0, NH, ks, vs)
    assert ks[1, 0, 2] == 1 and (u8(kc)[1, 0, 2] == 0).all()
    for b, n in enumerate(lens):
        n = min(n, S_max)
        for c, s, third in ((kc, ks, 1), (vc, vs, 2)):
            wc, wsc = T.kv_quantize(x[b, :n, third].transpose(0, 1))
            assert torch.equal(u8(c[b, :, :n]).cpu(), u8(wc)) and (u8(c)[b, :, n:] == 0x55).all()
            assert torch.equal(s[b, :, :n].cpu().view(torch.int32), wsc.view(torch.int32)) and (s[b, :, n:] == 7).all()


def _logits(model, ids, lens, steps, dtype, window_dev):
    cache = KVCache(model.cfg, len(lens), ids.shape[1], window_dev, dtype)
    ln, rec = torch.tensor(lens, device=window_dev), torch.arange(len(lens), device=window_dev)
    got = [model.prefill(ids, lens, cache)] + [model.decode_step(ids[rec, ln + k], cache) for k in range(steps)]
    return torch.stack(got, 1).float()


@pytest.mark.parametrize("window", [0, 64])
def test_prefill_and_decode_steps_with_an_fp8_cache(window):
    """Bound: 2 x the quantisation floor (fp32 CPU mirrors, FP8 against fp32 cache) + test_attn_decode_gpu.py's floor"""
    cfg = BertConfig(vocab_size=512, hidden=128, layers=2, heads=2, intermediate=512, max_position=256, window=window)
    torch.manual_seed(0)
    fused, ref = CausalLM(cfg).to(dev).eval(), CausalLM(cfg).eval()
    for prm in (p for p in fused.parameters() if p.dim() == 2):
        prm.data = prm.data.bfloat16()
    ref.load_state_dict({k: v.float().cpu() for k, v in fused.state_dict().items()})
    lens, S, steps = [5, 64, 70], 128, 3
    ids = torch.randint(0, 512, (3, S), generator=torch.Generator().manual_seed(24))
    qfloor = torch.sub(*(_logits(ref, ids, lens, 3, dt, "cpu") for dt in (FP8, torch.float32))).abs().max().item()
    ln = torch.tensor(lens, device=dev)
    am = (torch.arange(S, device=dev).unsqueeze(0) < (ln + steps).unsqueeze(1)).long()
    at = (ln - 1).unsqueeze(1) + torch.arange(steps + 1, device=dev)
    ref.to(dev).fused = False
    with torch.no_grad():
        pick = lambda x: x.view(3, S, -1)[torch.arange(3, device=dev).unsqueeze(1), at].float()  # noqa: E731
        floor = (pick(fused.logits(ids.to(dev), am)) - pick(ref.logits(ids.to(dev), am))).abs().max().item()
    got8, got16 = (_logits(fused, ids.to(dev), lens, steps, dt, dev) for dt in (FP8, torch.bfloat16))
    err = (got8 - got16).abs().max().item()
    print("[decode lm fp8] W=%d floor: quantisation %.5f, bf16/fp32 %.5f; measured %.5f" % (window, qfloor, floor, err))
    assert torch.isfinite(got8).all() and qfloor > 0 and err <= 2 * qfloor + floor


def test_refusals():
    z = lambda *s: torch.zeros(*s, device=dev, dtype=torch.bfloat16)  # noqa: E731
    lens0, sc = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, NH, 16, device=dev)
    c8 = z(1, NH, 16, 64).to(FP8)
    with pytest.raises(RuntimeError, match="needs its kscale"):
        lib().attn_decode(z(1, 3 * H), lens0, 0, 4, c8, c8.clone(), 0)
    with pytest.raises(RuntimeError, match="takes no kscale"):
        lib().attn_decode(z(1, 3 * H), lens0, 0, 4, z(1, NH, 16, 64), z(1, NH, 16, 64), 0, sc, sc.clone())
    with pytest.raises(ValueError, match="cache is full"):
        T.attn_decode(z(1, 3 * H), lens0, 16, 16, c8, c8.clone(), 0, sc, sc.clone())
    with pytest.raises(ValueError, match="served by attn_decode only"):
        T.attn_extend(z(1, 3 * H), lens0, 0, 4, c8, c8.clone(), 1)
    cfg = BertConfig(vocab_size=512, hidden=128, layers=1, heads=2, intermediate=512, max_position=128)
    model, ids = CausalLM(cfg).to(dev), torch.zeros(1, 20, dtype=torch.int64, device=dev)
    for call in (lambda c: model.extend(ids, c), lambda c: model.prefill(ids, [20], c, chunk=16)):
        with pytest.raises(ValueError, match="quantised"):
            call(KVCache(cfg, 1, 64, dev, FP8))
