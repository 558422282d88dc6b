"""Incremental decoding (csrc/kernels/attention_decode.hip): attn_decode against the last query row of the plain fp64
causal attention over cat(cache, new token), the fused append, exclusion bit for bit, split invariance, kv_cache_fill
and emb_fwd_at against their indexing expressions, and CausalLM prefill + decode_step against CausalLM.logits on the
grown sequence.  Kernel bounds: the causal forward's (tests/test_attn_causal_gpu.py) -- the same bf16 operands and fp32
softmax.  Measured values: profiles/attn_decode/test_errors.txt."""
import functools

import pytest
import torch

import dtg  # noqa: F401
from dtg.models import BertConfig, CausalLM, KVCache
from dtg.ops import lib, transformer as T

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
NH, H, SENT = 2, 128, 7.0
# one batch per cache size, every edge in it: an empty cache, one key, a chunk less one, exactly a chunk (the owner
# chunk then holds the new token alone) | a chunk and one, two less one, ten whole chunks, the last row of the cache
LENS = {300: [0, 1, 63, 64], 1100: [65, 127, 640, 1099]}


@functools.lru_cache(None)
def _case(S_max):
    """-> rows [B, S_max, 3H] (record b's qkv history; row len_b is the new token), qkv1, lens0, t, filled caches"""
    lens = LENS[S_max]
    B, t = len(lens), min(lens)
    g = torch.Generator(device="cpu").manual_seed(S_max)
    rows = (torch.randn(B, S_max, 3 * H, generator=g) * 1.5).bfloat16().to(dev)
    kc = torch.full((B, NH, S_max, 64), SENT, device=dev, dtype=torch.bfloat16)
    vc = kc.clone()
    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
    T.kv_cache_fill(rows.view(B * S_max, 3 * H), ln, kc, vc, B, S_max, NH)
    qkv1 = torch.stack([rows[b, n] for b, n in enumerate(lens)])
    return rows, qkv1, ln - t, t, kc, vc


@functools.lru_cache(None)
def _reference(S_max, window):
    """fp64 (ctx [B, H], lse [B, NH]) of the new token of each record"""
    rows = _case(S_max)[0]
    ctx, lse = [], []
    for b, n in enumerate(LENS[S_max]):
        seq = rows[b, :n + 1].double()
        ctx.append(T.attention_ref(seq, None, 1, n + 1, NH, causal=True, window=window)[-1])
        lo = max(0, n + 1 - window) if window else 0
        q, k = seq[-1, :H].view(NH, 1, 64), seq[lo:, H:2 * H].view(-1, NH, 64).transpose(0, 1)
        lse.append(torch.logsumexp((q @ k.transpose(1, 2)).squeeze(1) / 8.0, -1))
    return torch.stack(ctx), torch.stack(lse)


def _decode(S_max, window, nsplit, kc=None, vc=None):
    _, qkv1, lens0, t, kc0, vc0 = _case(S_max)
    kc, vc = (kc0.clone(), vc0.clone()) if kc is None else (kc, vc)
    lib().attn_decode_force_splits(nsplit)
    try:
        ctx, lse = T.attn_decode(qkv1, lens0, t, max(LENS[S_max]), kc, vc, window)
    finally:
        lib().attn_decode_force_splits(0)
    return ctx, lse, kc, vc


# window 200 is no multiple of 64; nsplit 0: the launcher's choice, 1: no combine, 5: one chunk per split at S_max = 300
# (splits 2..4 empty for every record) and 4 at 1100 (splits 1..4 empty for len = 65 and 127)
@pytest.mark.parametrize("nsplit", [0, 1, 5])
@pytest.mark.parametrize("window", [0, 64, 200])
@pytest.mark.parametrize("S_max", [300, 1100])
def test_attn_decode_against_fp64_and_append(S_max, window, nsplit):
    rows, qkv1, _, _, kc0, vc0 = _case(S_max)
    ctx, lse, kc, vc = _decode(S_max, window, nsplit)
    ref, ref_lse = _reference(S_max, window)
    e_out = ((ctx.double() - ref).norm() / ref.norm()).item()
    e_lse = (lse.double() - ref_lse).abs().max().item()
    print("[attn decode] S_max=%d window=%d nsplit=%d rel out %.2e, max |dLSE| %.2e" % (S_max, window, nsplit, e_out,
                                                                                       e_lse))
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    assert e_out < 1.5e-2
    assert e_lse <= 2e-2
    for b, n in enumerate(LENS[S_max]):  # rows < len as they were, row len the token's k / v, rows > len the sentinel
        for c, c0, third in ((kc, kc0, 1), (vc, vc0, 2)):
            assert torch.equal(c[b, :, :n], c0[b, :, :n])
            assert torch.equal(c[b, :, n], qkv1[b, third * H:(third + 1) * H].view(NH, 64))
            assert (c[b, :, n + 1:] == SENT).all()


@pytest.mark.parametrize("window,fill", [(64, "random"), (64, "nan"), (0, "nan")])
def test_excluded_rows_never_reach_the_result(window, fill):
    """window 64: record 2 (len 640) sees rows 577 .. 640, so rows < 577 may hold anything; window 0: rows > len of
    every record may.  Bit for bit, and finite: an excluded key is not loaded, not multiplied by zero."""
    S_max = 1100
    ctx, lse, _, _ = _decode(S_max, window, 5)
    kc, vc = _case(S_max)[4].clone(), _case(S_max)[5].clone()
    for c in (kc, vc):
        if window:
            c[2, :, :577] = torch.randn_like(c[2, :, :577]) * 3 if fill == "random" else float("nan")
        else:
            for b, n in enumerate(LENS[S_max]):
                c[b, :, n + 1:] = float("nan")
    ctx2, lse2, _, _ = _decode(S_max, window, 5, kc, vc)
    assert torch.isfinite(ctx2).all() and torch.isfinite(lse2).all()
    assert torch.equal(ctx2, ctx) and torch.equal(lse2, lse)


@pytest.mark.parametrize("window", [0, 200])
def test_split_invariance(window):
    """One split against 5 and 18 (a chunk per split).  The splits change the order of fp32 operations only: the
    running-max rescales, the combine's exp2 weights and its FMAs each cost about an ulp (2^-24) on l and on acc
    relative to sum(p |v|) <= l max|v|, at most ~2 per chunk and split, 18 + 18 here: 64 ulp is a safe count.  So
    |d ctx| <= 64 * 2^-24 * max|v| before the one bf16 rounding, which can then land on the neighbouring bf16 value:
    2^-7 |ctx| more.  lse = M ln 2 + log(l) with the same M: 64 ulp on l move it by 64 * 2^-24 = 4e-6, plus an ulp of
    the sum at |lse| < 16 (1e-6): 1e-5."""
    S_max = 1100
    vmax = _case(S_max)[0][:, :, 2 * H:].abs().max().item()
    ctx, lse, _, _ = _decode(S_max, window, 1)
    for nsplit in (5, 18):
        ctx2, lse2, _, _ = _decode(S_max, window, nsplit)
        d = (ctx2.float() - ctx.float()).abs()
        assert (d <= 2.0 ** -7 * ctx.float().abs() + 64 * 2.0 ** -24 * vmax).all(), d.max().item()
        assert (lse2 - lse).abs().max().item() <= 1e-5


def test_kv_cache_fill_is_the_indexing_expression():
    B, S0, S_max = 4, 70, 100
    lens = [0, S0, 90, 33]  # nothing, everything, clamped to S0, a part
    qkv = torch.randn(B * S0, 3 * H, device=dev).bfloat16()
    kc = torch.full((B, NH, S_max, 64), SENT, device=dev, dtype=torch.bfloat16)
    vc = kc.clone()
    T.kv_cache_fill(qkv, torch.tensor(lens, dtype=torch.int32, device=dev), kc, vc, B, S0, NH)
    x = qkv.view(B, S0, 3, NH, 64)
    for b, n in enumerate(lens):
        n = min(n, S0)
        for c, third in ((kc, 1), (vc, 2)):
            assert torch.equal(c[b, :, :n], x[b, :n, third].transpose(0, 1)) and (c[b, :, n:] == SENT).all()


def test_emb_fwd_at_is_the_gather():
    """Bit for bit: the kernel adds word + (pos + type) in fp32 and rounds once, and so does the expression below
    (fp32 addition is commutative, and the grouping is the same)."""
    B, V, P, Hh, t = 5, 50, 40, 640, 3  # 80 16-byte column chunks: a lane's second trip; two workgroups
    word, pos, typ = (torch.randn(n, Hh, device=dev).bfloat16() for n in (V, P, 2))
    ids = torch.tensor([0, 49, 7, 7, 20], device=dev)
    lens0 = torch.tensor([0, 36, 5, 6, 17], dtype=torch.int32, device=dev)
    want = (word.float()[ids] + (pos.float()[(lens0 + t).long()] + typ.float()[0])).bfloat16()
    assert torch.equal(T.emb_fwd_at(ids, lens0, t, word, pos, typ), want)


@pytest.mark.parametrize("window", [0, 64])
def test_prefill_and_decode_steps_match_the_full_forward(window):
    """Logits of prefill + 3 decode steps against CausalLM.logits (bf16 fused path) on the grown sequence at the same
    positions.  Noise floor: the largest logit difference between that reference and its own fp32 path at those
    positions.  The decode path and the reference are two bf16 evaluations of the same fp32 function, each within
    about a floor of it, so they may lie 2 floors apart: the bound is 2 x floor."""
    cfg = BertConfig(vocab_size=512, hidden=128, layers=2, heads=2, intermediate=512, max_position=256, window=window)
    torch.manual_seed(0)
    fused = CausalLM(cfg).to(dev).eval()
    for prm in fused.parameters():
        if prm.dim() == 2:
            prm.data = prm.data.bfloat16()
    ref = CausalLM(cfg).to(dev).eval()
    ref.load_state_dict({k: v.float() for k, v in fused.state_dict().items()})
    ref.fused = False
    lens, S, steps = [5, 64, 70], 128, 3
    # prompt seed 24: the fp32 model's least top-2 gap over the 12 positions is 0.046 on the CPU, with and without
    # the window (the best of seeds 0 .. 299; seed 0 leaves 0.005)
    ids = torch.randint(0, 512, (3, S), generator=torch.Generator().manual_seed(24)).to(dev)
    rec = torch.arange(3, device=dev)
    ln = torch.tensor(lens, device=dev)
    am = (torch.arange(S, device=dev).unsqueeze(0) < (ln + steps).unsqueeze(1)).long()
    at = (ln - 1).unsqueeze(1) + torch.arange(steps + 1, device=dev)  # [3, 4] positions
    with torch.no_grad():
        full = fused.logits(ids, am).view(3, S, -1)[rec.unsqueeze(1), at].float()
        full32 = ref.logits(ids, am).view(3, S, -1)[rec.unsqueeze(1), at]
    cache = KVCache(cfg, 3, S, dev)
    got = [fused.prefill(ids, lens, cache)] + [fused.decode_step(ids[rec, ln + k], cache) for k in range(steps)]
    got = torch.stack(got, 1).float()
    floor = (full - full32).abs().max().item()
    err = (got - full).abs().max().item()
    top2 = full.topk(2, -1).values
    gap = top2[..., 0] - top2[..., 1]
    print("[decode lm] window=%d noise floor %.5f, decode vs full forward %.5f (bound %.5f), least top-2 gap %.5f" % (
        window, floor, err, 2 * floor, gap.min().item()))
    assert cache.t == steps and torch.isfinite(got).all()
    assert err <= 2 * floor
    assert (gap > floor).all()  # no position is skipped: the seed leaves a gap above the floor everywhere
    assert torch.equal(got.argmax(-1), full.argmax(-1))


def test_refusals():
    z = lambda *s: torch.zeros(*s, device=dev, dtype=torch.bfloat16)  # noqa: E731
    lens0 = torch.zeros(1, dtype=torch.int32, device=dev)
    assert T.attn_decode_supported(64, 300) and lib().attn_decode_supported(64, 300)
    assert not T.attn_decode_supported(32, 300) and not lib().attn_decode_supported(32, 300)
    with pytest.raises(ValueError, match="head dim 64"):
        T.attn_decode(z(1, 3 * 2 * 32), lens0, 0, 4, z(1, 2, 16, 32), z(1, 2, 16, 32))
    with pytest.raises(RuntimeError, match="head dim 64"):
        lib().kv_cache_fill(z(8, 3 * 2 * 32), lens0, z(1, 2, 16, 32), z(1, 2, 16, 32), 8)
    with pytest.raises(ValueError, match="cache is full"):
        T.attn_decode(z(1, 3 * H), lens0, 16, 16, z(1, NH, 16, 64), z(1, NH, 16, 64))
    with pytest.raises(RuntimeError, match="cache is full"):
        lib().attn_decode(z(1, 3 * H), lens0, 16, 16, z(1, NH, 16, 64), z(1, NH, 16, 64), 0)
    model = CausalLM(BertConfig(vocab_size=512, hidden=128, layers=1, heads=2, intermediate=512, max_position=128))
    model = model.to(dev)
    with pytest.raises(ValueError, match="max_position"):
        model.generate(torch.zeros(1, 100, dtype=torch.int64, device=dev), [100], 29)
