"""Multi-token KV-cache attention (csrc/kernels/attention_extend.hip): attn_extend against rows len .. len + T - 1 of
the plain fp64 causal attention over cat(cache, new tokens), the fused append, ragged n_new, exclusion bit for bit,
T = 1 against attn_decode, split invariance, emb_fwd_span against emb_fwd_at, and CausalLM prefill + extend +
decode_step and the chunked prefill against CausalLM.logits on the grown sequence.  Kernel bounds: the causal forward's
and attn_decode's (the same bf16 operands and fp32 softmax).  Measured values: profiles/attn_extend/test_errors.txt."""
import functools

import pytest
import torch

import dtg  # noqa: F401
from dtg.models import BertConfig, CausalLM, KVCache
from dtg.ops import lib, transformer as T

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
NH, H, SENT, TMAX = 2, 128, 7.0, 64
# an empty cache, one key, a chunk less one, exactly a chunk | a chunk and one, two less one, ten whole chunks
LENS = {300: [0, 1, 63, 64], 1100: [65, 127, 640]}


@functools.lru_cache(None)
def _case(S_max):
    """-> rows [B, S_max, 3H] (record b's qkv history; rows len_b .. len_b + 63 are its new tokens), lens0, t, caches"""
    lens = LENS[S_max]
    B, t = len(lens), min(lens)
    g = torch.Generator(device="cpu").manual_seed(S_max)
    rows = (torch.randn(B, S_max, 3 * H, generator=g) * 1.5).bfloat16().to(dev)
    kc = torch.full((B, NH, S_max, 64), SENT, device=dev, dtype=torch.bfloat16)
    vc = kc.clone()
    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
    T.kv_cache_fill(rows.view(B * S_max, 3 * H), ln, kc, vc, B, S_max, NH)
    return rows, ln - t, t, kc, vc


@functools.lru_cache(None)
def _reference(S_max, window):
    """fp64 (ctx [B, 64, H], lse [B, NH, 64]) of the 64 new tokens of each record; causal, so a shorter T is a prefix"""
    rows = _case(S_max)[0]
    ctx, lse = [], []
    for b, n in enumerate(LENS[S_max]):
        seq = rows[b, :n + TMAX].double()
        ctx.append(T.attention_ref(seq, None, 1, n + TMAX, NH, causal=True, window=window)[n:])
        q, k = (seq[:, i * H:(i + 1) * H].view(-1, NH, 64).transpose(0, 1) for i in (0, 1))
        sc = (q @ k.transpose(1, 2) / 8.0).masked_fill(T._invisible(n + TMAX, window, dev), float("-inf"))
        lse.append(torch.logsumexp(sc, -1)[:, n:])
    return torch.stack(ctx), torch.stack(lse)


def _new(S_max, Tn):
    rows = _case(S_max)[0]
    return torch.stack([rows[b, n:n + Tn] for b, n in enumerate(LENS[S_max])]).reshape(-1, 3 * H)


def _extend(S_max, Tn, window, nsplit, kc=None, vc=None, qkvT=None, n_new=None):
    _, lens0, t, kc0, vc0 = _case(S_max)
    kc, vc = (kc0.clone(), vc0.clone()) if kc is None else (kc, vc)
    lib().attn_decode_force_splits(nsplit)
    try:
        ctx, lse = T.attn_extend(_new(S_max, Tn) if qkvT is None else qkvT, lens0, t, max(LENS[S_max]), kc, vc, Tn,
                                 window, n_new)
    finally:
        lib().attn_decode_force_splits(0)
    return ctx.view(-1, Tn, H), lse, kc, vc


def _check_cache(S_max, Tn, ns, kc, vc):
    """rows < len as they were, rows len .. len + n - 1 the tokens' k / v, rows beyond the sentinel"""
    kc0, vc0, new = _case(S_max)[3], _case(S_max)[4], _new(S_max, Tn).view(-1, Tn, 3, NH, 64)
    for b, (n0, n) in enumerate(zip(LENS[S_max], ns)):
        for c, c0, third in ((kc, kc0, 1), (vc, vc0, 2)):
            assert torch.equal(c[b, :, :n0], c0[b, :, :n0]) and (c[b, :, n0 + n:] == SENT).all()
            assert torch.equal(c[b, :, n0:n0 + n], new[b, :n, third].transpose(0, 1))


# window 8 < T cuts inside the new block, 200 is no multiple of 16; nsplit 0: the launcher's choice, 1: no combine,
# 5: empty splits (one chunk per split at S_max = 300, splits 1..4 empty for len = 65 and 127 at 1100)
@pytest.mark.parametrize("nsplit", [0, 1, 5])
@pytest.mark.parametrize("window", [0, 8, 64, 200])
@pytest.mark.parametrize("Tn", [1, 5, 16, 17, 64])
@pytest.mark.parametrize("S_max", [300, 1100])
def test_attn_extend_against_fp64_and_append(S_max, Tn, window, nsplit):
    ctx, lse, kc, vc = _extend(S_max, Tn, window, nsplit)
    ref, ref_lse = _reference(S_max, window)
    ref, ref_lse = ref[:, :Tn], ref_lse[:, :, :Tn]
    e_out = ((ctx.double() - ref).norm() / ref.norm()).item()
    e_lse = (lse.double() - ref_lse).abs().max().item()
    print("[attn extend] S_max=%d T=%d window=%d nsplit=%d rel out %.2e, max |dLSE| %.2e" % (S_max, Tn, window, nsplit,
                                                                                           e_out, e_lse))
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    assert e_out < 1.5e-2
    assert e_lse <= 2e-2
    _check_cache(S_max, Tn, [Tn] * len(LENS[S_max]), kc, vc)


RAGGED = [17, 0, 3]  # S_max = 1100, T = 17: every row, none, a part of the first tile


@pytest.mark.parametrize("fill", ["random", "nan"])
def test_ragged_append_and_excluded_rows_never_reach_the_result(fill):
    """W = 64, T = 17 (len = 640 among the records), ragged n_new: rows >= n_new[b] are exactly zero and not appended.
    Then cache rows below len + 1 - W (what query 0 sees), cache rows at and beyond len, and qkvT rows at and beyond
    n_new[b] hold other values / NaN: bit for bit the same, and finite."""
    S_max, Tn, W = 1100, 17, 64
    n_new = torch.tensor(RAGGED, dtype=torch.int32, device=dev)
    ctx, lse, kc, vc = _extend(S_max, Tn, W, 5, n_new=n_new)
    ref, ref_lse = _reference(S_max, W)
    _check_cache(S_max, Tn, RAGGED, kc, vc)
    for b, n in enumerate(RAGGED):
        assert (ctx[b, n:] == 0).all() and (lse[b, :, n:] == 0).all()
        if n:
            assert ((ctx[b, :n].double() - ref[b, :n]).norm() / ref[b, :n].norm()).item() < 1.5e-2
            assert (lse[b, :, :n].double() - ref_lse[b, :, :n]).abs().max().item() <= 2e-2
    kc, vc, qkvT = _case(S_max)[3].clone(), _case(S_max)[4].clone(), _new(S_max, Tn).clone().view(-1, Tn, 3 * H)
    junk = (lambda x: torch.randn_like(x) * 3) if fill == "random" else (lambda x: torch.full_like(x, float("nan")))
    for b, (n0, n) in enumerate(zip(LENS[S_max], RAGGED)):
        qkvT[b, n:] = junk(qkvT[b, n:])
        for c in (kc, vc):
            c[b, :, :n0 + 1 - W] = junk(c[b, :, :n0 + 1 - W])
            c[b, :, n0:] = junk(c[b, :, n0:])
    ctx2, lse2, _, _ = _extend(S_max, Tn, W, 5, kc, vc, qkvT.view(-1, 3 * H), n_new)
    assert torch.isfinite(ctx2).all() and torch.isfinite(lse2).all()
    assert torch.equal(ctx2, ctx) and torch.equal(lse2, lse)


@pytest.mark.parametrize("window", [0, 200])
@pytest.mark.parametrize("S_max", [300, 1100])
def test_one_token_is_attn_decode(S_max, window):
    """Two kernels, each within 1.5e-2 / 2e-2 of fp64: within 3e-2 / 4e-2 of each other."""
    ctx, lse, kc, vc = _extend(S_max, 1, window, 0)
    _, lens0, t, kc0, vc0 = _case(S_max)
    kd, vd = kc0.clone(), vc0.clone()
    ctx_d, lse_d = T.attn_decode(_new(S_max, 1), lens0, t, max(LENS[S_max]), kd, vd, window)
    ref = _reference(S_max, window)[0][:, :1]
    assert ((ctx[:, 0].double() - ctx_d.double()).norm() / ref.norm()).item() < 3e-2
    assert (lse[:, :, 0] - lse_d).abs().max().item() <= 4e-2
    assert torch.equal(kc, kd) and torch.equal(vc, vd)


@pytest.mark.parametrize("window", [0, 200])
def test_split_invariance(window):
    """One split against 5.  The splits change which chunks a wave folds together, so the running max a chunk's P is
    taken against: P = exp2(s - max) is rounded to bf16 for the MFMA (half an ulp, 2^-9 relative, per element), so
    acc / l moves by at most 2 * 2^-9 * sum(p |v|) / l <= 2^-8 max|v|; the fp32 rescales, the combine's exp2 weights
    and FMAs add the decode test's 64 ulp of 2^-24 max|v|.  The one bf16 rounding of ctx can then land on the
    neighbouring value: 2^-7 |ctx| more.  l is summed from the unrounded fp32 P: lse moves by 64 * 2^-24 plus an ulp
    of the sum at |lse| < 16, 1e-5, as in the decode test."""
    S_max, Tn = 1100, 17
    vmax = _case(S_max)[0][:, :, 2 * H:].abs().max().item()
    ctx, lse, _, _ = _extend(S_max, Tn, window, 1)
    ctx2, lse2, _, _ = _extend(S_max, Tn, window, 5)
    d = (ctx2.float() - ctx.float()).abs()
    assert (d <= 2.0 ** -7 * ctx.float().abs() + (2.0 ** -8 + 64 * 2.0 ** -24) * vmax).all(), d.max().item()
    assert (lse2 - lse).abs().max().item() <= 1e-5


def test_emb_fwd_span_is_emb_fwd_at_per_column():
    B, V, P, Hh, t, Tn = 5, 50, 40, 640, 3, 3  # 15 rows: four workgroups, the last one partial
    word, pos, typ = (torch.randn(n, Hh, device=dev).bfloat16() for n in (V, P, 2))
    ids = torch.randint(0, V, (B, Tn), device=dev)
    lens0 = torch.tensor([0, 34, 5, 6, 17], dtype=torch.int32, device=dev)
    got = T.emb_fwd_span(ids, lens0, t, word, pos, typ).view(B, Tn, Hh)
    for i in range(Tn):
        assert torch.equal(got[:, i], T.emb_fwd_at(ids[:, i].contiguous(), lens0, t + i, word, pos, typ))


@pytest.mark.parametrize("window", [0, 64])
def test_prefill_extend_decode_and_chunked_prefill_match_the_full_forward(window):
    """Logits of prefill, extend (T = 5) and one decode step against CausalLM.logits (bf16 fused path) on the grown
    sequence at the same positions, and prefill(chunk = 64 / 16) against prefill(chunk = 0).  Noise floor: the largest
    logit difference between that reference and its own fp32 path at those positions; two bf16 evaluations of the same
    fp32 function may lie 2 floors apart (the decode test's rule)."""
    cfg = BertConfig(vocab_size=512, hidden=128, layers=2, heads=2, intermediate=512, max_position=256, window=window)
    torch.manual_seed(0)
    fused = CausalLM(cfg).to(dev).eval()
    for prm in fused.parameters():
        if prm.dim() == 2:
            prm.data = prm.data.bfloat16()
    ref = CausalLM(cfg).to(dev).eval()
    ref.load_state_dict({k: v.float() for k, v in fused.state_dict().items()})
    ref.fused = False
    lens, S, Tn = [5, 64, 70], 128, 5
    # prompt seed 101: the fp32 model's least top-2 gap over the 21 positions is 0.025 on the CPU, with and without
    # the window (the best of seeds 0 .. 419)
    ids = torch.randint(0, 512, (3, S), generator=torch.Generator().manual_seed(101)).to(dev)
    rec = torch.arange(3, device=dev)
    ln = torch.tensor(lens, device=dev)
    am = (torch.arange(S, device=dev).unsqueeze(0) < (ln + Tn + 1).unsqueeze(1)).long()
    at = (ln - 1).unsqueeze(1) + torch.arange(Tn + 2, device=dev)  # [3, 7] positions
    with torch.no_grad():
        full = fused.logits(ids, am).view(3, S, -1)[rec.unsqueeze(1), at].float()
        full32 = ref.logits(ids, am).view(3, S, -1)[rec.unsqueeze(1), at]
    cache = KVCache(cfg, 3, S, dev)
    first = fused.prefill(ids, lens, cache)
    new = ids[rec.unsqueeze(1), ln.unsqueeze(1) + torch.arange(Tn, device=dev)]
    got = torch.cat([first.unsqueeze(1), fused.extend(new, cache),
                     fused.decode_step(ids[rec, ln + Tn], cache).unsqueeze(1)], 1).float()
    chunked = [fused.prefill(ids, lens, KVCache(cfg, 3, S, dev), chunk=c).float() for c in (64, 16)]
    floor = (full - full32).abs().max().item()
    err = (got - full).abs().max().item()
    err_c = max((x - first.float()).abs().max().item() for x in chunked)
    top2 = full.topk(2, -1).values
    gap = top2[..., 0] - top2[..., 1]
    print("[extend lm] window=%d noise floor %.5f, prefill+extend+decode vs full %.5f, chunked vs one-shot prefill %.5f "
          "(bound %.5f), least top-2 gap %.5f" % (window, floor, err, err_c, 2 * floor, gap.min().item()))
    assert cache.t == Tn + 1 and torch.isfinite(got).all()
    assert err <= 2 * floor and err_c <= 2 * floor
    assert (gap > floor).all()  # no position is skipped: the seed leaves a gap above the floor everywhere
    assert torch.equal(got.argmax(-1), full.argmax(-1))
    assert all(torch.equal(x.argmax(-1), full[:, 0].argmax(-1)) for x in chunked)


def test_refusals():
    z = lambda *s: torch.zeros(*s, device=dev, dtype=torch.bfloat16)  # noqa: E731
    lens0 = torch.zeros(1, dtype=torch.int32, device=dev)
    assert T.attn_extend_supported(64, 300, 64) and lib().attn_extend_supported(64, 300, 1)
    for dh, Tn in ((32, 4), (64, 0), (64, 65)):
        assert not T.attn_extend_supported(dh, 300, Tn) and not lib().attn_extend_supported(dh, 300, Tn)
    for Tn in (0, 65):
        with pytest.raises(ValueError, match="T <= 64"):
            T.attn_extend(z(max(Tn, 1), 3 * H), lens0, 0, 0, z(1, NH, 128, 64), z(1, NH, 128, 64), Tn)
    with pytest.raises(RuntimeError, match="T <= 64"):
        lib().attn_extend(z(65, 3 * H), lens0, 0, 0, z(1, NH, 128, 64), z(1, NH, 128, 64), 65, 0, None)
    with pytest.raises(ValueError, match="cache is full"):
        T.attn_extend(z(4, 3 * H), lens0, 13, 13, z(1, NH, 16, 64), z(1, NH, 16, 64), 4)
    with pytest.raises(RuntimeError, match="cache is full"):
        lib().attn_extend(z(4, 3 * H), lens0, 13, 13, z(1, NH, 16, 64), z(1, NH, 16, 64), 4, 0, None)
    with pytest.raises(ValueError, match="head dim 64"):
        T.attn_extend(z(4, 3 * 2 * 32), lens0, 0, 4, z(1, 2, 16, 32), z(1, 2, 16, 32), 4)
