"""Transformer ops on dtg's HIP kernels (csrc/kernels/transformer.hip) plus their PyTorch mirrors.

The mirrors define the semantics the kernels must reproduce (tests compare the two):

* ``dropout_keep``   -- the counter-hash dropout mask: element ``i`` of a tensor is kept iff
  ``fmix32(i * 0x9E3779B1 + seed) >= floor(p * 2**32)``.  The kernels regenerate it in backward,
  so no mask tensor is ever stored.
* ``attn_dropout_keep`` -- the attention-probability dropout: one hash per PAIR of adjacent elements, its
  low / high 16 bits against ``floor(p * 2**16)`` (the fused attention kernels hold 4 consecutive keys per lane).
* ``layer_norm_ref`` -- ``y = dropout_out(LN(res + dropout_in(h)))``.
* ``attention_ref``  -- softmax(QK^T/sqrt(d) + mask) -> attention dropout -> @V per head; ``causal=True`` puts
  ``-inf`` above the diagonal first (a key > query is out of the softmax; the dropout draw keeps the [S, S] layout),
  and ``window=W`` below the last W keys as well.

Not in the reference (TF1 toy models); this is the BERT-base slice of BASELINE.json
config 5.
"""
import math

import torch

from ._native import lib

_M32 = 0xFFFFFFFF


def _fmix32(h):
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def drop_threshold(p):
    if p <= 0:
        return 0
    return min(int(p * 4294967296.0), _M32)


def dropout_keep(seed, numel, p, device=None):
    """Boolean keep-mask of ``numel`` elements (flat index order), identical to the kernels'."""
    th = drop_threshold(p)
    if th == 0:
        return torch.ones(numel, dtype=torch.bool, device=device)
    idx = torch.arange(numel, dtype=torch.int64, device=device)
    h = _fmix32(((idx * 0x9E3779B1) + (seed & _M32)) & _M32)
    return h >= th


def attn_drop_threshold(p):
    """16-bit threshold of the attention-probability dropout (0 = off)."""
    if p <= 0:
        return 0
    t = int(p * 65536.0)
    return 0xFFFF if p * 65536.0 >= 65535.0 else max(t, 1)


def attn_dropout_keep(seed, numel, p, device=None):
    """Keep-mask of the attention-probability dropout, identical to attention.hip ``keep_attn`` and
    transformer.hip ``attn_softmax_fwd``: one hash per pair of adjacent elements, element ``i`` kept iff the
    low (even ``i``) / high (odd ``i``) 16 bits of ``fmix32((i >> 1) * 0x9E3779B1 + seed)`` are >= floor(p * 2**16)."""
    th = attn_drop_threshold(p)
    if th == 0:
        return torch.ones(numel, dtype=torch.bool, device=device)
    idx = torch.arange(numel, dtype=torch.int64, device=device)
    h = _fmix32((((idx >> 1) * 0x9E3779B1) + (seed & _M32)) & _M32)
    half = torch.where((idx & 1) == 1, h >> 16, h & 0xFFFF)
    return half >= th


def attn_dropout_ref(x, p, seed):
    if p <= 0:
        return x
    keep = attn_dropout_keep(seed, x.numel(), p, x.device).view(x.shape)
    return torch.where(keep, x / (1.0 - p), torch.zeros((), dtype=x.dtype, device=x.device))


def dropout_ref(x, p, seed):
    if p <= 0:
        return x
    keep = dropout_keep(seed, x.numel(), p, x.device).view(x.shape)
    return torch.where(keep, x / (1.0 - p), torch.zeros((), dtype=x.dtype, device=x.device))


def layer_norm_ref(h, res, gamma, beta, eps, p_in=0.0, seed_in=0, p_out=0.0, seed_out=0):
    s = dropout_ref(h, p_in, seed_in)
    if res is not None:
        s = s + res
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    y = (s - mean) * torch.rsqrt(var + eps) * gamma + beta
    return dropout_ref(y, p_out, seed_out)


def _invisible(S, window, device):
    """[S, S] bool: key > q, or (window > 0) key <= q - window"""
    inv = torch.ones(S, S, dtype=torch.bool, device=device).triu(1)
    if window > 0:
        inv |= torch.ones(S, S, dtype=torch.bool, device=device).tril(-window)
    return inv


def attention_ref(qkv, mask_add, B, S, nh, p=0.0, seed=0, causal=False, window=0):
    """qkv [B*S, 3H] -> context [B*S, H] (the fused layer's attention, in plain torch).  causal: query q sees keys
    <= q only (-inf above the diagonal before the softmax); the dropout mask is still drawn over the full [S, S].
    window > 0 (causal only): -inf where q - key >= window too, so q sees its last ``window`` keys, itself included."""
    if window and not causal:
        raise ValueError("window = %d needs causal=True" % window)
    H = qkv.shape[1] // 3
    dh = H // nh
    q, k, v = qkv.view(B, S, 3, nh, dh).permute(2, 0, 3, 1, 4)  # [B, nh, S, dh] each
    sc = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    if mask_add is not None:
        sc = sc + mask_add.view(B, 1, 1, S).to(sc.dtype)
    if causal:
        sc = sc.masked_fill(_invisible(S, window, sc.device), float("-inf"))
    pr = torch.softmax(sc, dim=-1)
    pr = attn_dropout_ref(pr.reshape(-1, S), p, seed).view(B, nh, S, S)
    return (pr @ v).permute(0, 2, 1, 3).reshape(B * S, H)


def mask_additive(attention_mask):
    """[B, S] 1/0 attention mask -> fp32 additive key mask (0 / -10000, as in BERT)."""
    if attention_mask.is_cuda and attention_mask.dtype in (torch.int64, torch.float32):
        return lib().mask_additive(attention_mask.contiguous())  # one dtg kernel
    return (1.0 - attention_mask.float()) * -10000.0


# ---- thin wrappers over the native ops ------------------------------------------------------
def gemm_batched(a, a_kc, b, b_kc, c, M, N, K, lda, ldb, ldc, nb, nh, sa, sb, sc, alpha=1.0, beta=0.0):
    """Strided two-level batched GEMM; sa/sb/sc = (batch stride, head stride) in elements."""
    lib().gemm_strided_batched(a, a_kc, b, b_kc, c, M, N, K, lda, ldb, ldc, nb, nh, sa[0], sa[1], sb[0], sb[1],
                               sc[0], sc[1], alpha, beta)
    return c


def attention_fwd(qkv, mask_add, B, S, nh, p, seed):
    """Fused-path attention forward.  Returns (ctx [T,H], P, Pd)."""
    L = lib()
    T, H3 = qkv.shape
    H = H3 // 3
    dh = H // nh
    scores = torch.empty(B * nh * S, S, device=qkv.device, dtype=torch.float32)
    # scores[b,h] = Q_bh K_bh^T / sqrt(dh):   A = Q (KC, ld 3H)   B = K (KC, ld 3H)
    gemm_batched(qkv, True, qkv[:, H:], True, scores, S, S, dh, H3, H3, S, B, nh, (S * H3, dh), (S * H3, dh),
                 (nh * S * S, S * S), alpha=1.0 / math.sqrt(dh))
    P, Pd = L.attn_softmax_fwd(scores, mask_add, nh * S, p, seed)
    ctx = torch.empty(T, H, device=qkv.device, dtype=qkv.dtype)
    # ctx[b, :, h] = Pd_bh V_bh:   A = Pd (KC, ld S)   B = V (MC: [K=keys, N=dh], ld 3H)
    gemm_batched(Pd, True, qkv[:, 2 * H:], False, ctx, S, dh, S, S, H3, H, B, nh, (nh * S * S, S * S),
                 (S * H3, dh), (S * H, dh))
    return ctx, P, Pd


def attention_bwd(dctx, qkv, P, Pd, B, S, nh, dqkv):
    """Fused-path attention backward: fills dqkv [T, 3H] from dctx [T, H]."""
    L = lib()
    T, H3 = qkv.shape
    H = H3 // 3
    dh = H // nh
    dPd = torch.empty(B * nh * S, S, device=qkv.device, dtype=torch.float32)
    # dPd = dctx_bh V_bh^T:   A = dctx (KC, ld H)   B = V (KC, ld 3H)
    gemm_batched(dctx, True, qkv[:, 2 * H:], True, dPd, S, S, dh, H, H3, S, B, nh, (S * H, dh), (S * H3, dh),
                 (nh * S * S, S * S))
    # dV = Pd^T dctx:   A = Pd stored [q][k] -> MC (ld S)   B = dctx stored [q][d] -> MC (ld H)
    gemm_batched(Pd, False, dctx, False, dqkv[:, 2 * H:], S, dh, S, S, H, H3, B, nh, (nh * S * S, S * S),
                 (S * H, dh), (S * H3, dh))
    dS = L.attn_softmax_bwd(P, Pd, dPd, 1.0 / math.sqrt(dh))
    # dQ = dS K:   A = dS (KC, ld S)   B = K stored [k][d] -> MC (ld 3H)
    gemm_batched(dS, True, qkv[:, H:], False, dqkv, S, dh, S, S, H3, H3, B, nh, (nh * S * S, S * S), (S * H3, dh),
                 (S * H3, dh))
    # dK = dS^T Q:  A = dS stored [q][k] -> MC (ld S)   B = Q stored [q][d] -> MC (ld 3H)
    gemm_batched(dS, False, qkv, False, dqkv[:, H:], S, dh, S, S, H3, H3, B, nh, (nh * S * S, S * S), (S * H3, dh),
                 (S * H3, dh))
    return dqkv


# ---- causal fused attention (csrc/kernels/attention_causal.hip) ------------------------------------------
def _native_bf16(t):
    return t.is_cuda and t.dtype == torch.bfloat16


def _causal_scores(qkv, mask_add, B, S, nh, window=0):
    dh = qkv.shape[1] // 3 // nh
    q, k, _ = qkv.view(B, S, 3, nh, dh).permute(2, 0, 3, 1, 4)
    sc = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    if mask_add is not None:
        sc = sc + mask_add.view(B, 1, 1, S).to(sc.dtype)
    return sc.masked_fill(_invisible(S, window, sc.device), float("-inf"))


def attn_causal_fwd(qkv, mask_add, B, S, nh, p=0.0, seed=0):
    """qkv [B*S, 3 * nh * 64] -> (ctx [B*S, nh * 64], lse fp32 [B * nh * S]) with a lower-triangular mask on top of
    the additive key mask: the HIP kernels on GPU bf16 tensors (64 <= S <= attn_stream_max_s, S % 64 == 0; other
    shapes are refused), the mirror (``attention_ref(causal=True)`` and the log-sum-exp of its scores) otherwise."""
    if _native_bf16(qkv):
        return tuple(lib().attn_causal_fwd(qkv, mask_add, B, S, nh, p, seed))
    lse = torch.logsumexp(_causal_scores(qkv, mask_add, B, S, nh).float(), -1).reshape(-1)
    return attention_ref(qkv, mask_add, B, S, nh, p, seed, causal=True), lse


def attn_causal_bwd(qkv, out, dout, lse, mask_add, B, S, nh, p=0.0, seed=0, dbias=None):
    """-> dqkv [B*S, 3 * nh * 64]; dbias (optional fp32 [3 * nh * 64]): the column sums of dqkv are ADDED into it.
    The HIP dQ + dKV launches on GPU bf16 tensors, autograd through the mirror otherwise."""
    if _native_bf16(qkv):
        return lib().attn_causal_bwd(qkv, out, dout, lse, mask_add, B, S, nh, p, seed, dbias)
    with torch.enable_grad():
        x = qkv.detach().requires_grad_()
        attention_ref(x, mask_add, B, S, nh, p, seed, causal=True).backward(dout.to(qkv.dtype))
    if dbias is not None:
        dbias += x.grad.sum(0).to(dbias.dtype)
    return x.grad


# ---- sliding-window causal fused attention (csrc/kernels/attention_window.hip) ---------------------------
def attn_window_fwd(qkv, mask_add, B, S, nh, window, p=0.0, seed=0):
    """``attn_causal_fwd`` with a window: query q sees keys q - window < key <= q.  The HIP kernels on GPU bf16
    tensors (``attn_causal_fwd``'s shapes, window % 64 == 0 and window >= 64; anything else is refused; window >= S
    is ``attn_causal_fwd`` itself), the mirror (``attention_ref(causal=True, window=window)``, any window > 0)
    otherwise."""
    if _native_bf16(qkv):
        return tuple(lib().attn_window_fwd(qkv, mask_add, B, S, nh, window, p, seed))
    if window <= 0:
        raise ValueError("window must be positive (got %d)" % window)
    lse = torch.logsumexp(_causal_scores(qkv, mask_add, B, S, nh, window).float(), -1).reshape(-1)
    return attention_ref(qkv, mask_add, B, S, nh, p, seed, causal=True, window=window), lse


def attn_window_bwd(qkv, out, dout, lse, mask_add, B, S, nh, window, p=0.0, seed=0, dbias=None):
    """-> dqkv [B*S, 3 * nh * 64]; dbias (optional fp32 [3 * nh * 64]): the column sums of dqkv are ADDED into it.
    The HIP dQ + dKV launches on GPU bf16 tensors, autograd through the mirror otherwise."""
    if _native_bf16(qkv):
        return lib().attn_window_bwd(qkv, out, dout, lse, mask_add, B, S, nh, window, p, seed, dbias)
    if window <= 0:
        raise ValueError("window must be positive (got %d)" % window)
    with torch.enable_grad():
        x = qkv.detach().requires_grad_()
        attention_ref(x, mask_add, B, S, nh, p, seed, causal=True, window=window).backward(dout.to(qkv.dtype))
    if dbias is not None:
        dbias += x.grad.sum(0).to(dbias.dtype)
    return x.grad


# ---- incremental decoding against a KV cache (csrc/kernels/attention_decode.hip) -------------------------
def attn_decode_supported(dh, S_max):
    """What the decode kernels take: head dim 64 and 1 <= S_max <= 2**30; nothing else is refused."""
    return dh == 64 and 1 <= S_max <= (1 << 30)


FP8 = torch.float8_e4m3fn  # the quantised cache's codes (csrc/kernels/attention_decode_fp8.hip)


def kv_quantize(x):
    """Rows ``x`` [..., dh] -> (codes float8_e4m3fn [..., dh], scale fp32 [...]): ``scale = amax|x| / 448`` (1 for a
    zero row) and ``code = e4m3_rne(x / scale)``, both in fp32 -- the kernels' quantiser bit for bit.  The divisors are
    tensors: torch turns a division by a Python scalar on the GPU into a multiplication by its reciprocal."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / torch.full_like(amax, 448.0))
    return (xf / scale.unsqueeze(-1)).to(FP8), scale


def kv_dequantize(codes, scale):
    """-> fp32 ``code * scale``, what ``attn_decode`` reads of a quantised row"""
    return codes.float() * scale.unsqueeze(-1)


def _quantised(fn, kcache, kscale, vscale):
    """Is the cache FP8?  It then needs both scale tensors, and any other cache takes none."""
    fp8 = kcache.dtype == FP8
    if fp8 != (kscale is not None) or fp8 != (vscale is not None):
        raise ValueError("%s: %s" % (fn, "an FP8 cache needs its kscale / vscale tensors (fp32 [B, nh, S_max])" if fp8
                                     else "a %s cache takes no kscale / vscale" % kcache.dtype))
    return fp8


def kv_cache_fill(qkv, lens0, kcache, vcache, B, S0, nh, kscale=None, vscale=None):
    """The prefill's copy: the K and V thirds of a padded ``qkv`` [B*S0, 3H] (row layout [3][nh][dh]) into
    ``kcache`` / ``vcache`` [B, nh, S_max, dh], rows below ``min(lens0[b], S0, S_max)`` only.  One HIP launch on GPU
    bf16 tensors, the indexing expression otherwise.  An FP8 cache (``float8_e4m3fn``, with ``kscale`` / ``vscale`` fp32
    [B, nh, S_max]) gets ``kv_quantize`` of those rows: the quantising HIP launch, or that expression."""
    fp8 = _quantised("kv_cache_fill", kcache, kscale, vscale)
    if _native_bf16(qkv):
        return lib().kv_cache_fill(qkv, lens0, kcache, vcache, S0, kscale, vscale)
    kv = qkv.view(B, S0, 3, nh, -1)
    for b, n in enumerate(lens0.tolist()):
        n = max(0, min(n, S0, kcache.shape[2]))
        rows_k, rows_v = kv[b, :n, 1].transpose(0, 1), kv[b, :n, 2].transpose(0, 1)
        if fp8:
            (rows_k, kscale[b, :, :n]), (rows_v, vscale[b, :, :n]) = kv_quantize(rows_k), kv_quantize(rows_v)
        kcache[b, :, :n] = rows_k
        vcache[b, :, :n] = rows_v


def attn_decode(qkv1, lens0, t, max_len, kcache, vcache, window=0, kscale=None, vscale=None):
    """One new token per record against the cache -> (ctx [B, H], lse fp32 [B, nh]).  ``qkv1`` [B, 3H] holds the
    token's q, k, v; record b has ``len = lens0[b] + t`` cached keys (``lens0`` int32 [B], ``t`` and ``max_len >= max
    len`` host ints).  The token sees cached keys ``max(0, len + 1 - window) .. len - 1`` and its own key (window 0:
    every key); its k / v rows are written to cache row ``len``.  The split-KV HIP kernels on GPU bf16 tensors (head
    dim 64; a full cache, ``max_len >= S_max``, is refused); otherwise the mirror: the last row of a causal attention
    over ``cat(cache[:len], new)``.

    An FP8 cache (``float8_e4m3fn`` codes with ``kscale`` / ``vscale`` fp32 [B, nh, S_max], ``kv_quantize``'s format):
    the visible cached rows count as ``code * scale``, the token's own key and value enter this step unquantised, and
    row ``len`` receives their codes and scales.  The FP8 HIP kernels on GPU bf16 ``qkv1``, the mirror otherwise."""
    B, nh, S_max, dh = kcache.shape
    if max_len >= S_max:
        raise ValueError("attn_decode: the cache is full (max_len = %d, S_max = %d)" % (max_len, S_max))
    fp8 = _quantised("attn_decode", kcache, kscale, vscale)
    if _native_bf16(qkv1):
        if not attn_decode_supported(dh, S_max):
            raise ValueError("attn_decode: head dim 64 and 1 <= S_max <= 2**30 required (got head dim %d, S_max = %d)"
                             % (dh, S_max))
        return tuple(lib().attn_decode(qkv1, lens0, t, max_len, kcache, vcache, window, kscale, vscale))
    q, k, v = qkv1.view(B, 3, nh, dh).unbind(1)
    ctx = torch.empty(B, nh, dh, dtype=qkv1.dtype, device=qkv1.device)
    lse = torch.empty(B, nh, dtype=torch.float32, device=qkv1.device)
    for b, n in enumerate((lens0 + t).tolist()):
        lo = max(0, n + 1 - window) if window > 0 else 0
        if fp8:
            (kcache[b, :, n], kscale[b, :, n]), (vcache[b, :, n], vscale[b, :, n]) = kv_quantize(k[b]), kv_quantize(v[b])
            kk, vv = (torch.cat([kv_dequantize(c[b, :, lo:n], s[b, :, lo:n]).to(x.dtype), x[b].unsqueeze(1)], 1)
                      for c, s, x in ((kcache, kscale, k), (vcache, vscale, v)))
        else:
            kcache[b, :, n], vcache[b, :, n] = k[b], v[b]
            kk, vv = kcache[b, :, lo:n + 1], vcache[b, :, lo:n + 1]
        sc = (kk @ q[b].unsqueeze(-1)).squeeze(-1) / math.sqrt(dh)  # [nh, keys]
        lse[b] = torch.logsumexp(sc.float(), -1)
        ctx[b] = (torch.softmax(sc, -1).unsqueeze(1) @ vv).squeeze(1)
    return ctx.view(B, nh * dh), lse


def emb_fwd_at(ids, lens0, t, word, pos, typ):
    """[B, H]: the embedding sum of one token per record at position ``lens0[b] + t``, token type 0 (one HIP launch
    on GPU bf16 tables, the gather otherwise); ``word + (pos + type)``, as ``emb_fwd`` adds."""
    if _native_bf16(word):
        return lib().emb_fwd_at(ids.contiguous(), lens0, t, word, pos, typ)
    return word[ids] + (pos[(lens0 + t).long()] + typ[0])


# ---- several new tokens per record against a KV cache (csrc/kernels/attention_extend.hip) ----------------
def attn_extend_supported(dh, S_max, T):
    """What the extend kernels take: ``attn_decode_supported`` and 1 <= T <= 64 new tokens per record."""
    return attn_decode_supported(dh, S_max) and 1 <= T <= 64


def attn_extend(qkvT, lens0, t, max_len, kcache, vcache, T, window=0, n_new=None):
    """``T`` new tokens per record against the cache -> (ctx [B*T, H], lse fp32 [B, nh, T]).  ``qkvT`` [B*T, 3H]:
    rows ``i < n_new[b]`` (int32 [B] on the tensors' device; None: all T) of record b are its tokens at positions
    ``len + i``, ``len = lens0[b] + t``.  Query i sees cached keys ``max(0, len + i + 1 - window) .. len - 1`` and the
    new keys ``max(0, i + 1 - window) .. i`` (window 0: every key); the tokens' k / v rows are written to cache rows
    ``len .. len + n_new[b] - 1``.  Rows ``i >= n_new[b]`` get zero ctx and lse.  The split-KV MFMA kernels on GPU bf16
    tensors (head dim 64); otherwise the mirror: per record the last rows of a causal attention over
    ``cat(cache[:len], new[:n])``.  ``T`` outside [1, 64], ``max_len + T > S_max`` and an FP8 cache are refused."""
    B, nh, S_max, dh = kcache.shape
    if kcache.dtype == FP8:
        raise ValueError("attn_extend: the quantised (FP8) cache is served by attn_decode only")
    if not 1 <= T <= 64:
        raise ValueError("attn_extend: 1 <= T <= 64 new tokens per record (got %d)" % T)
    if max_len + T > S_max:
        raise ValueError("attn_extend: the cache is full (max_len = %d, T = %d, S_max = %d)" % (max_len, T, S_max))
    if _native_bf16(qkvT):
        if not attn_extend_supported(dh, S_max, T):
            raise ValueError("attn_extend: head dim 64 and 1 <= S_max <= 2**30 required (got head dim %d, S_max = %d)"
                             % (dh, S_max))
        return tuple(lib().attn_extend(qkvT, lens0, t, max_len, kcache, vcache, T, window, n_new))
    q, k, v = qkvT.view(B, T, 3, nh, dh).unbind(2)  # [B, T, nh, dh] each
    ctx = torch.zeros(B, T, nh, dh, dtype=qkvT.dtype, device=qkvT.device)
    lse = torch.zeros(B, nh, T, dtype=torch.float32, device=qkvT.device)
    ns = [T] * B if n_new is None else [max(0, min(int(n), T)) for n in n_new.tolist()]
    for b, (L, n) in enumerate(zip((lens0 + t).tolist(), ns)):
        if n == 0 or L < 0 or L + n > S_max:
            continue
        kcache[b, :, L:L + n], vcache[b, :, L:L + n] = k[b, :n].transpose(0, 1), v[b, :n].transpose(0, 1)
        sc = (q[b, :n].transpose(0, 1) @ kcache[b, :, :L + n].transpose(1, 2)) / math.sqrt(dh)  # [nh, n, L + n]
        sc = sc.masked_fill(_invisible(L + n, window, sc.device)[L:], float("-inf"))
        lse[b, :, :n] = torch.logsumexp(sc.float(), -1)
        ctx[b, :n] = (torch.softmax(sc, -1) @ vcache[b, :, :L + n]).transpose(0, 1)
    return ctx.view(B * T, nh * dh), lse


def emb_fwd_span(ids, lens0, t, word, pos, typ):
    """[B*T, H]: the embedding sums of ids [B, T] at positions ``lens0[b] + t + i``, token type 0 (one HIP launch on
    GPU bf16 tables, the gather otherwise); ``word + (pos + type)``, as ``emb_fwd_at`` adds."""
    if _native_bf16(word):
        return lib().emb_fwd_span(ids.contiguous(), lens0, t, word, pos, typ)
    B, T = ids.shape
    at = (lens0.view(B, 1) + t + torch.arange(T, device=ids.device)).long().clamp(0, pos.shape[0] - 1)
    return (word[ids] + (pos[at] + typ[0])).view(B * T, -1)
