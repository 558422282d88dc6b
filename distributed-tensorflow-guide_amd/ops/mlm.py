"""BERT dynamic masking, one launch per batch (csrc/kernels/mlm_mask.hip).

``mlm_mask(input_ids i32 [B,S], a_len i32 [B], length i32 [B], index i64 [B], seed=, epoch=, P=, ...)`` returns
``(ids, token_type_ids, attention_mask [B,S], mlm_positions, mlm_labels [B,P])``, all int64: what
``BertForPreTraining.forward`` takes.  A row's result is a pure function of (seed, epoch, record index): it does not
depend on the batch the record is in, on the rank that reads it, or on which implementation computes it.  The rule
is integer only (``hash32`` is ``data/sampler.py::hash32``):

* candidates: positions ``j < length`` whose id is none of ``special_ids``; ``n_cand`` of them;
* ``n_pred = 0`` if ``n_cand == 0`` else ``min(P, n_cand, max(1, (n_cand * mask_per_mille + 500) // 1000))``;
* chosen: the ``n_pred`` candidates with the smallest ``((hash32(seed, epoch, index, j, 0) >> (32 - key_bits)) << 32)
  | j`` (``key_bits`` < 32 only makes ties frequent, for tests of the tie-break by position);
* action ``a = (hash32(seed, epoch, index, j, 1) * 10) >> 32``: ``a < 8`` writes ``mask_id``, ``a == 8`` keeps the
  token, ``a == 9`` writes ``vocab_lo + ((hash32(seed, epoch, index, j, 2) * (vocab_hi - vocab_lo)) >> 32)``;
* ``mlm_positions`` ascending with the original ids as ``mlm_labels``; unused slots hold (0, -1);
* rows ``>= valid_rows`` (padding rows of an evaluation pass) are copied unmasked and predict nothing;
* ``length`` and ``a_len`` are clamped to ``[0, S]``.

GPU tensors go through the HIP kernel (a missing extension is an error); CPU tensors through ``mlm_mask_ref``, the
same rule in torch int64 operations, which is also what the kernel is tested against.
"""
import numpy as np
import torch

from ._native import lib

MAX_SEQ = 2048
MAX_SPECIAL = 4
_M32 = 0xFFFFFFFF


def _fmix32(h):
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def hash32_t(*words):
    """``data/sampler.py::hash32`` on int64 tensors (or Python ints) holding 32-bit values: int64 products wrap, and
    the low 32 bits of a wrapped product are those of the exact one."""
    h = 0x9E3779B9
    for w in words:
        w = (w & _M32) if torch.is_tensor(w) else (int(w) & _M32)
        h = _fmix32((h ^ ((w * 0x9E3779B1) & _M32)) & _M32)
        h = (h * 5 + 0xE6546B64) & _M32
    return _fmix32(h)


def n_pred_of(n_cand, P, mask_per_mille):
    """The count rule on a numpy array or a tensor of candidate counts."""
    want = (n_cand * mask_per_mille + 500) // 1000
    if torch.is_tensor(n_cand):
        return torch.minimum(want.clamp(min=1), n_cand).clamp(max=P) * (n_cand > 0)
    return np.minimum(np.minimum(np.maximum(want, 1), n_cand), P) * (n_cand > 0)


def count_valid(input_ids, length, P, mask_per_mille, special_ids, valid_rows=None):
    """Host side of the same count rule: numpy ``input_ids [B,S]``, ``length [B]`` -> ``sum n_pred`` over the first
    ``valid_rows`` rows, the number of labels >= 0 the kernel writes.  No device read."""
    ids, length = np.asarray(input_ids), np.asarray(length)
    B, S = ids.shape
    vr = B if valid_rows is None else int(valid_rows)
    cand = np.arange(S)[None, :] < np.clip(length, 0, S)[:, None]
    for s in special_ids:
        cand &= ids != s
    return int(n_pred_of(cand[:vr].sum(1).astype(np.int64), P, mask_per_mille).sum())


def _check(input_ids, a_len, length, index, P, mask_per_mille, mask_id, vocab_lo, vocab_hi, special_ids, valid_rows,
           key_bits):
    if input_ids.dtype != torch.int32 or input_ids.dim() != 2:
        raise ValueError("input_ids must be int32 [B, S], got %s %s" % (input_ids.dtype, tuple(input_ids.shape)))
    B, S = input_ids.shape
    if not 1 <= S <= MAX_SEQ:
        raise ValueError("1 <= S <= %d required, got %d" % (MAX_SEQ, S))
    for name, t, dt in (("a_len", a_len, torch.int32), ("length", length, torch.int32), ("index", index, torch.int64)):
        if t.dtype != dt or tuple(t.shape) != (B,) or t.device != input_ids.device:
            raise ValueError("%s must be %s [%d] on the device of input_ids" % (name, dt, B))
    if P < 1 or not 0 <= mask_per_mille <= 1000 or not 1 <= key_bits <= 32:
        raise ValueError("P >= 1, 0 <= mask_per_mille <= 1000 and 1 <= key_bits <= 32 required")
    if not (0 <= vocab_lo < vocab_hi < 2 ** 31 and 0 <= mask_id < 2 ** 31):
        raise ValueError("0 <= vocab_lo < vocab_hi < 2^31 and 0 <= mask_id < 2^31 required")
    special_ids = tuple(int(s) for s in special_ids)
    if len(special_ids) > MAX_SPECIAL:
        raise ValueError("at most %d special ids" % MAX_SPECIAL)
    valid_rows = B if valid_rows is None else int(valid_rows)
    if not 0 <= valid_rows <= B:
        raise ValueError("0 <= valid_rows <= B required")
    if input_ids.device.type == "cpu" and B:  # device tensors were validated where they were made (the loader)
        if not bool(((0 <= a_len) & (a_len <= length) & (length <= S)).all()):
            raise ValueError("0 <= a_len <= length <= S required in every row")
    return B, S, special_ids, valid_rows


def mlm_mask_ref(input_ids, a_len, length, index, *, seed, epoch, P, mask_per_mille=150, mask_id, vocab_lo, vocab_hi,
                 special_ids=(), valid_rows=None, key_bits=32):
    """The mirror: the rule above in torch int64 operations (two stable sorts), on the device of ``input_ids``."""
    B, S, special_ids, valid_rows = _check(input_ids, a_len, length, index, P, mask_per_mille, mask_id, vocab_lo,
                                           vocab_hi, special_ids, valid_rows, key_bits)
    dev = input_ids.device
    raw = input_ids.to(torch.int64)
    n = length.to(torch.int64).clamp(0, S).view(B, 1)
    a = a_len.to(torch.int64).clamp(0, S).view(B, 1)
    j = torch.arange(S, device=dev, dtype=torch.int64).view(1, S)
    rows = torch.arange(B, device=dev).view(B, 1)
    cand = (j < n) & (rows < valid_rows)
    for s in special_ids:
        cand &= raw != s
    n_cand = cand.sum(1)
    n_pred = n_pred_of(n_cand, P, mask_per_mille).view(B, 1)
    idx = index.view(B, 1)
    key = hash32_t(seed, epoch, idx, j, 0) >> (32 - key_bits)
    key = torch.where(cand, key, torch.full_like(key, 1 << 32))  # above every real key
    order = torch.sort(key, dim=1, stable=True).indices  # ties break toward the lower position
    rank = torch.empty_like(order).scatter_(1, order, j.expand(B, S))
    chosen = cand & (rank < n_pred)
    act = (hash32_t(seed, epoch, idx, j, 1) * 10) >> 32
    rnd = vocab_lo + ((hash32_t(seed, epoch, idx, j, 2) * (vocab_hi - vocab_lo)) >> 32)
    new = torch.where(act < 8, torch.full_like(raw, mask_id), torch.where(act == 8, raw, rnd))
    ids = torch.where(chosen, new, raw)
    first = torch.sort(torch.where(chosen, j, S), dim=1).values[:, :P]  # chosen positions ascending, then S
    if first.shape[1] < P:
        first = torch.cat([first, first.new_full((B, P - first.shape[1]), S)], 1)
    used = torch.arange(P, device=dev).view(1, P) < n_pred
    positions = torch.where(used, first, torch.zeros_like(first))
    labels = torch.where(used, raw.gather(1, positions), torch.full_like(positions, -1))
    return ids, ((j >= a) & (j < n)).to(torch.int64), (j < n).to(torch.int64), positions, labels


def mlm_mask(input_ids, a_len, length, index, *, seed, epoch, P, mask_per_mille=150, mask_id, vocab_lo, vocab_hi,
             special_ids=(), valid_rows=None, key_bits=32, out=None):
    """-> (ids, token_type_ids, attention_mask, mlm_positions, mlm_labels).  out: optional tuple of the five int64
    destinations, contiguous ``[B,S]`` x 3 and ``[B,P]`` x 2 on the inputs' device (views into larger buffers are
    fine)."""
    B, S, special_ids, valid_rows = _check(input_ids, a_len, length, index, P, mask_per_mille, mask_id, vocab_lo,
                                           vocab_hi, special_ids, valid_rows, key_bits)
    dev = input_ids.device
    if out is not None:
        shapes = [(B, S)] * 3 + [(B, P)] * 2
        if len(out) != 5 or any(t.dtype != torch.int64 or tuple(t.shape) != s or t.device != dev
                                or not t.is_contiguous() for t, s in zip(out, shapes)):
            raise ValueError("out must be five contiguous int64 tensors [B,S] x 3, [B,P] x 2 on the inputs' device")
    kw = dict(seed=seed, epoch=epoch, P=P, mask_per_mille=mask_per_mille, mask_id=mask_id, vocab_lo=vocab_lo,
              vocab_hi=vocab_hi, special_ids=special_ids, valid_rows=valid_rows, key_bits=key_bits)
    if not input_ids.is_cuda:
        res = mlm_mask_ref(input_ids, a_len, length, index, **kw)
        if out is None:
            return res
        for o, r in zip(out, res):
            o.copy_(r)
        return tuple(out)
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.int64, device=dev) for s in [(B, S)] * 3 + [(B, P)] * 2)
    if B:
        lib().mlm_mask(input_ids.contiguous(), a_len.contiguous(), length.contiguous(), index.contiguous(), *out,
                       int(seed) & _M32, int(epoch) & _M32, int(mask_per_mille), int(mask_id), int(vocab_lo),
                       int(vocab_hi), list(special_ids), valid_rows, int(key_bits))
    return tuple(out)
