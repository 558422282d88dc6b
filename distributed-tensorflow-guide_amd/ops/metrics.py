"""Evaluation metrics: per-row cross-entropy and label rank, and their accumulation (csrc/kernels/eval_metrics.hip).

``xent_topk(logits [B, V], labels int64 [B]) -> (loss fp32 [B], rank int32 [B])``

* ``loss[r] = logsumexp(x[r, :]) - x[r, label]``
* ``rank[r] = #{j : x[r, j] > x[r, label]} + #{j < label : x[r, j] == x[r, label]}``: the label's 0-based position in
  a descending sort of the row with ties broken toward the lower column.  Top-k correct is ``rank < k``.
* ``label < 0``: an ignored row (the MLM convention of ``softmax_cross_entropy``), ``loss = 0``, ``rank = -1``.
* ``label >= V``: out of range, ``loss = 0``, ``rank = -2``; the row is never indexed with it.
* the label's logit is NaN, or the row's logsumexp is NaN (a NaN anywhere in the row): ``rank = V``, a miss at every
  k, so a diverged model does not score 100 %.

``metric_accumulate(acc fp64 [8], loss, rank, ks, V)`` adds a batch into ``acc``: ``[0]`` rows with ``rank >= 0``,
``[1]`` the fp64 sum of their loss, ``[2]`` rows with ``rank == -2``, ``[3]`` rows with ``rank == V``, ``[4 + i]`` rows
with ``0 <= rank < ks[i]`` for up to four ``ks``.  Counts are exact in fp64, so one dtype carries everything through
one all-reduce, and nothing is read on the host per batch.

GPU tensors go through the HIP kernels (a missing extension is an error); CPU tensors through the ``*_ref`` mirrors,
which are also what the kernels are tested against.
"""
import torch

from ._native import lib

ACC_SLOTS = 8
MAX_KS = 4


def _check(logits, labels):
    if logits.dim() != 2 or logits.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("logits must be bf16 or fp32 [B, V], got %s %s" % (logits.dtype, tuple(logits.shape)))
    if labels.dtype != torch.int64 or tuple(labels.shape) != (logits.shape[0],):
        raise ValueError("labels must be int64 [%d], got %s %s" % (logits.shape[0], labels.dtype, tuple(labels.shape)))
    if labels.device != logits.device:
        raise ValueError("logits and labels must be on the same device")
    if logits.shape[1] < 1:
        raise ValueError("V >= 1 required")


def _check_acc(acc, loss, rank, ks, V):
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= MAX_KS or min(ks) < 1:
        raise ValueError("1 <= len(ks) <= %d and every k >= 1 required, got %r" % (MAX_KS, ks))
    if acc.dtype != torch.float64 or tuple(acc.shape) != (ACC_SLOTS,) or not acc.is_contiguous():
        raise ValueError("acc must be a contiguous fp64 tensor [%d]" % ACC_SLOTS)
    if loss.dtype != torch.float32 or rank.dtype != torch.int32 or loss.dim() != 1 or loss.shape != rank.shape:
        raise ValueError("loss fp32 [B] and rank int32 [B] required")
    if not (acc.device == loss.device == rank.device):
        raise ValueError("acc, loss and rank must be on the same device")
    if int(V) < 1:
        raise ValueError("V >= 1 required")
    return ks


def xent_topk_ref(logits, labels):
    """The mirror in plain tensor operations (fp32 arithmetic for the loss), on the device of ``logits``."""
    _check(logits, labels)
    B, V = logits.shape
    x = logits.float()
    ignored, beyond = labels < 0, labels >= V
    lab = labels.clamp(0, V - 1)
    xl = x.gather(1, lab[:, None])  # [B, 1]
    cols = torch.arange(V, device=x.device)[None, :]
    above = (x > xl).sum(1) + ((x == xl) & (cols < lab[:, None])).sum(1)
    lse = torch.logsumexp(x, 1)
    rank = torch.where(torch.isnan(xl[:, 0]) | torch.isnan(lse), torch.full_like(above, V), above)
    loss = lse - xl[:, 0]
    zero = torch.zeros((), dtype=loss.dtype, device=x.device)
    loss = torch.where(ignored | beyond, zero, loss)
    rank = torch.where(ignored, torch.full_like(rank, -1), rank)
    rank = torch.where(beyond, torch.full_like(rank, -2), rank)
    return loss, rank.to(torch.int32)


def xent_topk(logits, labels, out=None):
    """-> (loss fp32 [B], rank int32 [B]); see the module docstring.  out: optional ``(loss, rank)`` destinations,
    contiguous ``[B]`` tensors on the logits' device (they may be views into larger buffers)."""
    _check(logits, labels)
    if out is not None:
        lo, ro = out
        B = logits.shape[0]
        if (lo.dtype != torch.float32 or ro.dtype != torch.int32 or tuple(lo.shape) != (B,) or tuple(ro.shape) != (B,)
                or lo.device != logits.device or ro.device != logits.device or not lo.is_contiguous()
                or not ro.is_contiguous()):
            raise ValueError("out must be (fp32 [%d], int32 [%d]) contiguous on the logits' device" % (B, B))
    if not logits.is_cuda:
        loss, rank = xent_topk_ref(logits, labels)
        if out is None:
            return loss, rank
        lo.copy_(loss)
        ro.copy_(rank)
        return lo, ro
    if out is None:
        return lib().xent_rank(logits.contiguous(), labels.contiguous())
    return lib().xent_rank(logits.contiguous(), labels.contiguous(), lo, ro)


def metric_accumulate_ref(acc, loss, rank, ks, V):
    """The mirror: the same eight sums with torch reductions, added into ``acc`` in place."""
    ks = _check_acc(acc, loss, rank, ks, V)
    scored = rank >= 0
    add = torch.zeros(ACC_SLOTS, dtype=torch.float64, device=acc.device)
    add[0] = scored.sum()
    add[1] = torch.where(scored, loss.double(), torch.zeros((), dtype=torch.float64, device=acc.device)).sum()
    add[2] = (rank == -2).sum()
    add[3] = (rank == int(V)).sum()
    for i, k in enumerate(ks):
        add[4 + i] = (scored & (rank < k)).sum()
    acc += add
    return acc


def metric_accumulate(acc, loss, rank, ks, V):
    """acc += this batch's sums, in place; returns ``acc``.  ``B == 0`` adds nothing."""
    ks = _check_acc(acc, loss, rank, ks, V)
    if not acc.is_cuda:
        return metric_accumulate_ref(acc, loss, rank, ks, V)
    lib().metric_accumulate(acc, loss.contiguous(), rank.contiguous(), ks, int(V))
    return acc
