"""Flat-buffer optimizer applies (csrc/kernels/optim.hip) with a CPU reference path.

Every function updates ``master`` (fp32) in place from ``grad`` (fp32 or bf16), optionally
refreshes a bf16 ``mirror`` of the weights, scales the gradient by ``gscale`` (times the device-resident
scalar ``clip`` when one is given) and zeroes it.
``hyper`` is a float32 device tensor {lr, step} so the apply is graph-capturable.
"""
import torch

from ._native import lib


def _cpu_finish(master, mirror, grad, zero_grad):
    if mirror is not None:
        mirror.copy_(master)
    if zero_grad:
        grad.zero_()


def _cpu_clip(gscale, clip):
    """``clip``: an optional one-element tensor (the global-norm clip factor, ops/layerwise.py) multiplied into the
    gradient scale; on the GPU the kernel reads it from device memory."""
    return gscale if clip is None else gscale * float(clip[0])


def sgd(master, grad, hyper, mirror=None, wd=0.0, gscale=1.0, zero_grad=False, clip=None):
    if master.is_cuda:
        return lib().sgd_apply(master, mirror, grad, hyper, wd, gscale, zero_grad, clip)
    gscale = _cpu_clip(gscale, clip)
    lr = float(hyper[0])
    g = grad.float() * gscale + wd * master
    master.add_(g, alpha=-lr)
    _cpu_finish(master, mirror, grad, zero_grad)


def momentum(master, grad, mom, hyper, mirror=None, mu=0.9, wd=0.0, nesterov=False, gscale=1.0, zero_grad=False,
             clip=None):
    if master.is_cuda:
        return lib().momentum_apply(master, mirror, grad, mom, hyper, mu, wd, nesterov, gscale, zero_grad, clip)
    gscale = _cpu_clip(gscale, clip)
    lr = float(hyper[0])
    g = grad.float() * gscale + wd * master
    mom.mul_(mu).add_(g)
    master.add_(g + mu * mom if nesterov else mom, alpha=-lr)
    _cpu_finish(master, mirror, grad, zero_grad)


def adagrad(master, grad, acc, hyper, mirror=None, eps=0.0, gscale=1.0, zero_grad=False, clip=None):
    """TF ApplyAdagrad: acc += g^2 ; w -= lr * g / sqrt(acc)  (SURVEY §2.5 N5)."""
    if master.is_cuda:
        return lib().adagrad_apply(master, mirror, grad, acc, hyper, eps, gscale, zero_grad, clip)
    gscale = _cpu_clip(gscale, clip)
    lr = float(hyper[0])
    g = grad.float() * gscale
    acc.add_(g * g)
    master.sub_(lr * g * torch.rsqrt(acc + eps))
    _cpu_finish(master, mirror, grad, zero_grad)


def adam(master, grad, m, v, hyper, mirror=None, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, gscale=1.0,
         zero_grad=False, clip=None):
    """AdamW (decoupled weight decay); hyper = {lr, step} with step already incremented."""
    if master.is_cuda:
        return lib().adam_apply(master, mirror, grad, m, v, hyper, b1, b2, eps, wd, gscale, zero_grad, clip)
    gscale = _cpu_clip(gscale, clip)
    lr, t = float(hyper[0]), float(hyper[1])
    g = grad.float() * gscale
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    mh = m / (1 - b1 ** t)
    vh = v / (1 - b2 ** t)
    master.sub_(lr * (mh / (vh.sqrt() + eps) + wd * master))
    _cpu_finish(master, mirror, grad, zero_grad)


def hyper_tick(hyper):
    """hyper[1] += 1 on the device (the step counter the fused applies read)."""
    lib().hyper_tick(hyper)


def axpby(acc, g, alpha, beta):
    """acc = alpha * acc + beta * g (window accumulate for DOWNPOUR / ADAG / SDAG)."""
    if acc.is_cuda:
        return lib().axpby(acc, g, alpha, beta)
    acc.mul_(alpha).add_(g.float(), alpha=beta)


# ---- k-way sum-apply (sync PS with backup workers, parallel/sync_ps.py) ---------------------------------------
# The applies above with the effective gradient  g = ((acc or 0) + srcs[0] + ... + srcs[k-1]) * gscale, summed in
# fp32 in exactly that order, 1 <= k <= 8 sources of one dtype, ``acc`` an optional fp32 buffer.  Nothing is zeroed.
MAX_SRCS = 8


def _cpu_sum(srcs, acc, master):
    if not 1 <= len(srcs) <= MAX_SRCS:
        raise RuntimeError("1..8 gradient sources, got %d" % len(srcs))
    if len({s.dtype for s in srcs}) != 1 or any(s.numel() != master.numel() for s in srcs):
        raise RuntimeError("sources must have one dtype and the destination's size")
    g = acc.clone() if acc is not None else torch.zeros_like(master)
    for s in srcs:
        g.add_(s.float())
    return g


def sgd_sum(master, srcs, hyper, mirror=None, wd=0.0, gscale=1.0, acc=None):
    srcs = list(srcs)
    if master.is_cuda:
        return lib().sgd_sum_apply(master, mirror, srcs, hyper, wd, gscale, acc)
    sgd(master, _cpu_sum(srcs, acc, master), hyper, mirror, wd, gscale)


def momentum_sum(master, srcs, mom, hyper, mirror=None, mu=0.9, wd=0.0, nesterov=False, gscale=1.0, acc=None):
    srcs = list(srcs)
    if master.is_cuda:
        return lib().momentum_sum_apply(master, mirror, srcs, mom, hyper, mu, wd, nesterov, gscale, acc)
    momentum(master, _cpu_sum(srcs, acc, master), mom, hyper, mirror, mu, wd, nesterov, gscale)


def adagrad_sum(master, srcs, slot, hyper, mirror=None, eps=0.0, gscale=1.0, acc=None):
    srcs = list(srcs)
    if master.is_cuda:
        return lib().adagrad_sum_apply(master, mirror, srcs, slot, hyper, eps, gscale, acc)
    adagrad(master, _cpu_sum(srcs, acc, master), slot, hyper, mirror, eps, gscale)


def adam_sum(master, srcs, m, v, hyper, mirror=None, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, gscale=1.0, acc=None):
    srcs = list(srcs)
    if master.is_cuda:
        return lib().adam_sum_apply(master, mirror, srcs, m, v, hyper, b1, b2, eps, wd, gscale, acc)
    adam(master, _cpu_sum(srcs, acc, master), m, v, hyper, mirror, b1, b2, eps, wd, gscale)


def grad_sum(acc, srcs, first, scale=1.0):
    """acc = (0 if first else acc) + scale * (srcs[0] + ... + srcs[k-1]), 1 <= k <= 8.  With ``first`` the old
    contents of ``acc`` are not read (NaN / Inf left by an abandoned step cannot leak)."""
    srcs = list(srcs)
    if acc.is_cuda:
        return lib().grad_sum(acc, srcs, bool(first), scale)
    if not 1 <= len(srcs) <= MAX_SRCS:
        raise RuntimeError("1..8 sources, got %d" % len(srcs))
    if len({s.dtype for s in srcs}) != 1 or any(s.numel() != acc.numel() for s in srcs):
        raise RuntimeError("sources must have one dtype and the accumulator's size")
    s = srcs[0].float().clone()
    for t in srcs[1:]:
        s.add_(t.float())
    if first:
        acc.copy_(s.mul_(scale))
    else:
        acc.add_(s, alpha=scale)


# ---- gradient accumulation over micro-batches (parallel/accum.py) ------------------------------------------------
def grad_fold_ref(acc, g, first):
    """The CPU path of :func:`grad_fold` and the mirror its GPU tests compare against: one fp32 add per element."""
    if first:
        acc.copy_(g.float())
    else:
        acc.add_(g.float())
    g.zero_()


def grad_unfold_ref(g, acc, lo, hi):
    """The CPU path of :func:`grad_unfold` and its mirror: one fp32 add and one cast to ``g``'s dtype (round to
    nearest even for bf16, the identity for fp32) per element of [lo, hi)."""
    g[lo:hi] = (acc[lo:hi] + g[lo:hi].float()).to(g.dtype)


def _check_fold(acc, g):
    if acc.dtype != torch.float32 or g.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("acc must be fp32 and g fp32 or bf16, got %s / %s" % (acc.dtype, g.dtype))
    if acc.dim() != 1 or g.dim() != 1 or acc.numel() != g.numel():
        raise RuntimeError("acc and g must be flat buffers of one length")


def grad_fold(acc, g, first):
    """acc = (0 if first else acc) + float(g); g = 0 -- one pass, one launch.  ``acc`` fp32, ``g`` fp32 or bf16 of
    the same length.  With ``first`` the old contents of ``acc`` are not read (no zero fill needed; NaN left by an
    abandoned window cannot leak), the contract of ``grad_sum(first=True)``."""
    _check_fold(acc, g)
    if acc.is_cuda:
        return lib().grad_fold(acc, g, bool(first))
    grad_fold_ref(acc, g, first)


def grad_unfold(g, acc, lo=0, hi=None):
    """g[i] = cast(acc[i] + float(g[i])) for i in [lo, hi) (default: everything); ``acc`` is left as it is.  The
    range form serves DataParallel's buckets, which are slices of a flat group."""
    _check_fold(acc, g)
    hi = g.numel() if hi is None else hi
    if not 0 <= lo <= hi <= g.numel():
        raise RuntimeError("range [%d, %d) outside [0, %d)" % (lo, hi, g.numel()))
    if acc.is_cuda:
        return lib().grad_unfold(g, acc, int(lo), int(hi))
    grad_unfold_ref(g, acc, lo, hi)


def refresh_mirror(master, mirror):
    if master.is_cuda:
        return lib().f32_to_bf16(master, mirror)
    mirror.copy_(master)
