"""ResNet bottleneck as ONE autograd node with a hand-written backward (GPU, bf16, NHWC).

Everything runs on dtg's HIP kernels on [rows, channels] views of NHWC activations:

  forward   y1 = x W1^T (MFMA GEMM)        a1 = relu(bn1(y1))             (fused BN+ReLU)
            y2 = conv3x3(a1, W2, stride)  a2 = relu(bn2(y2))             (implicit-GEMM conv)
            y3 = a2 W3^T                  idn = x | bn_d(conv1x1_s(x, Wd))
            out = relu(bn3(y3) + idn)                                     (fused BN+add+ReLU)
  backward  the residual gradient that BN3's backward emits (dres) is the buffer the first
            conv's dgrad GEMM accumulates into (beta = 1): the "x is used twice" gradient sum
            costs no separate add kernel; conv weight gradients are accumulated straight into
            the flat gradient buffer and BN gamma/beta gradients are accumulated in the BN
            finalize kernel -- autograd sees no parameter gradients at all, the all-reduce
            buckets are notified through parallel/grad_sink.
Strided dgrads (3x3/s2 and the 1x1/s2 projection) run dtg's residue-class dgrad kernel; the
projection's accumulates (beta = 1) straight into the conv1 dgrad output.

BN statistics are fused into the producing GEMM/conv epilogue (csrc/include/dtg/bn_epi.cuh):
forward, every conv output's per-channel sum / sum of squares; backward, the dgrads feeding BN2 and
BN1 emit the relu-masked gradient plus sum(dp) and sum(dp*xhat).  Each BN then costs finalize +
one elementwise pass instead of a reduction pass + finalize + elementwise pass.  _FUSE = False
restores the separate statistics kernels (A/B tests).

BN3 of block i (relu(bn3(y3) + identity) = the block output = block i+1's input) is reduced one
block LATER: block i+1's last dgrad GEMM, the final writer of dL/d out_i, applies block i's relu
mask (out_i > 0, i.e. its own saved input) and reduces block i's BN3 statistics in its epilogue
(mode 3).  The two blocks meet through a _Bn3Link attached to the output tensor.  Block i uses the
partials only if the gradient it receives is that very buffer (so nothing else was summed into it
by autograd); otherwise it falls back to the full BN backward, which re-applies the (idempotent)
mask.

The forward has a cross-block hand-over too (_FWD1): where the shapes allow, block i's BN3 apply pass also computes
block i+1's conv1 output and its BN statistics from the output tile it holds on chip, and passes them along on the
output tensor (_Conv1Ahead); block i+1 takes them only for that very tensor and weight.

Each pass of the node (_BottleneckFn) first decides -- the switches and the *_ok predicates are read once, into an
immutable _FwdPlan / _BwdPlan -- and then runs top to bottom in the order above.
"""
import os
from collections import namedtuple
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from ..ops import conv as conv_ops
from ..ops._native import lib
from ..ops.gemm import gemm
from ..parallel import grad_sink, overlap


def _rows(t):
    n, c, h, w = t.shape
    if not t.is_contiguous(memory_format=torch.channels_last):
        t = t.contiguous(memory_format=torch.channels_last)
    return t.permute(0, 2, 3, 1).reshape(n * h * w, c)


def _mat(w):  # 1x1 conv weight [K, C, 1, 1] -> [K, C]
    return w.reshape(w.shape[0], w.shape[1]) if w.is_contiguous() else w.as_strided((w.shape[0], w.shape[1]),
                                                                                     (w.shape[1], 1))


def _krsc(w):  # channels_last [K, C, R, S] -> contiguous [K, R, S, C] view
    return w.permute(0, 2, 3, 1)


_FUSE = True  # BN statistics in the GEMM/conv epilogues (False: separate statistics kernels, for A/B tests)
_LINK = True  # cross-block BN3 reduction (needs _FUSE)
# linked stride-2 projection: its dgrad writes only the even (h, w) rows, which the next mode-3 GEMM alone
# reads (no zero-fill of a [N, H, W, C] gradient per stage transition); 0 restores the zero-filled form
_SUB2 = True
# (Round-3/4 experiments, removed in round 5 with their kernels -- git history has them: BN2 + relu applied in
# conv3's operand prologues instead of an apply pass, 14.46k vs 14.80k img/s at b512 (profiles/r03_bn2_prologue);
# BN3 / BN1 backward folded into the following 1x1 dgrads over [dp | y] along K, 14.2k vs 15.2k at b1024
# (profiles/r04_bn_fold).)
# _DXW = True: where the shape allows (stage 1: 256 x 64, bn_dx_wgrad_ok), conv3's weight gradient is computed inside
# BN3's dx pass on the main stream (csrc/kernels/bn_dx_wgrad.hip) instead of re-reading dx on the side stream:
# the backward is HBM-bound across both streams, and that re-read cost 0.3 ms of step per block
# (profiles/r04_dx_wgrad).
_DXW = True
_DXW2 = True  # ... and the stage-1 stride-1 projection's weight gradient in the dual form of that pass
# _DXD = True: ... and conv3's data gradient (stage 1, bn_dx_dgrad_ok): dp2 = mask2 * (dy3 W3) and BN2's backward
# partials are computed from the dx tile while the pass holds it in LDS, so dy3 ([P, 256], 1.64 GB at batch 1024) is
# neither written nor read back and the gemm_bn mode-3 launch of these blocks goes away.  The identity blocks use
# the plain form, the projection block the two-weight dual form (needs _DXW2).
# _DXD_S2 = True: the same in stage 2's identity blocks (512 x 128, bn_dx_dgrad_full_ok): there the pass's workgroups
# each covered a 256-channel slice, which would split the K of dy3 W3, so the full-width form gives one workgroup all
# 512 channels of a row block (dy3: [P, 512], 0.82 GB at batch 1024).  The stage-2 projection block stays on the
# GEMM: the dual form of that width does not fit the register file (profiles/r09_dx_dgrad_s2).
_DXD = True
_DXD2 = True  # ... in the projection block too (False: only the identity blocks, for A/B runs)
_DXD_S2 = True
_dxd_calls = 0  # times the fused-dgrad path was taken (tests)
# _DXR = True: stage 1's fused-dgrad dx pass does not read y3 either.  In this model y3 is bf16(a2 W3^T), the forward's
# conv3 (K = 64), and the pass already holds both operands on chip -- the a2 block for the weight gradient, W3 for the
# data gradient -- so it forms each block's y3 again by MFMA (dgx; 36 % of the pass's bytes).  Only for the very weight
# the forward multiplied by (storage and version, as _Conv1Ahead.matches), and only where y3 is at least
# _DXR_MIN_BYTES: a y3 that fits the 256 MiB Infinity Cache can be served from it rather than from HBM, and the
# recompute only trades an HBM read for MFMA and L2 work.  The forward is untouched: y3 is still written and saved (the
# apply pass and the next block's mode-3 GEMM read it).
_DXR = True
_DXR_MIN_BYTES = 256 << 20
_dxr_calls = 0  # times the dx pass recomputed y3 (tests)
# _FWD1 = True: the forward mirror of _DXD.  Block i's output out = relu(bn3(y3) + identity) ([P, 256], 1.64 GB at
# batch 1024 in stage 1) was written by BN3's apply pass and read straight back by block i+1's conv1 (gemm_bn mode 1).
# Where the shape allows (bn_apply_gemm_ok: 256 -> 64 inside stage 1, 256 -> 128 into stage 2) the apply pass computes
# y1n = out W1n^T and its BN statistics from the tile it holds on chip (csrc/kernels/bn_dx_wgrad.hip,
# bn_apply_gemm_kernel) and hands them to block i+1 on the output tensor (_Conv1Ahead); out is still written: it is
# the residual and conv1's weight-gradient operand.  The backward is untouched.
_FWD1 = True
# _FWD1_S2 = True: the same inside stage 2 (512 -> 128, both forms; out: [P, 512], 0.82 GB): a workgroup of 8 waves owns
# all 512 channels of a row block, one workgroup per CU.  Needs _FWD1.
_FWD1_S2 = True
_fwd1_calls = 0  # times a block took its conv1 output from the previous block's apply pass (tests)


class _Conv1Ahead:
    """Block i+1's conv1 output and its pooled statistics slot, computed by block i's BN3 apply pass."""
    __slots__ = ("out", "w_ptr", "w_ver", "y1n", "part")

    def __init__(self, out, w, wm, y1n, part):
        self.out, self.w_ptr, self.w_ver, self.y1n, self.part = out, wm.data_ptr(), w._version, y1n, part

    def matches(self, x2, w, wm):
        """Only for that very input and that very (unmodified) weight storage."""
        return (self.part is not None and x2.data_ptr() == self.out.data_ptr() and x2.shape == self.out.shape
                and wm.data_ptr() == self.w_ptr and w._version == self.w_ver and wm.shape[0] == self.y1n.shape[1])

    def take(self):
        r = (self.y1n, self.part)
        self.out = self.y1n = self.part = None
        return r

    def drop(self):
        if self.part is not None:
            self.part.zero_()  # pooled slots must go back zeroed (see bn_part in csrc/bindings/ops.cc)
        self.out = self.y1n = self.part = None

    def __del__(self):  # never consumed (the output went somewhere else than into the next block)
        try:
            self.drop()
        except Exception:
            pass


def _next_conv1(blk, x, rows, cout):
    """The following block's conv1 weight as a detached [N, cout] matrix, if BN3's apply pass can compute that conv."""
    nxt = blk._next[0] if blk._next else None
    if nxt is None or not nxt.fused or not _fused_ok(nxt, x.is_cuda, x.dtype, cout):
        return None
    w = nxt.c1.conv.weight
    if w.shape[1] != cout or w.device != x.device:
        return None
    if not lib().bn_apply_gemm_ok(rows, cout, w.shape[0]) or (cout == 512 and not _FWD1_S2):
        return None
    if blk.down is not None and cout == 256 and w.shape[0] != 64:  # no two-BN form at 256 x 128
        return None
    return w


class _Bn3Link:
    """Block i's BN3 tensors, filled with the mode-3 partials by block i+1's backward.  For a projection
    block also its shortcut BN's input and statistics (yd, md, idd): the same masked gradient feeds
    that BN, so block i+1's epilogue reduces its statistics too (part2)."""
    __slots__ = ("y3", "m3", "i3", "gamma", "beta", "bits", "yd", "md", "idd", "part", "part2", "dp")

    def __init__(self, y3, m3, i3, gamma, beta, bits, yd=None, md=None, idd=None):
        self.y3, self.m3, self.i3, self.gamma, self.beta = y3, m3, i3, gamma, beta
        self.bits = bits  # packed (out > 0): the relu mask, 1/16 of the bytes of re-reading out
        self.yd, self.md, self.idd = yd, md, idd
        self.part = self.part2 = self.dp = None


def _gacc(p):
    """The buffer a parameter's gradient is accumulated into (its flat view, or a fresh one)."""
    if grad_sink.enabled(p):
        return p.grad, True
    return torch.zeros_like(p, dtype=torch.float32 if p.dim() <= 1 else p.dtype), False


# _BITS = False: the backward recomputes BN1/BN2's relu masks from y and the BN statistics (mode 2)
# instead of reading the packed masks the forward apply wrote (mode 3, 1/16 of y's bytes)
_BITS = True


# Split-K targets (workgroups) of the weight gradients when they run on the side stream (parallel/overlap.py,
# one rank): there they overlap the dgrad / BN-backward chain, and fewer, longer splits (fewer fp32 partial
# slabs, fewer CUs taken from the main stream) measured faster -- ResNet-50 b512 13.99k -> 14.19k img/s
# for the 1x1 GEMM wgrads at 128 instead of 512, and +0.7 % for the 3x3 conv wgrads at 512 instead of
# 1024.  On the main stream (several ranks, or DTG_WGRAD_STREAM=0) the kernels' own defaults stay: there
# 128 ran 12.4k vs 13.67k img/s (profiles/r02_wgrad_split_policy).  DTG_RESNET_WSPLIT_WGS /
# DTG_RESNET_CWSPLIT_WGS override the side-stream targets (0: the defaults).  Round 4 at b1024, with the stage-1/2
# conv3 weight gradients fused into the dx passes: 1x1 at 256 beats 128 by 0.3-0.5 % (64: -6 %, 512: +0.1-0.4 %),
# and with the 1x1 at 256 the 3x3 at 256 beats 512 by 0.5 % (128: -3 %, 1024: -0.4 %; profiles/r04_wgrad_split).
_WSPLIT_WGS = int(os.environ.get("DTG_RESNET_WSPLIT_WGS", "256"))
_CWSPLIT_WGS = int(os.environ.get("DTG_RESNET_CWSPLIT_WGS", "256"))
_wsplit_cache = {}


def _wgrad(dy, x, out):
    """out (+)= dy^T x for [P, M] dy and [P, N] x (P pixels): a 1x1 conv weight gradient, in a side-stream scope."""
    with overlap.wgrad_scope(dy, x):
        tgt = _WSPLIT_WGS if overlap.enabled() else 0
        key = (dy.shape[1], x.shape[1], dy.shape[0], tgt)
        sk = _wsplit_cache.get(key)
        if sk is None:
            sk = _wsplit_cache[key] = lib().gemm_pick_split(key[0], key[1], key[2], False, tgt) if tgt > 0 else 0
        gemm(dy, False, x, False, out=out, beta=1.0, split_k=sk)


def _conv_wgrad(dy4, x4, dw, st, pad):
    """dw (+)= 3x3 / strided conv weight gradient, in a side-stream scope with its split target (see above)."""
    with overlap.wgrad_scope(dy4, x4):
        lib().conv_wgrad(dy4, x4, dw, 1.0, st, pad, target_wgs=_CWSPLIT_WGS if overlap.enabled() else 0)


def _params(blk):
    """The block's parameters, in the order forward takes them and backward returns their gradients."""
    return [p for cb in (blk.c1, blk.c2, blk.c3, blk.down) if cb is not None
            for p in (cb.conv.weight, cb.bn.weight, cb.bn.bias)]


def _bn_args(bn):  # what the forward BN ops take: affine, running statistics, momentum, eps
    return bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps


def _grad_out(p, acc, direct):
    """What a backward returns for p: nothing if accumulated straight into the flat gradient (its bucket is notified)"""
    if direct:
        grad_sink.notify(p)
        return None
    return acc.to(p.dtype)


class _Grads:
    """The accumulators (_gacc) of a block's parameter gradients: g(p), g.bn(bn) = (dgamma, dbeta)."""
    def __init__(self, params):
        self.params, self.accs = params, [_gacc(p) for p in params]
        self._of = {id(p): a for p, (a, _) in zip(params, self.accs)}

    def __call__(self, p):
        return self._of[id(p)]

    def bn(self, bn):
        return self._of[id(bn.weight)], self._of[id(bn.bias)]

    def finish(self, device):
        if not all(direct for _, direct in self.accs):
            overlap.sync_current(device)  # side-stream wgrads land in these before autograd adds them
        return [_grad_out(p, a, direct) for p, (a, direct) in zip(self.params, self.accs)]


# The four native BN passes whose result tuple depends on what was fused into them (nxt: next_w, next_part; fused: wact,
# wgrad, wact2, wgrad2, dg*), with named results.  A dx pass that went on to conv3's dgrad returns no dx but dp, part:
# the masked gradient below conv3 and BN2's backward partials (a pooled slot).
_Applied = namedtuple("_Applied", "out mean inv mean2 inv2 y1n", defaults=(None,) * 3)
_Dx = namedtuple("_Dx", "dx dx2 dp part", defaults=(None,) * 3)


def _bn_fwd_part(y, part, res, bn, bits, **nxt):
    r = lib().bn_fwd_part(y, part, res, *_bn_args(bn), True, bits=bits, **nxt)
    return _Applied(r[0], r[1], r[2], y1n=r[3] if nxt else None)


def _bn_fwd2_part(y, part, bn, y2, part2, bn2, bits, **nxt):  # relu(bn(y) + bn2(y2)) in one pass
    assert bn2.momentum == bn.momentum and bn2.eps == bn.eps
    r = lib().bn_fwd2_part(y, part, *_bn_args(bn)[:4], y2, part2, *_bn_args(bn2)[:4], bn.momentum, bn.eps, bits=bits,
                           **nxt)
    return _Applied(r[0], r[1], r[2], r[3], r[4], r[5] if nxt else None)


def _bn_bwd_part(dp, y, part, bn, mean, inv, acc, **fused):
    r = lib().bn_bwd_part(dp, y, part, bn.weight, mean, inv, False, *acc, **fused)
    return _Dx(r[0], None, r[4], r[5]) if "dgw" in fused else _Dx(r[0])


def _bn_bwd2_part(dp, y, part, bn, mean, inv, acc, y2, part2, bn2, mean2, inv2, acc2, **fused):  # both dx in one pass
    r = lib().bn_bwd2_part(dp, y, part, bn.weight, mean, inv, *acc, y2, part2, bn2.weight, mean2, inv2, *acc2, **fused)
    return _Dx(r[0], r[1], r[2], r[3]) if "dgw" in fused else _Dx(r[0], r[1])


# The steps that exist with and without _FUSE.  Unfused, a producer returns None for the partial sums of its output.
def _conv_fwd(fuse, x2, nhw, w, st, pad):
    """conv(x, w) as [rows, K] for x2 = the rows of an [n, h, w, C] tensor; a 1x1 / stride-1 conv is a GEMM."""
    L = lib()
    if w.shape[2] == 1 and st == 1:
        return L.gemm_bn(x2, _mat(w), 1, pooled=True) if fuse else (gemm(x2, True, _mat(w), True), None)
    x4 = x2.view(*nhw, -1)
    y, part = L.conv_fwd_bn(x4, _krsc(w), st, pad, pooled=True) if fuse else (L.conv_fwd(x4, _krsc(w), st, pad), None)
    return y.view(-1, w.shape[0]), part


def _bn_relu_fwd(y, part, bn):
    """relu(bn(y)), the saved mean and invstd, and the packed relu mask (None: unfused, or _BITS off)."""
    if part is None:
        return (*lib().bn_fwd_train(y, None, *_bn_args(bn), True), None)
    bits = torch.empty(y.shape[0], y.shape[1] // 8, device=y.device, dtype=torch.uint8) if _BITS else None
    r = _bn_fwd_part(y, part, None, bn, bits)
    return r.out, r.mean, r.inv, bits


def _bn_relu_bwd(dp, part, a, y, mean, inv, bn, acc):
    """dL/dy of a = relu(bn(y)): from the masked gradient and its partials; unfused (part None), the full backward."""
    if part is not None:
        return _bn_bwd_part(dp, y, part, bn, mean, inv, acc).dx
    dy, _, _, _ = lib().bn_bwd(dp, a, y, bn.weight, mean, inv, True, False, *acc)
    return dy


# The choices of a pass: made before its first launch (the forward's at the top of forward()), not revised afterwards.
_FwdPlan = namedtuple("_FwdPlan", "fuse link ahead next_w")
_BwdPlan = namedtuple("_BwdPlan", "fuse linked dual wg3 wgd dgrad dgfull dgx lk_in sub2")


def _w_id(w):  # a weight as a GEMM saw it: its matrix storage and version
    return _mat(w).data_ptr(), w._version


def _plan_bwd(ctx, do, y3):
    """BN3's dx pass has five forms: the full backward (not linked) and, on a linked gradient, the plain pass, + wg3,
    + wg3 + dgrad (dgfull: at stage 2's width), and the dual pass (+ wg3, + wg3 + wgd, + wg3 + wgd + dgrad).  It yields
    dy3, or with dgrad dp2 / q2 instead, and with dual dyd."""
    L = lib()
    n, c, h, w, st, width, cout, _, _ = ctx.geom
    rows, lk, lk_in = do.shape[0], ctx.link_out, ctx.link_in
    fuse = _FUSE
    bits2 = fuse and ctx.bits12[1] is not None  # the fused dgrad needs the forward's packed mask
    # what the shape lets the pass take along: conv3's weight gradient, and conv3's dgrad with BN2's backward partials
    wg3 = bool(_DXW and L.bn_dx_wgrad_ok(rows, cout, width))
    dg = bool(wg3 and bits2 and _DXD and L.bn_dx_dgrad_ok(rows, cout, width))
    dgfull = bool(wg3 and bits2 and _DXD_S2 and L.bn_dx_dgrad_full_ok(rows, cout, width))  # identity blocks only
    # linked: dout is the very buffer block i+1's mode-3 GEMM wrote, so nothing else was summed into it: it is masked
    # and BN3's statistics are reduced; dual: the shortcut BN's too (projection block), both dx in one pass over it
    linked = lk is not None and lk.part is not None and do.data_ptr() == lk.dp.data_ptr() and do.shape == lk.dp.shape
    dual = linked and lk.part2 is not None
    # wgd: stage 1's stride-1 projection's weight gradient (dyd^T x) too; the dual pass has the dgrad only with both
    wgd = bool(dual and wg3 and _DXW2 and st == 1 and c == width == 64 and cout == 256)
    dgrad = linked and ((dg and wgd and _DXD2) if dual else (dg or dgfull))
    dgfull = dgrad and not dual and dgfull
    # dgx: the pass recomputes y3 instead of reading it (_DXR).  The size first, in Python: below it nothing is asked
    dgx = bool(_DXR and dgrad and not dgfull and y3.numel() * 2 >= _DXR_MIN_BYTES
               and ctx.w3_id == _w_id(ctx.blk.c3.conv.weight) and L.bn_dx_recompute_ok(rows, cout, width, dual))
    # lk_in: the previous block's link, if conv1's dgrad finishes that block's BN3 reduction (mode 3); sub2: the
    # stride-2 projection's dgrad then writes the even (h, w) rows only and mode 3 reads just those
    if lk_in is not None and lk_in.y3.shape != (n * h * w, c):
        lk_in = None
    sub2 = bool(lk_in is not None and ctx.blk.down is not None and st == 2 and _SUB2)
    return _BwdPlan(fuse=fuse, linked=linked, dual=dual, wg3=linked and wg3, wgd=wgd, dgrad=dgrad,
                    dgfull=dgfull, dgx=dgx, lk_in=lk_in, sub2=sub2)


class _BottleneckFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, blk, link_in, hand, ahead, *params):
        global _fwd1_calls
        n, c, h, w = x.shape
        st, width, cout = blk.c2.conv.stride, blk.c1.conv.weight.shape[0], blk.c3.conv.weight.shape[0]
        p_, q_ = (h + 2 - 3) // st + 1, (w + 2 - 3) // st + 1
        x2 = _rows(x)
        b1, b2, b3 = blk.c1.bn, blk.c2.bn, blk.c3.bn
        w1, w2, w3 = blk.c1.conv.weight, blk.c2.conv.weight, blk.c3.conv.weight
        # link: BN3's backward reduction is left to the next block; ahead: conv1's output and statistics come from the
        # previous block's BN3 apply pass; next_w: the next block's conv1 weight if this block's apply pass computes it
        fuse = _FUSE
        plan = _FwdPlan(fuse=fuse, link=fuse and _LINK,
                        ahead=fuse and ahead is not None and ahead.matches(x2, w1, _mat(w1)),
                        next_w=_next_conv1(blk, x, n * p_ * q_, cout) if fuse and _FWD1 else None)
        # conv1 -> BN1 + relu -> conv2 (3x3) -> BN2 + relu -> conv3
        if plan.ahead:
            y1, p1 = ahead.take()
            _fwd1_calls += 1
        else:
            if ahead is not None:
                ahead.drop()
            y1, p1 = _conv_fwd(fuse, x2, (n, h, w), w1, 1, 0)
        a1, m1, i1, bits1 = _bn_relu_fwd(y1, p1, b1)
        y2, p2 = _conv_fwd(fuse, a1, (n, h, w), w2, st, 1)
        a2, m2, i2, bits2 = _bn_relu_fwd(y2, p2, b2)
        y3, p3 = _conv_fwd(fuse, a2, (n, p_, q_), w3, 1, 0)
        # the shortcut's projection
        bd = blk.down.bn if blk.down is not None else None
        yd, pd = _conv_fwd(fuse, x2, (n, h, w), blk.down.conv.weight, st, 0) if bd is not None else (None, None)
        # out = relu(bn3(y3) + identity), its packed mask, the next block's conv1 with a pooled slot for its statistics
        bits = torch.empty(y3.shape[0], cout // 8, device=y3.device, dtype=torch.uint8) if plan.link else None
        nxt = {}
        if plan.next_w is not None:
            nxt = dict(next_w=_mat(plan.next_w.detach()),
                       next_part=lib().bn_part_alloc(y3, plan.next_w.shape[0], pooled=True))
        if not fuse:  # the shortcut BN on its own, then BN3 + add + relu
            idn, md, idd = (x2, None, None) if yd is None else lib().bn_fwd_train(yd, None, *_bn_args(bd), False)
            r = _Applied(*lib().bn_fwd_train(y3, idn, *_bn_args(b3), True), md, idd)
        elif yd is not None:  # both BNs in one pass (no materialised identity branch)
            r = _bn_fwd2_part(y3, p3, b3, yd, pd, bd, bits, **nxt)
        else:
            r = _bn_fwd_part(y3, p3, x2, b3, bits, **nxt)
        ctx.blk, ctx.geom, ctx.bits12 = blk, (n, c, h, w, st, width, cout, p_, q_), (bits1, bits2)
        ctx.w3_id = _w_id(w3)  # y3 = a2 w3^T holds for this weight only (_DXR)
        ctx.link_in = link_in if plan.link else None
        ctx.link_out = hand.bn3 = (_Bn3Link(y3, r.mean, r.inv, b3.weight, b3.bias, bits, yd, r.mean2, r.inv2)
                                   if plan.link else None)
        if r.y1n is not None:
            hand.conv1 = _Conv1Ahead(r.out, plan.next_w, nxt["next_w"], r.y1n, nxt["next_part"])
        ctx.save_for_backward(x2, y1, a1, m1, i1, y2, a2, m2, i2, y3, r.out, r.mean, r.inv,
                              *((yd, r.mean2, r.inv2) if yd is not None else ()))
        return r.out.view(n, p_, q_, cout).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout):
        global _dxd_calls, _dxr_calls
        L = lib()
        blk = ctx.blk
        n, c, h, w, st, width, cout, p_, q_ = ctx.geom
        x2, y1, a1, m1, i1, y2, a2, m2, i2, y3, out, m3, i3, *down = ctx.saved_tensors
        b1, b2, b3 = blk.c1.bn, blk.c2.bn, blk.c3.bn
        w1, w2, w3 = blk.c1.conv.weight, blk.c2.conv.weight, blk.c3.conv.weight
        bd, wd = (blk.down.bn, blk.down.conv.weight) if blk.down is not None else (None, None)
        g = _Grads(_params(blk))
        do = _rows(dout)
        plan = _plan_bwd(ctx, do, y3)
        (bits1, bits2), lk, lk_in = ctx.bits12, ctx.link_out, plan.lk_in
        ctx.bits12 = ctx.link_in = None
        # BN3 (+ residual, relu): dres is the gradient flowing into the identity branch
        dyd = None
        if plan.linked:  # block i+1 already masked dL/d out (do is dp) and reduced this BN's statistics
            fused = {}
            if plan.wg3:
                fused.update(wact=a2, wgrad=g(w3).view(cout, width))
            if plan.wgd:
                fused.update(wact2=x2, wgrad2=g(wd).view(cout, c))
            if plan.dgrad:  # the fused dgrad's operands: conv3's weight and the BN below it (BN2)
                fused.update(dgw=_mat(w3), dgy=y2, dgmean=m2, dginv=i2, dgbits=bits2,
                             dgpart=L.bn_part_alloc(y2, width, pooled=True), dgfull=plan.dgfull)
                _dxd_calls += 1
            if plan.dgx:
                fused.update(dgx=True)
                _dxr_calls += 1
            if plan.dual:
                r = _bn_bwd2_part(do, y3, lk.part, b3, m3, i3, g.bn(b3), down[0], lk.part2, bd, down[1], down[2],
                                  g.bn(bd), **fused)
            else:
                r = _bn_bwd_part(do, y3, lk.part, b3, m3, i3, g.bn(b3), **fused)
            dy3, dyd, dp2, q2 = r
            dres = do  # our own buffer (pointer-checked by the plan): dx accumulates into it in place
        else:
            for pt in ((lk.part, lk.part2) if lk is not None else ()):
                if pt is not None:
                    pt.zero_()  # pooled slots must go back zeroed (see bn_part in csrc/bindings/ops.cc)
            dy3, dres, _, _ = L.bn_bwd(do, out, y3, b3.weight, m3, i3, True, True, *g.bn(b3))
        if lk is not None:
            lk.part = lk.part2 = lk.dp = None
        # conv3 (1x1): its dgrad epilogue masks by BN2's relu and reduces BN2's statistics; each unless the dx pass did
        if not plan.fuse:
            dp2, q2 = gemm(dy3, True, _mat(w3), False), None
        elif not plan.dgrad:  # the mask from the forward's bits (mode 3, nothing to accumulate) or recomputed (mode 2)
            dp2, q2 = L.gemm_bn(dy3, _mat(w3), 3 if bits2 is not None else 2, y2, m2, i2, b2.weight, b2.bias,
                                mask=bits2, pooled=True)
        if not plan.wg3:
            _wgrad(dy3, a2, g(w3).view(cout, width))
        # BN2 + conv2 (3x3): its dgrad epilogue does the same for BN1; then BN1
        dy2_4 = _bn_relu_bwd(dp2, q2, a2, y2, m2, i2, b2, g.bn(b2)).view(n, p_, q_, width)
        if plan.fuse:
            dp1, q1 = L.conv_dgrad_bn(dy2_4, _krsc(w2).contiguous(), h, w, st, 1, y1, m1, i1, b1.weight, b1.bias,
                                       pooled=True, bits=bits1)
        else:
            dp1, q1 = L.conv_dgrad(dy2_4, _krsc(w2).contiguous(), h, w, st, 1), None
        dp1 = dp1.view(-1, width)
        _conv_wgrad(dy2_4, a1.view(n, h, w, width), g(w2).permute(0, 2, 3, 1), st, 1)
        dy1 = _bn_relu_bwd(dp1, q1, a1, y1, m1, i1, b1, g.bn(b1))
        # the shortcut: dx2 starts as its gradient, conv1's dgrad accumulates into it
        if blk.down is None:
            dx2 = dres
        else:
            if dyd is None:
                dyd, _, _, _ = L.bn_bwd(dres, None, down[0], bd.weight, down[1], down[2], False, False, *g.bn(bd))
            dyd4 = dyd.view(n, p_, q_, cout)
            if st == 1:
                dx2 = gemm(dyd, True, _mat(wd), False)
            elif lk_in is not None:  # projection dgrad first, so the conv1 dgrad GEMM is the last writer
                dx2 = L.conv_dgrad(dyd4, _krsc(wd).contiguous(), h, w, st, 0, zero_rest=not plan.sub2).view(-1, c)
            else:  # no link to fill: conv1's dgrad here, the projection's accumulates into it
                dx2 = gemm(dy1, True, _mat(w1), False)
                L.conv_dgrad(dyd4, _krsc(wd).contiguous(), h, w, st, 0, out=dx2.view(n, h, w, c), beta=1.0)
            if st != 1:
                _conv_wgrad(dyd4, x2.view(n, h, w, c), g(wd).permute(0, 2, 3, 1), st, 0)
            elif not plan.wgd:
                _wgrad(dyd, x2, g(wd).view(cout, c))
        # conv1 (1x1): its dgrad accumulates into dx2
        if lk_in is not None:  # mode 3: finish the previous block's BN3 reduction (its shortcut BN's too, if it has one)
            part2 = L.bn_part_alloc(dp1, c, pooled=True) if lk_in.yd is not None else None
            _, part = L.gemm_bn(dy1, _mat(w1), 3, lk_in.y3, lk_in.m3, lk_in.i3, lk_in.gamma, lk_in.beta,
                                mask=lk_in.bits, out=dx2, pooled=True, x2=lk_in.yd, mean2=lk_in.md,
                                invstd2=lk_in.idd, part2=part2, sub2_hw=(h, w) if plan.sub2 else None)
            lk_in.part, lk_in.part2, lk_in.dp = part, part2, dx2
        elif blk.down is None or st == 1:
            gemm(dy1, True, _mat(w1), False, out=dx2, beta=1.0)
        _wgrad(dy1, x2, g(w1).view(width, c))
        return (dx2.view(n, h, w, c).permute(0, 3, 1, 2), None, None, None, None, *g.finish(x2.device))


def _fused_ok(blk, is_cuda, dtype, cin):
    ws = [blk.c1.conv.weight, blk.c2.conv.weight, blk.c3.conv.weight]
    return (blk.training and is_cuda and dtype == torch.bfloat16 and all(v.dtype == torch.bfloat16 for v in ws)
            and cin % 64 == 0 and blk.c1.conv.weight.shape[0] % 64 == 0)


def fused_ok(blk, x):
    return _fused_ok(blk, x.is_cuda, x.dtype, x.shape[1])


def bottleneck(blk, x):
    hand = SimpleNamespace(bn3=None, conv1=None)  # what forward leaves to attach to the output tensor
    y = _BottleneckFn.apply(x, blk, getattr(x, "_dtg_bn3", None), hand, getattr(x, "_dtg_conv1", None), *_params(blk))
    if hand.bn3 is not None:
        y._dtg_bn3 = hand.bn3
    if hand.conv1 is not None:
        y._dtg_conv1 = hand.conv1
    return y


# ---- stem: 7x7/2 conv (8-channel padded input) -> BN -> ReLU -> 3x3/2 max-pool, one autograd node ------
# csrc/kernels/stem.hip: the BN statistics come from the conv epilogue, BN+ReLU+pool is one pass over the
# conv output, and the backward recomputes the pre-pool gradient inside both BN-backward passes, so
# neither the BN output nor the pre-pool gradient (411 MB each at batch 256) is ever written.
# _STEM = False restores conv -> BN -> max-pool as separate ops (A/B tests).
_STEM = True
_POOL = (3, 2, 1)  # ResNet's stem max-pool: 3x3, stride 2, pad 1
# _STEM_YAM = True: the forward pool also saves y at each window's argmax ([N, 56, 56, 64], 1/4 of y), so the
# backward's BN statistics pass runs over the pooled tensors instead of gathering over y (csrc/kernels/stem.hip
# stem_bwd_pooled_stats_kernel; exact same terms, another summation order)
_STEM_YAM = True
# stem weight gradient (pixel-pair form): LDS schedule 3 (register-pipelined) and 512 split-K workgroups, measured
# 674 vs 748-878 us at b1024 for the default single stage / 1024 (tools/stem_wgrad_ab.py, profiles/r04_stem_pooled);
# 0 / 0 restore the defaults
_STEM_WG_SCHED = 3
_STEM_WG_WGS = 512


class _StemFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stem, w, gamma, beta):
        L = lib()
        n, c, h, wd = x.shape
        conv, bn = stem.conv, stem.bn
        k, _, r, s = w.shape
        st, pad = conv.stride, conv.padding
        if conv_ops.stem_pairs_ok(x, w, st):  # 4 channels x 2 pixels per 16-B chunk (ops/conv.py stem_pairs)
            x8, w8, (rk, sk) = conv_ops.stem_pairs(x, w, st, pad)
            y4, part = L.conv_fwd_c8(x8, w8, rk, sk, st, 0, True, stride_w=1)  # + BN statistics in the epilogue
            ctx.pairs = True
        else:
            ctx.pairs = False
            x8 = F.pad(x.permute(0, 2, 3, 1), (0, 8 - c)).contiguous()   # [N, H, W, 8]
            w8 = F.pad(w.permute(0, 2, 3, 1), (0, 8 - c)).reshape(k, r * s * 8)
            kp = (r * s * 8 + 63) // 64 * 64
            w8 = F.pad(w8, (0, kp - r * s * 8)).contiguous()           # [K, Kp], (r, s, c) columns
            y4, part = L.conv_fwd_c8(x8, w8, r, s, st, pad, True)      # + BN statistics in the epilogue
        yam_ok = _STEM_YAM and L.stem_pooled_stats_ok(y4.shape[-1])
        res = L.stem_bn_pool_fwd(y4, part, gamma, beta, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
                                 *_POOL, save_yam=yam_ok)
        out, idx, smean, sinv = res[:4]
        ctx.save_for_backward(x8, y4, idx, smean, sinv, res[4] if yam_ok else None)
        ctx.stem = stem
        ctx.geom = (c, k, r, s, st, pad)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout):
        L = lib()
        x8, y4, idx, smean, sinv, yam = ctx.saved_tensors
        c, k, r, s, st, pad = ctx.geom
        stem = ctx.stem
        w, gamma, beta = stem.conv.weight, stem.bn.weight, stem.bn.bias
        (dg, dg_direct), (db, db_direct) = _gacc(gamma), _gacc(beta)
        do4 = dout.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
        dy4 = L.stem_bn_pool_bwd(do4, idx, y4, gamma, beta, smean, sinv, *_POOL, dgamma_acc=dg, dbeta_acc=db,
                                 yam=yam)[0]
        if ctx.pairs:  # pair form: the stored input is [N, Hp, Wp/2, 8]
            dwp = torch.empty(k, r, (s + 1) // 2, 8, device=x8.device, dtype=torch.float32)  # beta 0: overwritten
            L.conv_wgrad(dy4, x8, dwp, 0.0, st, 0, stride_w=1, sched=_STEM_WG_SCHED,
                         target_wgs=_STEM_WG_WGS)
        else:
            dwp = torch.empty(k, r, s, 8, device=x8.device, dtype=torch.float32)
            L.conv_wgrad(dy4, x8, dwp, 0.0, st, pad)
        if grad_sink.enabled(w):
            L.stem_dw_add(dwp, w.grad, ctx.pairs)  # straight into the flat gradient's [K, R, S, C] memory
            dw = _grad_out(w, None, True)
        else:
            dw = conv_ops.stem_pairs_dw(dwp, c, s) if ctx.pairs else dwp[..., :c].permute(0, 3, 1, 2)
            dw = _grad_out(w, dw, False).contiguous(memory_format=torch.channels_last)
        return (None, None, dw, _grad_out(gamma, dg, dg_direct), _grad_out(beta, db, db_direct))


def stem_ok(stem, x):
    w = stem.conv.weight
    return (_STEM and stem.training and x.is_cuda and x.dtype == torch.bfloat16 and not x.requires_grad
            and w.dtype == torch.bfloat16 and x.shape[1] <= 8 and w.shape[0] % 64 == 0
            and x.is_contiguous(memory_format=torch.channels_last))


def stem_pool(stem, x):
    """max_pool2d(relu(bn(conv(x))), 3, 2, 1) for the ResNet stem as one fused autograd node."""
    return _StemFn.apply(x, stem, stem.conv.weight, stem.bn.weight, stem.bn.bias)
