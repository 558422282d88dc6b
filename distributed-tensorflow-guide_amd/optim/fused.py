"""Fused flat-buffer optimizers for the north-star models (one kernel launch per dtype group).

The per-step hyper-parameters (learning rate, step count) live in a device tensor so a whole
training step can be captured in a hipGraph and replayed with a new schedule value.
"""
import torch

from ..ops import layerwise as L
from ..ops import optim_kernels as K
from ..utils.trace import trace_range


class _FlatOptimizer:
    # Optimizers whose step needs a reduction over the gradient -- the layer-wise rules (FusedLAMB, FusedLARS) and
    # any optimizer built with ``clip_norm`` -- set ``_normed`` and step through :meth:`_step_normed`: a per-range
    # pass (``_pre``) as each gradient range becomes ready, then ``_post`` (seg_finalize + the applies).
    _normed = False
    clip_norm = None

    def __init__(self, flat, lr, weight_decay=0.0, wd_groups=("compute",)):
        self.flat = flat
        groups = list(flat)
        dev = groups[0].master.device if groups else torch.device("cpu")
        self.hyper = torch.tensor([float(lr), 0.0], dtype=torch.float32, device=dev)
        self.lr = float(lr)
        self.weight_decay = weight_decay
        self.wd_groups = set(wd_groups)
        self.step_count = 0
        self._sum_acc = {}  # step_sum's fp32 spill buffers (more than 8 contributions), by group name
        self._lw_plan = None  # ops/layerwise.py tables + scratch, built on the first normed step

    def new_slot(self, g, key):
        """Allocate (and initialise) group ``g``'s optimizer slot ``key`` -- also its alignment padding, which no
        checkpoint holds (a restore allocates the slots it loads through this)."""
        return g.state_buffer(key)

    def set_lr(self, lr):
        self.lr = float(lr)
        self.hyper[0].fill_(self.lr)

    def _wd(self, g):
        return self.weight_decay if g.name in self.wd_groups else 0.0

    def step(self, grad_scale=1.0, zero_grad=True, ranges=None, grads=None):
        """One optimizer step over every flat group.  ``ranges`` (DataParallel.step): a list of
        (group, lo, hi, ready) covering the groups, applied in that order, each after ``ready()`` has made the
        current stream wait for that slice's gradient (its bucket's collective) -- so the apply of the buckets
        reduced early runs while the last bucket's collective is still on the wire.  ``grads`` (the asynchronous
        PS's apply, parallel/async_ps.py): one gradient buffer per flat group, read in place of the group's own.
        The layer-wise optimizers and ``clip_norm`` take the same arguments (:meth:`_step_normed`); for them a range
        must begin and end between parameters, as DataParallel's buckets do (ValueError otherwise, before anything
        is touched)."""
        from ..parallel import overlap
        spans = None
        if self._normed and ranges is not None and grads is None:
            spans = [self._plan().span(g, lo, hi) for g, lo, hi, _ in ranges]
        overlap.join()  # side-stream weight gradients done before the apply reads them
        self.step_count += 1
        with trace_range("dtg.apply"):  # roctx range (DTG_TRACE=1)
            if self.hyper.is_cuda:
                K.hyper_tick(self.hyper)  # dtg kernel (no framework elementwise launch on the step)
            else:
                self.hyper[1].add_(1.0)
            if self._normed:
                self._step_normed(grad_scale, zero_grad, ranges, grads, spans)
            elif grads is not None:
                for g, b in zip(self.flat, grads):
                    self._apply(_Slice(g, 0, g.numel, b), grad_scale, zero_grad)
            elif ranges is None:
                for g in self.flat:
                    self._apply(g, grad_scale, zero_grad)
            else:
                for g, lo, hi, ready in ranges:
                    ready()
                    self._apply(_Slice(g, lo, hi), grad_scale, zero_grad)

    def step_sum(self, sources, grad_scale=1.0):
        """One optimizer step on the SUM of several gradient contributions (the synchronous PS's apply,
        parallel/sync_ps.py).  ``sources``: a list, in contribution order, of per-group gradient-buffer lists
        (``sources[c][i]`` is contribution c's buffer for the i-th flat group).  Same bookkeeping as :meth:`step`,
        then one k-way sum-apply kernel per group: the contributions are summed in fp32 registers, scaled by
        ``grad_scale`` and applied -- no accumulator round trip.  More than 8 contributions spill: those beyond
        the first 8 are summed into a lazily allocated fp32 buffer (``grad_sum``), which the sum-apply then takes
        with the first 8.  The group's own gradient buffer is neither read nor zeroed.  The layer-wise optimizers and
        ``clip_norm`` need norms of the summed gradient before any element is applied: they sum ALL contributions into
        the spill buffers and step on those as ``grads=``."""
        from ..parallel import overlap
        sources = [list(s) for s in sources]
        groups = list(self.flat)
        if not sources or any(len(s) != len(groups) for s in sources):
            raise ValueError("step_sum: every contribution needs one gradient buffer per flat group")
        if self._normed:
            # the trust ratios and the clip factor need the SUMMED gradient: sum every contribution into the fp32
            # spill buffers first, then step on them (they are scratch: neither zeroed nor kept)
            accs = []
            for i, g in enumerate(groups):
                acc = self._spill_acc(g)
                srcs = [s[i] for s in sources]
                for c in range(0, len(srcs), K.MAX_SRCS):
                    K.grad_sum(acc, srcs[c:c + K.MAX_SRCS], first=(c == 0))
                accs.append(acc)
            return self.step(grad_scale=grad_scale, zero_grad=False, grads=accs)
        overlap.join()
        self.step_count += 1
        with trace_range("dtg.apply_sum"):
            if self.hyper.is_cuda:
                K.hyper_tick(self.hyper)
            else:
                self.hyper[1].add_(1.0)
            for i, g in enumerate(groups):
                srcs = [s[i] for s in sources]
                acc = None
                if len(srcs) > K.MAX_SRCS:
                    acc = self._spill_acc(g)
                    rest = srcs[K.MAX_SRCS:]
                    for c in range(0, len(rest), K.MAX_SRCS):
                        K.grad_sum(acc, rest[c:c + K.MAX_SRCS], first=(c == 0))
                    srcs = srcs[:K.MAX_SRCS]
                self._apply_sum(g, srcs, grad_scale, acc)

    # ---- steps that need a norm ------------------------------------------------------------------------------
    def _plan(self):
        if self._lw_plan is None:
            self._lw_plan = L.LayerwisePlan(self.flat)
        return self._lw_plan

    def _step_normed(self, gscale, zero_grad, ranges, grads, spans):
        """items: (group, span of the chunk table, element range, gradient buffer).  With ``ranges`` the per-range
        pass is launched right after that range's ``ready()``, so it overlaps the collective tail; the chunking and
        the finalize order do not depend on the ranges, so the result is bit-identical to a whole-group step."""
        plan = self._plan()
        items = []
        if grads is not None:
            for g, b in zip(self.flat, grads):
                items.append((g, plan.span(g), (0, g.numel), b))
        elif ranges is None:
            for g in self.flat:
                items.append((g, plan.span(g), (0, g.numel), g.grad))
        else:
            for (g, lo, hi, ready), span in zip(ranges, spans):
                ready()
                items.append((g, span, (lo, hi), g.grad))
                self._pre(plan, items[-1], gscale, zero_grad)
        if grads is not None or ranges is None:
            for it in items:
                self._pre(plan, it, gscale, zero_grad)
        self._post(plan, items, gscale, zero_grad)

    def _finalize(self, plan, rule, gscale, clip=True, adapt_groups=(), eta=0.0, eps=0.0):
        L.seg_finalize(plan, rule, [g.name in adapt_groups for g in self.flat], [self._wd(g) for g in self.flat],
                       self.clip_norm if clip else None, gscale, eta, eps)

    def _pre(self, plan, item, gscale, zero_grad):
        """Clipping alone: the range's gradient sum of squares."""
        g, span, _, grad = item
        L.seg_sqnorm(plan, span, None, grad)

    def _post(self, plan, items, gscale, zero_grad):
        """Clipping alone: the clip factor, then the elementwise apply with it."""
        self._finalize(plan, L.NONE, gscale)
        for g, _, (lo, hi), grad in items:
            self._apply(_Slice(g, lo, hi, grad), gscale, zero_grad, clip=plan.cfac)

    def _apply(self, g, gscale, zero_grad, clip=None):
        """The elementwise apply of one group or slice.  The layer-wise optimizers have none: their step size depends
        on the parameter an element belongs to (``_pre`` / ``_post``)."""
        raise NotImplementedError("%s has no elementwise apply" % type(self).__name__)

    def _spill_acc(self, g):
        if g.name not in self._sum_acc:
            self._sum_acc[g.name] = torch.empty_like(g.master)  # grad_sum(first=True) never reads it
        return self._sum_acc[g.name]

    def minimize(self, loss_fn, global_step=None, inputs=(), name=None, accum_steps=1):
        """A train op for dtg sessions (``sess.run(op, feed_dict)``): forward + backward of ``loss_fn(*inputs)``,
        this optimizer's fused apply, global_step += 1, on one replica (train/eager.py; for several ranks wrap it
        in ``dtg.train.SyncReplicasOptimizer``, the all-reduce mode).  ``accum_steps``: micro-batches per step
        (gradient accumulation, parallel/accum.py)."""
        from ..train.eager import minimize
        return minimize(self, loss_fn, global_step, inputs, None, name, accum_steps)

    def state_dict(self):
        return {"step": self.step_count, "lr": self.lr,
                "state": {g.name: {k: v for k, v in g.state.items()} for g in self.flat}}

    def load_state_dict(self, sd):
        self.step_count = int(sd.get("step", 0))
        self.set_lr(sd.get("lr", self.lr))
        self.hyper[1].fill_(float(self.step_count))
        for g in self.flat:
            for k, v in sd.get("state", {}).get(g.name, {}).items():
                g.state_buffer(k).copy_(v)


class _Slice:
    """A contiguous element range [lo, hi) of a flat group, with the group's name / buffers sliced alike (the
    fused applies are elementwise, so applying a group slice by slice is bit-identical to applying it whole).
    ``grad``: a buffer of the group's layout to take the gradient from instead of the group's own."""

    def __init__(self, g, lo, hi, grad=None):
        self._g, self.lo, self.hi = g, lo, hi
        self.name = g.name
        self.master = g.master[lo:hi]
        self.grad = (g.grad if grad is None else grad)[lo:hi]
        self.mirror = g.mirror[lo:hi] if g.mirror is not None else None
        self.state = g.state

    def state_buffer(self, key):
        return self._g.state_buffer(key)[self.lo:self.hi]


class FusedSGD(_FlatOptimizer):
    """Momentum SGD (PyTorch semantics, optional Nesterov); momentum=0 -> plain SGD."""

    def __init__(self, flat, lr, momentum=0.9, weight_decay=0.0, nesterov=False, wd_groups=("compute",),
                 clip_norm=None):
        super().__init__(flat, lr, weight_decay, wd_groups)
        self.momentum = momentum
        self.nesterov = nesterov
        self.clip_norm = _check_clip(clip_norm)
        self._normed = clip_norm is not None

    def _apply(self, g, gscale, zero_grad, clip=None):
        if self.momentum == 0.0:
            K.sgd(g.master, g.grad, self.hyper, g.mirror, self._wd(g), gscale, zero_grad, clip)
        else:
            K.momentum(g.master, g.grad, g.state_buffer("momentum"), self.hyper, g.mirror, self.momentum,
                       self._wd(g), self.nesterov, gscale, zero_grad, clip)

    def _apply_sum(self, g, srcs, gscale, acc):
        if self.momentum == 0.0:
            K.sgd_sum(g.master, srcs, self.hyper, g.mirror, self._wd(g), gscale, acc)
        else:
            K.momentum_sum(g.master, srcs, g.state_buffer("momentum"), self.hyper, g.mirror, self.momentum,
                           self._wd(g), self.nesterov, gscale, acc)


class FusedAdam(_FlatOptimizer):
    """AdamW with decoupled weight decay (BERT pre-training)."""

    def __init__(self, flat, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, wd_groups=("compute",),
                 clip_norm=None):
        super().__init__(flat, lr, weight_decay, wd_groups)
        self.betas = betas
        self.eps = eps
        self.clip_norm = _check_clip(clip_norm)
        self._normed = clip_norm is not None

    def _apply(self, g, gscale, zero_grad, clip=None):
        K.adam(g.master, g.grad, g.state_buffer("m"), g.state_buffer("v"), self.hyper, g.mirror, self.betas[0],
               self.betas[1], self.eps, self._wd(g), gscale, zero_grad, clip)

    def _apply_sum(self, g, srcs, gscale, acc):
        K.adam_sum(g.master, srcs, g.state_buffer("m"), g.state_buffer("v"), self.hyper, g.mirror, self.betas[0],
                   self.betas[1], self.eps, self._wd(g), gscale, acc)


class FusedAdagrad(_FlatOptimizer):
    """TF-style Adagrad (initial accumulator 0.1, no epsilon) -- DOWNPOUR's optimizer."""

    def __init__(self, flat, lr, initial_accumulator_value=0.1, eps=0.0):
        super().__init__(flat, lr, 0.0)
        self.init_acc = initial_accumulator_value
        self.eps = eps

    def new_slot(self, g, key):
        fresh = key not in g.state
        buf = g.state_buffer(key)
        if fresh and key == "acc":
            buf.fill_(self.init_acc)
        return buf

    def _acc(self, g):
        # the WHOLE group's accumulator is created and filled with the initial value on first use: DataParallel.step
        # applies a group slice by slice (_Slice shares the group's state dict), so a per-slice "fresh" test would
        # fill only the first slice and leave later slices at the allocator's zeros (lr * sign(g), or 0/0)
        full = g._g if isinstance(g, _Slice) else g
        if "acc" not in full.state:
            self.new_slot(full, "acc")
        return g.state_buffer("acc")

    def _apply(self, g, gscale, zero_grad):
        K.adagrad(g.master, g.grad, self._acc(g), self.hyper, g.mirror, self.eps, gscale, zero_grad)

    def _apply_sum(self, g, srcs, gscale, acc):
        # _acc: the whole group's accumulator starts at the initial value here too
        K.adagrad_sum(g.master, srcs, self._acc(g), self.hyper, g.mirror, self.eps, gscale, acc)


class FusedLAMB(_FlatOptimizer):
    """LAMB (You et al., "Large Batch Optimization for Deep Learning", 2019): AdamW's update u scaled per
    parameter by the trust ratio ||w|| / ||u||, for the groups in ``adapt_groups`` (r = 1 elsewhere and where a
    norm is 0).  ``clip_norm``: the gradient is first clipped to that global norm (tf.clip_by_global_norm, the
    BERT recipe's 1.0).  Two streaming passes per group (moments + norms, apply) around one seg_finalize; state is
    ``m`` and ``v`` as for FusedAdam."""
    _normed = True

    def __init__(self, flat, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, wd_groups=("compute",),
                 adapt_groups=("compute",), clip_norm=None):
        super().__init__(flat, lr, weight_decay, wd_groups)
        self.betas = betas
        self.eps = eps
        self.adapt_groups = set(adapt_groups)
        self.clip_norm = _check_clip(clip_norm)

    def _moments(self, plan, item, gscale, zero_grad):
        g, span, _, grad = item
        L.lamb_moments(plan, span, g.master, grad, g.state_buffer("m"), g.state_buffer("v"), self.hyper,
                       self.betas[0], self.betas[1], self.eps, self._wd(g), gscale, self.clip_norm is not None,
                       zero_grad)

    def _pre(self, plan, item, gscale, zero_grad):
        if self.clip_norm is None:
            self._moments(plan, item, gscale, zero_grad)  # g^ needs no global norm: the moments pass goes first
        else:
            L.seg_sqnorm(plan, item[1], None, item[3])

    def _post(self, plan, items, gscale, zero_grad):
        if self.clip_norm is not None:
            self._finalize(plan, L.NONE, gscale)
            for it in items:
                self._moments(plan, it, gscale, zero_grad)
        self._finalize(plan, L.LAMB, gscale, clip=False, adapt_groups=self.adapt_groups)
        for g, span, _, _ in items:
            L.lamb_apply(plan, span, g.master, g.mirror, g.state_buffer("m"), g.state_buffer("v"), self.hyper,
                         self.betas[0], self.betas[1], self.eps, self._wd(g))


class FusedLARS(_FlatOptimizer):
    """LARS (You et al., "Large Batch Training of Convolutional Networks", 2017) with momentum:
    m = mu * m + lr * r * (g + wd * w), w -= m, r = eta * ||w|| / (||g|| + wd * ||w|| + eps) per parameter of the
    groups in ``adapt_groups`` (r = 1 elsewhere and where a norm is 0).  One norm pass and one apply pass per group
    around one seg_finalize; state is ``momentum`` as for FusedSGD."""
    _normed = True

    def __init__(self, flat, lr, momentum=0.9, weight_decay=5e-5, eta=0.001, eps=0.0, wd_groups=("compute",),
                 adapt_groups=("compute",), clip_norm=None):
        super().__init__(flat, lr, weight_decay, wd_groups)
        self.momentum = momentum
        self.eta = eta
        self.eps = eps
        self.adapt_groups = set(adapt_groups)
        self.clip_norm = _check_clip(clip_norm)

    def _pre(self, plan, item, gscale, zero_grad):
        g, span, _, grad = item
        L.seg_sqnorm(plan, span, g.master, grad)

    def _post(self, plan, items, gscale, zero_grad):
        self._finalize(plan, L.LARS, gscale, adapt_groups=self.adapt_groups, eta=self.eta, eps=self.eps)
        for g, span, _, grad in items:
            L.lars_apply(plan, span, g.master, g.mirror, grad, g.state_buffer("momentum"), self.hyper, self.momentum,
                         self._wd(g), gscale, self.clip_norm is not None, zero_grad)


def _check_clip(clip_norm):
    if clip_norm is not None and not float(clip_norm) > 0.0:
        raise ValueError("clip_norm must be positive or None, got %r" % (clip_norm,))
    return None if clip_norm is None else float(clip_norm)


def make_optimizer(kind, flat, lr, **kw):
    """A fused flat optimizer by name, for the CLI flags of the async-PS examples and bench (``--local_opt``,
    ``--ps_opt``): ``sgd`` plain SGD (TF GradientDescentOptimizer, ADAG's local and global rule), ``momentum``
    momentum 0.9 SGD, ``adagrad`` TF Adagrad with initial accumulator 0.1 (DOWNPOUR's local and global rule,
    /root/reference/DOWNPOUR/DOWNPOUR.py:57, :92), ``adam`` AdamW.  ``none`` returns None."""
    if kind in (None, "none"):
        return None
    if kind == "sgd":
        return FusedSGD(flat, lr=lr, momentum=0.0)
    if kind == "momentum":
        return FusedSGD(flat, lr=lr, momentum=kw.get("momentum", 0.9), weight_decay=kw.get("weight_decay", 0.0))
    if kind == "adagrad":
        return FusedAdagrad(flat, lr=lr)
    if kind == "adam":
        return FusedAdam(flat, lr=lr, weight_decay=kw.get("weight_decay", 0.01))
    # the layer-wise adaptive rules for large batches (``clip_norm`` is passed on)
    if kind == "lamb":
        return FusedLAMB(flat, lr=lr, weight_decay=kw.get("weight_decay", 0.01), clip_norm=kw.get("clip_norm"))
    if kind == "lars":
        return FusedLARS(flat, lr=lr, momentum=kw.get("momentum", 0.9), weight_decay=kw.get("weight_decay", 5e-5),
                         clip_norm=kw.get("clip_norm"))
    raise ValueError("unknown optimizer %r (sgd, momentum, adagrad, adam, lamb, lars, none)" % (kind,))
