"""Gradient accumulation over micro-batches with an fp32 accumulator.

One optimizer step on the gradient of ``A`` micro-batches, each run through its own forward and backward, so a card
steps at ``A`` times the batch its memory holds (the batch sizes LAMB / LARS exist for)::

    acc = GradAccumulator(flat, steps=A, dp=dp)
    for xb, yb in micro_batches:            # A of them
        acc.begin()
        loss_fn(model(xb), yb).backward()
        acc.end()
    acc.step(opt)                           # opt on cast(sum_i float(g_i)) * grad_scale / A

Not zeroing the flat gradient between the backwards would sum in the gradient's dtype: the compute group's buffer is
bf16 and the weight-gradient kernels add into it (parallel/grad_sink.py), so the running sum would be rounded to 8
mantissa bits at every add.  Instead every group gets one lazily allocated fp32 accumulator with the master's layout:

* after each of the micro-steps ``0 .. A-2``, ``end()`` folds the group's gradient into it and zeroes the gradient in
  one launch (``grad_fold``; the first fold of a window overwrites, so the accumulator is never filled and nothing an
  abandoned window left in it can leak).  Every backward therefore starts from a zeroed gradient buffer, as without
  accumulation, and the fp32 group is folded like the compute group: no op has to be audited for add-versus-overwrite;
* the last micro-step's gradient stays in the flat buffer and the accumulator is added onto it (``grad_unfold``): the
  flat gradient then holds the sum of the ``A`` micro-gradients, rounded ONCE to its dtype -- the precision class of
  one large batch's weight gradient.  From there the bucketed all-reduce, the per-bucket applies, the LAMB / LARS /
  clip norms and the apply's zero_grad run the code they run without accumulation, with the gradient scale times 1/A.

With a :class:`~dtg.parallel.DataParallel`, the micro-steps ``0 .. A-2`` launch no collective (its ``_comm`` gate), and
on the last one each bucket is unfolded right before its all-reduce is enqueued, on the stream that enqueues it
(``DataParallel._pre_launch``).  Without one -- or where it registers no hooks -- whole groups are unfolded in
:meth:`step`.  BatchNorm normalises each micro-batch with its own statistics and updates the running statistics per
micro-batch: what ``A`` data-parallel ranks do.  The optimizer's step count moves once per window.

``steps=1`` is the plain path: nothing is allocated, no kernel is added, ``dp`` is not touched.

A window is not capturable in a hipGraph (its micro-steps differ: ``first``, the collectives' gate): ``begin()`` under
capture and ``GraphedStep`` around an accumulating step raise.
"""
import torch

from . import overlap
from ..ops import optim_kernels as K


class GradAccumulator:
    def __init__(self, flat, steps, dp=None):
        steps = int(steps)
        if steps < 1:
            raise ValueError("accumulation steps must be >= 1, got %d" % steps)
        self.flat, self.steps, self.dp = flat, steps, dp
        self.acc = {}          # group name -> fp32 accumulator (allocated by the first fold)
        self._micro = 0        # micro-steps of the open window that have ended
        self._open = False     # between begin() and end()
        self._comm = None      # dp's own collective gate, saved while the window holds it closed
        self._unfolded = set()  # indices of the buckets unfolded in this window
        if steps > 1 and dp is not None:
            if getattr(dp, "_pre_launch", None) is not None:
                raise RuntimeError("this DataParallel already serves another GradAccumulator")
            dp._pre_launch = self._on_launch

    @property
    def micro(self):
        """Position in the window: the number of micro-steps ended since the last :meth:`step` (0 .. steps)."""
        return self._micro

    # -- one micro-batch ----------------------------------------------------------------------------------------
    def begin(self):
        if self.steps == 1:
            return
        if _capturing():
            raise RuntimeError("gradient accumulation (steps=%d) cannot be captured in a hipGraph: the micro-steps of "
                               "a window differ; run the accumulating step eagerly" % self.steps)
        if self._open or self._micro >= self.steps:
            raise RuntimeError("begin(): %s" % ("the previous micro-step has not ended" if self._open else
                                                "the window is complete, call step()"))
        self._open = True
        dp = self.dp
        if dp is not None:
            if self._micro == 0:
                self._comm = dp._comm
            # hooks keep counting, but only the last micro-step's backward launches collectives
            dp._comm = self._comm and self._micro == self.steps - 1

    def end(self):
        if self.steps == 1:
            return
        if not self._open:
            raise RuntimeError("end() without begin()")
        self._open = False
        if self._micro < self.steps - 1:
            overlap.join()  # side-stream weight gradients land before the fold reads them
            for g in self.flat:
                K.grad_fold(self._acc(g), g.grad, self._micro == 0)
            if self.dp is not None:
                self.dp._reset()
        self._micro += 1

    # -- closing the window ---------------------------------------------------------------------------------------
    def step(self, opt, zero_grad=True):
        """The optimizer step of the window: ``dp.step(opt)`` or ``opt.step()`` with the gradient scale times
        1 / steps."""
        dp = self.dp
        if self.steps == 1:
            return dp.step(opt, zero_grad=zero_grad) if dp is not None else opt.step(zero_grad=zero_grad)
        if self._open or self._micro != self.steps:
            raise RuntimeError("step() after %d of %d micro-steps" % (self._micro, self.steps))
        inv = 1.0 / self.steps
        try:
            if dp is None or not dp._comm or (dp.world == 1 and not dp._force):
                # no bucket is launched (no DataParallel, collectives off, or one rank without hooks)
                overlap.join()
                for g in self.flat:
                    K.grad_unfold(g.grad, self._acc(g), 0, g.numel)
                if dp is None:
                    return opt.step(grad_scale=inv, zero_grad=zero_grad)
            # buckets still waiting are launched -- and unfolded by _on_launch -- inside dp.step
            return dp.step(opt, zero_grad=zero_grad, scale=inv)
        finally:
            self._close()

    def reset(self):
        """Abandon the window: what was accumulated is dropped (the next window's first fold overwrites it) and the
        flat gradient is zeroed, so the next backward starts clean."""
        if self.steps == 1:
            return
        overlap.join()
        for g in self.flat:
            g.zero_grad()
        if self.dp is not None:
            self.dp._reset()
        self._close()

    def _close(self):
        if self.dp is not None and self._comm is not None:
            self.dp._comm = self._comm
        self._comm = None
        self._micro = 0
        self._open = False
        self._unfolded.clear()

    def _acc(self, g):
        a = self.acc.get(g.name)
        if a is None:
            a = self.acc[g.name] = torch.empty_like(g.master)  # grad_fold(first=True) never reads it
        return a

    def _on_launch(self, b):
        """DataParallel._launch, on the launching stream, before bucket ``b``'s all-reduce is enqueued."""
        if self._micro < self.steps - 1 or b.index in self._unfolded:
            return
        self._unfolded.add(b.index)
        K.grad_unfold(b.group.grad, self._acc(b.group), b.start, b.end)

    def detach(self):
        """Give the DataParallel back (its launches call nothing of this accumulator's any more)."""
        if self.dp is not None and getattr(self.dp, "_pre_launch", None) == self._on_launch:
            self.dp._pre_launch = None


def _capturing():
    from . import graphs
    return graphs._IN_CAPTURE or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())


def find_accumulating(fn):
    """A GradAccumulator with steps > 1 that the callable ``fn`` reaches -- ``fn`` itself, its ``__self__`` or a
    closure cell, or the ``accum`` attribute of one of those (the train ops of train/eager.py carry theirs) -- or
    None."""
    cand = [fn, getattr(fn, "__self__", None)]
    cand += [c.cell_contents for c in (getattr(fn, "__closure__", None) or ()) if _has_contents(c)]
    for o in cand:
        for a in (o, getattr(o, "accum", None)):
            if isinstance(a, GradAccumulator) and a.steps > 1:
                return a
    return None


def _has_contents(cell):
    try:
        cell.cell_contents
        return True
    except ValueError:
        return False
