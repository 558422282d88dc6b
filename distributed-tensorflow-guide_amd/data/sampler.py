"""Deterministic sharded sampler: which records a rank reads at a global step, as a pure function of the step.

Epoch ``e``'s order is the stable argsort of one 32-bit hash key per record index (the murmur3 finalizer that
``ops/transformer.py::_fmix32`` mirrors, over (index, seed, e); ties break by index).  Global batch ``b`` of the epoch
is ``perm[b*G : (b+1)*G]`` with ``G = batch * world`` and rank ``r`` takes ``[r*batch : (r+1)*batch]`` of it, so
``world`` ranks x ``batch`` read exactly the global batch of one rank x ``world * batch``, in rank-major order.  The
last partial global batch of an epoch is dropped.  There is no state to checkpoint: resuming is
``at(restored_global_step)``.

``EvalSampler`` is the evaluation pass: in order, nothing dropped, the last global batch padded.
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def fmix32(h):
    """murmur3's 32-bit finalizer on a uint64 array holding 32-bit values (ops/transformer.py::_fmix32)."""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    return h ^ (h >> np.uint64(16))


def hash32(*words):
    """One 32-bit hash of a tuple of integer words (scalars or arrays, broadcast): a chain of finalizer rounds,
    each word entering through an odd multiplier.  Returned as uint64 holding 32-bit values."""
    h = np.uint64(0x9E3779B9)
    for w in words:
        w = np.asarray(w).astype(np.uint64) & _M32
        h = fmix32((h ^ ((w * np.uint64(0x9E3779B1)) & _M32)) & _M32)
        h = (h * np.uint64(5) + np.uint64(0xE6546B64)) & _M32
    return fmix32(h)


class ShardedSampler:
    def __init__(self, n, batch, world=1, rank=0, seed=0, shuffle=True):
        if batch < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("ShardedSampler: batch >= 1, world >= 1 and 0 <= rank < world required")
        if n < batch * world:
            raise ValueError("ShardedSampler: %d records do not fill one global batch of %d x %d" % (n, batch, world))
        self.n, self.batch, self.world, self.rank, self.seed, self.shuffle = n, batch, world, rank, seed, shuffle
        self.steps_per_epoch = n // (batch * world)
        self._perm = (None, None)  # (epoch, permutation): the one epoch in use

    def permutation(self, epoch):
        if self._perm[0] != epoch:
            idx = np.arange(self.n, dtype=np.int64)
            perm = np.argsort(hash32(idx, self.seed, epoch), kind="stable") if self.shuffle else idx
            self._perm = (epoch, perm.astype(np.int64))
        return self._perm[1]

    def at(self, step):
        """Global step -> (epoch, this rank's record indices int64 [batch])."""
        if step < 0:
            raise ValueError("negative step")
        epoch, b = divmod(int(step), self.steps_per_epoch)
        lo = (b * self.world + self.rank) * self.batch
        return epoch, self.permutation(epoch)[lo:lo + self.batch].copy()

    def __iter__(self):
        step = 0
        while True:
            yield self.at(step)
            step += 1


class EvalSampler:
    """Every record exactly once, in order: ``steps = ceil(n / (batch * world))`` on every rank.  Global batch ``b`` is
    records ``[b*G, min(n, (b+1)*G))`` with ``G = batch * world`` and rank ``r`` takes its ``batch``-sized slice of it; a
    short (or empty) slice is padded by repeating index 0 and ``at`` reports how many leading entries are real.
    ``n < batch * world`` is allowed."""

    def __init__(self, n, batch, world=1, rank=0):
        if n < 1 or batch < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("EvalSampler: n >= 1, batch >= 1, world >= 1 and 0 <= rank < world required")
        self.n, self.batch, self.world, self.rank = n, batch, world, rank
        self.steps = self.steps_per_epoch = -(-n // (batch * world))

    def at(self, step):
        """Step in [0, steps) -> (this rank's record indices int64 [batch], valid): the first ``valid`` are records,
        the rest padding."""
        step = int(step)
        if not 0 <= step < self.steps:
            raise ValueError("EvalSampler: step %d outside [0, %d)" % (step, self.steps))
        lo = (step * self.world + self.rank) * self.batch
        valid = max(0, min(self.n, lo + self.batch) - lo)
        idx = np.zeros(self.batch, dtype=np.int64)
        idx[:valid] = np.arange(lo, lo + valid, dtype=np.int64)
        return idx, valid
