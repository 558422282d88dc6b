"""The prefetch ring that every loader shares: record shards -> pinned ring -> device -> one launch per batch.

A ring of ``depth`` slots; each slot holds the pinned host tensors its loader names and their device twins.  One
producer thread runs steps ``s, s+1, ...``: sampler, the loader's host fill (native GIL-free gathers into the slot,
validation), host->device copies on the ring's own copy stream, an event after the copies.  ``next()`` makes the
current stream wait for that event, has the loader launch its kernel on it into fresh output tensors and records the
slot's "consumed" event; the producer reuses a slot only once that event has completed (it waits on the event, never
on the device).  The slots outlive a ``seek``, so a slot whose last kernel has not run is still waited for after it.

On the CPU the interface is the same, with the loader's PyTorch mirror as the kernel and no streams or events.

A loader is a subclass that gives ``_thread_name`` and three methods: ``_layout()`` (validate the record fields ->
the slot's [(shape, dtype)]), ``_host_fill(slot, epoch, idx, valid)`` and ``_consume(slot, tensors)``.
"""
import atexit
import queue
import threading
import time
import weakref

import torch

from .records import ShardSet
from .sampler import EvalSampler, ShardedSampler


class _Slot:
    """``host``: the pinned tensors of the layout; on CUDA ``dev``: their device twins, and the two events.  A
    loader's host fill may set further per-step attributes."""

    def __init__(self, layout, device):
        cuda = device.type == "cuda"
        self.host = tuple(torch.empty(shape, dtype=dtype, pin_memory=cuda) for shape, dtype in layout)
        if cuda:
            self.dev = tuple(torch.empty_like(t, device=device) for t in self.host)
            self.ready = torch.cuda.Event()
        self.consumed = None  # recorded by next() after the slot's kernel; None: never used


def _close_ref(ref):
    obj = ref()
    if obj is not None:
        obj.close()


class PrefetchRing:
    _thread_name = None

    def __init__(self, shards, batch, device, world, rank, seed, train, depth, threads, drop_last):
        """drop_last=False (evaluation only, ``train=False``): one pass of ``steps_per_epoch`` steps visits every
        record exactly once over the ranks (EvalSampler); the rows that pad the last batches repeat record 0."""
        self.shards = shards if isinstance(shards, ShardSet) else ShardSet(shards)
        if depth < 1 or not 1 <= threads <= 64:
            raise ValueError("depth >= 1 and 1 <= threads <= 64 required")
        if not drop_last and train:
            raise ValueError("drop_last=False is the evaluation pass: it requires train=False")
        self.batch, self.train, self.threads, self.drop_last = batch, train, threads, drop_last
        self.device = torch.device(device)
        self._cuda = self.device.type == "cuda"
        layout = self._layout()
        self.sampler = ShardedSampler(len(self.shards), batch, world, rank, seed, shuffle=train) if drop_last else \
            EvalSampler(len(self.shards), batch, world, rank)
        self.steps_per_epoch = self.sampler.steps_per_epoch
        if self._cuda:
            self._copy_stream = torch.cuda.Stream(self.device)
        self._slots = [_Slot(layout, self.device) for _ in range(depth)]
        from .. import _runtime
        self._gather = _runtime.gather_rows
        self._thread = None
        self._step = 0  # the step next() returns next
        self.batches = self.waits = 0
        self.wait_ms = self.gather_ms = self.reuse_wait_ms = 0.0
        self._closed = False
        atexit.register(_close_ref, weakref.ref(self))

    # ---- what a loader gives ------------------------------------------------------------------------------
    def _layout(self):
        """Validate the record fields -> [(shape, dtype)] of one slot's host tensors."""
        raise NotImplementedError

    def _host_fill(self, slot, epoch, idx, valid):
        """Fill ``slot.host`` with the records ``idx`` (``_gather_rows``), validate them and mark the padding rows
        ``valid:``; runs on the producer thread and touches no device."""
        raise NotImplementedError

    def _consume(self, slot, tensors):
        """Launch the batch's kernel on ``tensors`` (``slot.dev`` on CUDA, on the current stream; ``slot.host`` on
        the CPU) into fresh tensors -> what ``next()`` returns.  Nothing returned may alias the slot."""
        raise NotImplementedError

    # ---- producer -----------------------------------------------------------------------------------------
    def _gather_rows(self, dst, field, idx, threads=1):
        t0 = time.perf_counter()
        self._gather(dst.data_ptr(), self.shards.addresses(field, idx), self.shards.row_bytes(field), threads)
        self.gather_ms += (time.perf_counter() - t0) * 1e3

    def _fill(self, slot, step):
        if self.drop_last:
            epoch, idx = self.sampler.at(step)
            valid = len(idx)
        else:
            epoch, (idx, valid) = 0, self.sampler.at(step)
        self._host_fill(slot, epoch, idx, valid)
        if self._cuda:
            with torch.cuda.stream(self._copy_stream):
                for d, h in zip(slot.dev, slot.host):
                    d.copy_(h, non_blocking=True)
                slot.ready.record(self._copy_stream)

    def _produce(self, step, free_q, ready_q, stop):
        try:
            if self._cuda:
                torch.cuda.set_device(self.device)
            while True:
                slot = free_q.get()
                if slot is None or stop.is_set():
                    return
                if not self.drop_last and step >= self.steps_per_epoch:
                    return  # the evaluation pass is over
                if slot.consumed is not None:
                    t0 = time.perf_counter()
                    slot.consumed.synchronize()  # this slot's last kernel has read its device buffers
                    self.reuse_wait_ms += (time.perf_counter() - t0) * 1e3
                self._fill(slot, step)
                ready_q.put((step, slot))
                step += 1
        except BaseException as e:  # noqa: BLE001 - handed to the consumer
            ready_q.put((e, None))

    def _start(self, step):
        self._free_q, self._ready_q, self._stop = queue.Queue(), queue.Queue(), threading.Event()
        for s in self._slots:  # with their ``consumed`` events: a slot's last kernel is waited for across a seek
            self._free_q.put(s)
        self._step = step
        self._thread = threading.Thread(target=self._produce, args=(step, self._free_q, self._ready_q, self._stop),
                                        name=self._thread_name, daemon=True)
        self._thread.start()

    def _halt(self):
        if self._thread is not None:
            self._stop.set()
            self._free_q.put(None)
            self._thread.join()
            self._thread = None

    # ---- consumer -----------------------------------------------------------------------------------------
    @property
    def step(self):
        return self._step

    def seek(self, step):
        """Discard what was prefetched and restart production at ``step``."""
        if self._closed:
            raise RuntimeError("%s is closed" % type(self).__name__)
        self._halt()
        self._start(int(step))

    def next(self):
        """-> the batch of step ``self.step`` (the loader's ``_consume``); advances the step."""
        if self._closed:
            raise RuntimeError("%s is closed" % type(self).__name__)
        if not self.drop_last and self._step >= self.steps_per_epoch:
            raise StopIteration  # one evaluation pass; seek(0) starts the next
        if self._thread is None:
            self._start(self._step)
        try:
            step, slot = self._ready_q.get_nowait()
        except queue.Empty:  # the producer is behind
            t0 = time.perf_counter()
            step, slot = self._ready_q.get()
            self.waits += 1
            self.wait_ms += (time.perf_counter() - t0) * 1e3
        if slot is None:
            self._halt()
            raise RuntimeError("%s: the producer thread failed" % type(self).__name__) from step
        assert step == self._step, (step, self._step)
        if self._cuda:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(slot.ready)
            out = self._consume(slot, slot.dev)
            slot.consumed = torch.cuda.Event()
            slot.consumed.record(cur)
        else:
            out = self._consume(slot, slot.host)
        self._free_q.put(slot)
        self._step += 1
        self.batches += 1
        return out

    __next__ = next

    def __iter__(self):
        return self

    def counters(self):
        """batches; waits / wait_ms: how often and how long next() blocked on the producer; gather_ms: the host
        gathers; reuse_wait_ms: how long the producer itself waited for the device to release a slot.  A host that
        runs ahead of the device is held to ``depth`` batches, so waits with a large reuse_wait_ms are back-pressure
        from the device, not a slow producer."""
        return {"batches": self.batches, "waits": self.waits, "wait_ms": self.wait_ms, "gather_ms": self.gather_ms,
                "reuse_wait_ms": self.reuse_wait_ms}

    def close(self):
        """Stop and join the producer thread (idempotent)."""
        if not self._closed:
            self._closed = True
            self._halt()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class FeedHook:
    """Session hook that feeds placeholders from a loader.  The batch is a function of the global step:
    ``after_create_session`` seeks the loader to the session's (possibly restored) step, ``before_run`` feeds the
    batch of the current step -- the same one again while the step has not advanced, so a run that only reads a
    variable consumes nothing -- and ``end`` closes the loader.  A subclass gives ``_feed(batch) -> feed dict``,
    called before every run with what the loader's ``next()`` returned for the step."""

    def __init__(self, loader, global_step):
        self._loader, self._gs = loader, global_step
        self._fed = None  # (step, batch)

    def _feed(self, batch):
        raise NotImplementedError

    def begin(self):
        pass

    def after_create_session(self, session, coord):
        self._fed = None
        self._loader.seek(int(session._read(self._gs)))

    def before_run(self, run_context):
        from ..train.hooks import SessionRunArgs
        step = int(run_context.session._read(self._gs))
        if self._fed is None or self._fed[0] != step:
            if self._loader.step != step:
                self._loader.seek(step)
            self._fed = (step, self._loader.next())
        return SessionRunArgs(fetches=None, feed_dict=self._feed(self._fed[1]))

    def after_run(self, run_context, run_values):
        pass

    def end(self, session):
        self._loader.close()
