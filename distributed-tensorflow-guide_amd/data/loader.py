"""Prefetching loader: record shards -> pinned ring -> device -> one augmentation launch per batch.

A ring of ``depth`` slots; each slot holds a pinned raw-image buffer ``[batch, H, W, 3]``, a pinned parameter table
and a pinned label buffer, and their device twins.  One producer thread runs steps ``s, s+1, ...``: sampler,
augmentation parameters (made and validated on the host), native GIL-free gather into the slot, host->device copies
on the loader's own copy stream, an event after the copies.  ``next()`` makes the current stream wait for that
event, launches ``crop_resize_norm`` on it into a fresh output tensor and records the slot's "consumed" event; the
producer reuses a slot only once that event has completed (it waits on the event, never on the device).

On the CPU the interface is the same, with the PyTorch mirror as the augmentation and no streams.
"""
import atexit
import queue
import threading
import time
import weakref

import torch

from ..ops.augment import IMAGENET_MEAN, IMAGENET_STD, crop_resize_norm, norm_constants
from .augment_params import eval_params, train_params, validate_params
from .records import ShardSet
from .sampler import EvalSampler, ShardedSampler


class _Slot:
    def __init__(self, batch, H, W, device):
        cuda = device.type == "cuda"
        self.raw = torch.empty((batch, H, W, 3), dtype=torch.uint8, pin_memory=cuda)
        self.params = torch.empty((batch, 5), dtype=torch.int32, pin_memory=cuda)
        self.labels = torch.empty((batch,), dtype=torch.int64, pin_memory=cuda)
        self.indices = None
        if cuda:
            self.d_raw = torch.empty_like(self.raw, device=device)
            self.d_params = torch.empty_like(self.params, device=device)
            self.d_labels = torch.empty_like(self.labels, device=device)
            self.ready = torch.cuda.Event()
        self.consumed = None  # recorded by next() after the slot's kernel; None: never used


def _close_ref(ref):
    obj = ref()
    if obj is not None:
        obj.close()


class DeviceLoader:
    def __init__(self, shards, batch, S, device, world=1, rank=0, seed=0, train=True, depth=3, threads=4,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD, image_field="image", label_field="label",
                 dtype=torch.bfloat16, drop_last=True):
        """dtype: what ``next()`` returns the images as (the kernel writes bf16; another dtype is a cast of that,
        for fp32 CPU models).  drop_last=False (evaluation only, ``train=False``): one pass of ``steps_per_epoch``
        steps visits every record exactly once over the ranks (EvalSampler); the rows that pad the last batches
        repeat record 0 and carry label -1, which the loss and the metric kernels ignore."""
        self.shards = shards if isinstance(shards, ShardSet) else ShardSet(shards)
        fields = self.shards.fields
        dt, shape = fields[image_field]
        if dt != "uint8" or len(shape) != 3 or shape[2] != 3:
            raise ValueError("field %r must be uint8 [H, W, 3], got %s %s" % (image_field, dt, shape))
        if fields[label_field] != ("int64", ()):
            raise ValueError("field %r must be int64 []" % label_field)
        if depth < 1 or not 1 <= threads <= 64:
            raise ValueError("depth >= 1 and 1 <= threads <= 64 required")
        self.H, self.W = shape[0], shape[1]
        self.batch, self.S, self.seed, self.train, self.threads = batch, S, seed, train, threads
        self.device = torch.device(device)
        self._cuda = self.device.type == "cuda"
        self._image, self._label, self._dtype = image_field, label_field, dtype
        if not drop_last and train:
            raise ValueError("drop_last=False is the evaluation pass: it requires train=False")
        self.drop_last = drop_last
        self.sampler = ShardedSampler(len(self.shards), batch, world, rank, seed, shuffle=train) if drop_last else \
            EvalSampler(len(self.shards), batch, world, rank)
        self.steps_per_epoch = self.sampler.steps_per_epoch
        self.scale, self.shift = norm_constants(mean, std)
        if self._cuda:
            self._d_scale, self._d_shift = self.scale.to(self.device), self.shift.to(self.device)
            self._copy_stream = torch.cuda.Stream(self.device)
        self._slots = [_Slot(batch, self.H, self.W, self.device) for _ in range(depth)]
        from .. import _runtime
        self._gather = _runtime.gather_rows
        self._thread = None
        self._step = 0  # the step next() returns next
        self.batches = self.waits = 0
        self.wait_ms = self.gather_ms = self.reuse_wait_ms = 0.0
        self._closed = False
        atexit.register(_close_ref, weakref.ref(self))

    # ---- producer -----------------------------------------------------------------------------------------
    def _fill(self, slot, step):
        if self.drop_last:
            epoch, idx = self.sampler.at(step)
            valid = len(idx)
        else:
            epoch, (idx, valid) = 0, self.sampler.at(step)
        p = train_params(idx, epoch, self.seed, self.H, self.W) if self.train else \
            eval_params(len(idx), self.H, self.W)
        validate_params(p, self.H, self.W)
        t0 = time.perf_counter()
        self._gather(slot.raw.data_ptr(), self.shards.addresses(self._image, idx),
                     self.shards.row_bytes(self._image), self.threads)
        self._gather(slot.labels.data_ptr(), self.shards.addresses(self._label, idx), 8, 1)
        self.gather_ms += (time.perf_counter() - t0) * 1e3
        if valid < len(idx):
            slot.labels[valid:] = -1  # padding rows: ignored by the loss and the metrics
        slot.params.copy_(torch.from_numpy(p))
        slot.indices = idx
        if self._cuda:
            with torch.cuda.stream(self._copy_stream):
                slot.d_raw.copy_(slot.raw, non_blocking=True)
                slot.d_params.copy_(slot.params, non_blocking=True)
                slot.d_labels.copy_(slot.labels, non_blocking=True)
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
        for s in self._slots:
            self._free_q.put(s)
        self._step = step
        self._thread = threading.Thread(target=self._produce, args=(step, self._free_q, self._ready_q, self._stop),
                                        name="dtg-data-producer", daemon=True)
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
            raise RuntimeError("DeviceLoader is closed")
        self._halt()
        self._start(int(step))

    def next(self):
        """-> (images bf16 [batch, 3, S, S] channels_last, labels int64 [batch] on the device, indices int64 [batch]
        on the host) of step ``self.step``; advances the step."""
        if self._closed:
            raise RuntimeError("DeviceLoader is closed")
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
            raise RuntimeError("DeviceLoader: the producer thread failed") from step
        assert step == self._step, (step, self._step)
        if self._cuda:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(slot.ready)
            images = crop_resize_norm(slot.d_raw, slot.d_params, self.S, self._d_scale, self._d_shift)
            labels = slot.d_labels.clone()
            slot.consumed = torch.cuda.Event()
            slot.consumed.record(cur)
        else:
            images = crop_resize_norm(slot.raw, slot.params, self.S, self.scale, self.shift)
            labels = slot.labels.clone()
        if images.dtype != self._dtype:
            images = images.to(self._dtype)
        indices = torch.from_numpy(slot.indices.copy())
        self._free_q.put(slot)
        self._step += 1
        self.batches += 1
        return images, labels, indices

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


class DataFeedHook:
    """Session hook that feeds ``images_ph`` / ``labels_ph`` from a loader.  The batch is a function of the global
    step: ``after_create_session`` seeks the loader to the session's (possibly restored) step, ``before_run`` feeds
    the batch of the current step -- the same one again while the step has not advanced, so a run that only reads
    a variable consumes nothing -- and ``end`` closes the loader."""

    def __init__(self, loader, images_ph, labels_ph, global_step):
        self._loader, self._x, self._y, self._gs = loader, images_ph, labels_ph, global_step
        self._fed = None  # (step, images, labels)

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
            images, labels, _ = self._loader.next()
            self._fed = (step, images, labels)
        return SessionRunArgs(fetches=None, feed_dict={self._x: self._fed[1], self._y: self._fed[2]})

    def after_run(self, run_context, run_values):
        pass

    def end(self, session):
        self._loader.close()
