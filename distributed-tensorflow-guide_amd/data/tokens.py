"""Prefetching token loader: token record shards -> pinned ring -> device -> one masking launch per batch.

The design and the guarantees of ``loader.py::DeviceLoader``, for BERT pre-training records (``input_ids`` int32 [S],
``a_len`` int32, ``length`` int32, ``next_sentence_label`` int64).  A ring of ``depth`` slots, each the four pinned
fields plus the record indices and their device twins.  One producer thread runs steps ``s, s+1, ...``: sampler,
native GIL-free gather into the slot, validation of the lengths, the step's prediction count (``ops/mlm.py::
count_valid`` on the pinned ids: no device read), host->device copies on the loader's own copy stream, an event after
the copies.  ``next()`` makes the current stream wait for that event, launches ``mlm_mask`` on it into fresh output
tensors and records the slot's "consumed" event; the producer reuses a slot only once that event has completed (it
waits on the event, never on the device).

The masks are a pure function of (seed, epoch, record index).  Training takes the step's epoch from the sampler, so
every epoch masks a record anew; evaluation takes epoch 0 and ``eval_seed``, so every evaluation of a set sees the
same masks.  On the CPU the interface is the same, with the PyTorch mirror as the masking and no streams.
"""
import atexit
import json
import os
import queue
import threading
import time
import weakref

import numpy as np
import torch

from ..ops.mlm import MAX_SEQ, count_valid, mlm_mask
from .records import ShardSet
from .sampler import EvalSampler, ShardedSampler

META_FILE = "tokens.json"
# the ids of the uncased BERT vocabulary: [PAD] 0, [CLS] 101, [SEP] 102, [MASK] 103, words from 999
BERT_UNCASED = {"pad_id": 0, "cls_id": 101, "sep_id": 102, "mask_id": 103, "vocab_lo": 999, "vocab_hi": 30522}


def write_token_meta(directory, **ids):
    """The token ids a set was written with -> ``directory/tokens.json`` (settings only)."""
    meta = {k: int(ids[k]) for k in ("pad_id", "cls_id", "sep_id", "mask_id", "vocab_lo", "vocab_hi")}
    with open(os.path.join(directory, META_FILE), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    return meta


def read_token_meta(directory):
    """-> the dict of ``write_token_meta``; BERT's uncased ids when the set has no tokens.json."""
    path = os.path.join(directory, META_FILE)
    if not os.path.exists(path):
        return dict(BERT_UNCASED)
    with open(path) as f:
        return {k: int(v) for k, v in json.load(f).items()}


def masking_args(meta):
    """tokens.json -> the TokenLoader keywords it determines."""
    return dict(mask_id=meta["mask_id"], vocab_lo=meta["vocab_lo"], vocab_hi=meta["vocab_hi"],
                special_ids=(meta["pad_id"], meta["cls_id"], meta["sep_id"], meta["mask_id"]))


class _Slot:
    def __init__(self, batch, S, device):
        cuda = device.type == "cuda"
        self.ids = torch.empty((batch, S), dtype=torch.int32, pin_memory=cuda)
        self.a_len = torch.empty((batch,), dtype=torch.int32, pin_memory=cuda)
        self.length = torch.empty((batch,), dtype=torch.int32, pin_memory=cuda)
        self.nsp = torch.empty((batch,), dtype=torch.int64, pin_memory=cuda)
        self.index = torch.empty((batch,), dtype=torch.int64, pin_memory=cuda)
        self.host = (self.ids, self.a_len, self.length, self.nsp, self.index)
        self.epoch = self.valid = self.num_valid = 0
        if cuda:
            self.dev = tuple(torch.empty_like(t, device=device) for t in self.host)
            self.ready = torch.cuda.Event()
        self.consumed = None  # recorded by next() after the slot's kernel; None: never used


def _close_ref(ref):
    obj = ref()
    if obj is not None:
        obj.close()


class TokenLoader:
    def __init__(self, shards, batch, device, world=1, rank=0, seed=0, train=True, depth=3, P=20, mask_per_mille=150,
                 mask_id=BERT_UNCASED["mask_id"], vocab_lo=BERT_UNCASED["vocab_lo"], vocab_hi=BERT_UNCASED["vocab_hi"],
                 special_ids=(0, 101, 102, 103), drop_last=True, eval_seed=0, threads=2):
        """drop_last=False (evaluation only, ``train=False``): one pass of ``steps_per_epoch`` steps visits every
        record exactly once over the ranks (EvalSampler); the rows that pad the last batches repeat record 0, are
        copied unmasked with every MLM label -1, and carry ``nsp_label`` -1."""
        self.shards = shards if isinstance(shards, ShardSet) else ShardSet(shards)
        fields = self.shards.fields
        dt, shape = fields.get("input_ids", (None, None))
        if dt != "int32" or len(shape) != 1 or not 1 <= shape[0] <= MAX_SEQ:
            raise ValueError("field 'input_ids' must be int32 [S], 1 <= S <= %d, got %s %s" % (MAX_SEQ, dt, shape))
        for name, want in (("a_len", "int32"), ("length", "int32"), ("next_sentence_label", "int64")):
            if fields.get(name) != (want, ()):
                raise ValueError("field %r must be %s []" % (name, want))
        if depth < 1 or not 1 <= threads <= 64:
            raise ValueError("depth >= 1 and 1 <= threads <= 64 required")
        if not drop_last and train:
            raise ValueError("drop_last=False is the evaluation pass: it requires train=False")
        self.S, self.batch, self.P, self.train, self.threads = shape[0], batch, int(P), train, threads
        self.seed = int(seed) if train else int(eval_seed)
        self.device = torch.device(device)
        self._cuda = self.device.type == "cuda"
        self.drop_last = drop_last
        self.mask = dict(P=self.P, mask_per_mille=int(mask_per_mille), mask_id=int(mask_id), vocab_lo=int(vocab_lo),
                         vocab_hi=int(vocab_hi), special_ids=tuple(int(s) for s in special_ids))
        self.sampler = ShardedSampler(len(self.shards), batch, world, rank, seed, shuffle=train) if drop_last else \
            EvalSampler(len(self.shards), batch, world, rank)
        self.steps_per_epoch = self.sampler.steps_per_epoch
        if self._cuda:
            self._copy_stream = torch.cuda.Stream(self.device)
        self._slots = [_Slot(batch, self.S, self.device) for _ in range(depth)]
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
        t0 = time.perf_counter()
        self._gather(slot.ids.data_ptr(), self.shards.addresses("input_ids", idx), self.S * 4, self.threads)
        self._gather(slot.a_len.data_ptr(), self.shards.addresses("a_len", idx), 4, 1)
        self._gather(slot.length.data_ptr(), self.shards.addresses("length", idx), 4, 1)
        self._gather(slot.nsp.data_ptr(), self.shards.addresses("next_sentence_label", idx), 8, 1)
        self.gather_ms += (time.perf_counter() - t0) * 1e3
        a, n = slot.a_len.numpy(), slot.length.numpy()
        if not ((1 <= a) & (a <= n) & (n <= self.S)).all():
            bad = int(np.flatnonzero(~((1 <= a) & (a <= n) & (n <= self.S)))[0])
            raise ValueError("record %d: 1 <= a_len <= length <= %d required, got a_len %d, length %d" % (
                idx[bad], self.S, a[bad], n[bad]))
        if valid < len(idx):
            slot.nsp[valid:] = -1  # padding rows: ignored by the loss and the metrics
        slot.index.copy_(torch.from_numpy(idx))
        slot.epoch = epoch if self.train else 0
        slot.valid = valid
        slot.num_valid = max(1, count_valid(slot.ids.numpy(), n, self.P, self.mask["mask_per_mille"],
                                            self.mask["special_ids"], valid))
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
        for s in self._slots:
            self._free_q.put(s)
        self._step = step
        self._thread = threading.Thread(target=self._produce, args=(step, self._free_q, self._ready_q, self._stop),
                                        name="dtg-token-producer", daemon=True)
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
            raise RuntimeError("TokenLoader is closed")
        self._halt()
        self._start(int(step))

    def next(self):
        """-> ((ids, token_types, attention_mask [batch, S], mlm_positions, mlm_labels [batch, P], nsp_labels
        [batch]) int64 on the device, num_valid: the Python int ``max(1, number of mlm_labels >= 0)`` computed on the
        host, indices int64 [batch] on the host) of step ``self.step``; advances the step."""
        if self._closed:
            raise RuntimeError("TokenLoader is closed")
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
            raise RuntimeError("TokenLoader: the producer thread failed") from step
        assert step == self._step, (step, self._step)
        kw = dict(self.mask, seed=self.seed, epoch=slot.epoch, valid_rows=slot.valid)
        if self._cuda:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(slot.ready)
            ids, a_len, length, nsp, index = slot.dev
            out = mlm_mask(ids, a_len, length, index, **kw)
            nsp = nsp.clone()
            slot.consumed = torch.cuda.Event()
            slot.consumed.record(cur)
        else:
            out = mlm_mask(slot.ids, slot.a_len, slot.length, slot.index, **kw)
            nsp = slot.nsp.clone()
        num_valid, indices = slot.num_valid, slot.index.clone()
        self._free_q.put(slot)
        self._step += 1
        self.batches += 1
        return (*out, nsp), num_valid, indices

    __next__ = next

    def __iter__(self):
        return self

    def counters(self):
        """As ``DeviceLoader.counters``: batches; waits / wait_ms: how often and how long next() blocked on the
        producer; gather_ms: the host gathers; reuse_wait_ms: how long the producer waited for the device to release
        a slot."""
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


class TokenFeedHook:
    """Session hook that feeds the six BERT placeholders from a TokenLoader, as ``DataFeedHook`` does for images: the
    batch is a function of the global step -- ``after_create_session`` seeks the loader to the session's (possibly
    restored) step, ``before_run`` feeds the batch of the current step, the same one again while the step has not
    advanced -- and ``end`` closes the loader.  ``set_num_valid(n)`` is called with the fed batch's prediction count
    before every run, for the model's loss denominator."""

    def __init__(self, loader, placeholders, global_step, set_num_valid=None):
        if len(placeholders) != 6:
            raise ValueError("six placeholders required: ids, token types, attention mask, positions, labels, nsp")
        self._loader, self._ph, self._gs, self._set = loader, list(placeholders), global_step, set_num_valid
        self._fed = None  # (step, tensors, num_valid)

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
            tensors, num_valid, _ = self._loader.next()
            self._fed = (step, tensors, num_valid)
        if self._set is not None:
            self._set(self._fed[2])
        return SessionRunArgs(fetches=None, feed_dict=dict(zip(self._ph, self._fed[1])))

    def after_run(self, run_context, run_values):
        pass

    def end(self, session):
        self._loader.close()
