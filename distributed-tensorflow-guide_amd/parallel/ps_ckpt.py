"""Checkpoint and restart of the GPU parameter servers (parallel/async_ps.py, parallel/sync_ps.py).

The reference's async scripts all checkpoint (``DOWNPOUR/DOWNPOUR.py:121-127``, ``ADAG/ADAG.py:114-115``,
``Hogwild/Hogwild.py:47-49``: a MonitoredTrainingSession with ``checkpoint_dir``); the parameters of dtg's GPU
parameter servers live in one process's HBM, so that process has to write them down.

The servers' host loops never synchronise the device, and a checkpoint keeps that:

* :class:`FlatSnapshot` captures a FlatParams model with ONE ``state_pack`` launch per flat group
  (csrc/kernels/snapshot.hip: the master and the group's optimizer slots into a checkpoint image, every parameter
  in logical order) and one device copy of the flat BN buffers -- enqueued on the apply stream, so the images hold
  exactly the state after the update that precedes them, whatever is applied next;
* :class:`PSCheckpointer` then records an event, lets a dedicated copy stream move the images into pinned host
  memory behind it, and hands a second event to a writer thread, which waits for it, slices the pinned images
  into per-key numpy views (no copy) and writes the TensorBundle through the native in-place writer
  (``_runtime.write_bundle_buffers``: CRC32C and file I/O with the GIL released).  Only then is the ``checkpoint``
  state file replaced, so it never names an incomplete bundle.  A save that comes due while the previous
  snapshot's images are still in flight is skipped (``skipped``): the serve loop never waits for a checkpoint.

The keys are those of ``train/saver.py::flat_arrays`` plus ``global_step``: ``restore_flat``, ``Saver`` and
``CheckpointReader`` read a PS checkpoint, and a checkpoint of the single-process trainers seeds a PS job.
On CPU tensors (the gloo tests) the same code runs without streams.
"""
import os
import queue
import threading
import time

import numpy as np
import torch

from ..ops import snapshot as S
from ..train import saver as _saver


def _slot_keys(g):
    return tuple(g.state.keys())


class FlatSnapshot:
    """Packed checkpoint images of a FlatParams model (and its fused optimizer's slots): per flat group a device
    image and a host image of shape [1 + slots, numel]; the flat BN buffer likewise.  Images are allocated once
    and rebuilt when the slot set changes (momentum / Adam slots appear at the first apply)."""

    def __init__(self, flat, optimizer=None, pin=True):
        self.flat, self.opt = flat, optimizer
        groups = list(flat)
        self.dev = groups[0].master.device if groups else torch.device("cpu")
        self.cuda = self.dev.type == "cuda"
        self.pin = bool(pin and self.cuda)
        self.plans = {g.name: S.SnapshotPlan.of_group(g) for g in groups}
        self._keys = None
        self.dev_img, self.host_img = {}, {}
        self.dev_buf = self.host_buf = None
        self.dev_other = {}  # module buffers outside the flat fp32 buffer (none in dtg's models), by name

    def _slots(self, g):
        return _slot_keys(g) if self.opt is not None else ()

    def ensure(self):
        keys = tuple((g.name, self._slots(g)) for g in self.flat)
        if keys == self._keys:
            return
        self._keys = keys
        for g in self.flat:
            k = 1 + len(self._slots(g))
            plan = self.plans[g.name]
            self.host_img[g.name] = plan.new_image(k, pin=self.pin, device="cpu")
            self.dev_img[g.name] = plan.new_image(k) if self.cuda else self.host_img[g.name]
        fb = self.flat.buffers
        if fb is not None and self.host_buf is None:
            self.host_buf = torch.zeros(fb.numel, dtype=torch.float32, pin_memory=self.pin)
            self.dev_buf = torch.zeros_like(fb.flat) if self.cuda else self.host_buf

    def _bufs(self, g):
        return [g.master] + [g.state[k] for k in self._slots(g)]

    def _flat_buffer_names(self):
        fb = self.flat.buffers
        return set(fb.names) if fb is not None else set()

    def capture(self):
        """Enqueue the snapshot on the current stream: the pack launches and one copy of the flat buffers."""
        self.ensure()
        for g in self.flat:
            bufs, img = self._bufs(g), self.dev_img[g.name]
            for c in range(0, len(bufs), S.MAX_STATE_SRCS):
                S.state_pack(self.plans[g.name], bufs[c:c + S.MAX_STATE_SRCS], img[c:c + S.MAX_STATE_SRCS])
        if self.flat.buffers is not None:
            self.dev_buf.copy_(self.flat.buffers.flat)
        inflat = self._flat_buffer_names()
        self.dev_other = {n: b.detach().clone() for n, b in self.flat.module.named_buffers() if n not in inflat}

    def to_host(self, non_blocking=False):
        """Device images -> host images on the current stream (nothing to do on CPU tensors)."""
        if not self.cuda:
            return
        for g in self.flat:
            self.host_img[g.name].copy_(self.dev_img[g.name], non_blocking=non_blocking)
        if self.dev_buf is not None:
            self.host_buf.copy_(self.dev_buf, non_blocking=non_blocking)

    def arrays(self, step_count=None):
        """The named arrays of ``flat_arrays(flat, optimizer)`` -- same keys, order, shapes and dtypes -- as numpy
        VIEWS of the host images (valid until the next capture lands)."""
        out = []
        np_img = {g.name: self.host_img[g.name].numpy() for g in self.flat}
        for g in self.flat:
            for n, p, o, numel in g.param_slices():
                out.append((n, np_img[g.name][0, o:o + numel].reshape(tuple(p.shape))))
        fb = self.flat.buffers
        if fb is not None:
            hb = self.host_buf.numpy()
            at = {n: (o, v.numel(), tuple(v.shape)) for n, o, v in zip(fb.names, fb.offsets, fb.views)}
        for n, b in self.flat.module.named_buffers():
            if fb is not None and n in at:
                o, numel, shape = at[n]
                out.append((n, hb[o:o + numel].reshape(shape)))
            else:
                out.append((n, _saver._np_of(self.dev_other[n])))
        if self.opt is not None:
            out.append((_saver.SLOT_LAYOUT_KEY, np.array(_saver.SLOT_LAYOUT_LOGICAL, dtype=np.int64)))
            sc = int(getattr(self.opt, "step_count", 0)) if step_count is None else int(step_count)
            out.append(("optimizer/step", np.array(sc, dtype=np.int64)))
            for g in self.flat:
                for j, k in enumerate(self._slots(g)):
                    for n, p, o, numel in g.param_slices():
                        out.append(("%s/%s" % (n, k), np_img[g.name][1 + j, o:o + numel].reshape(tuple(p.shape))))
        return out

    # ---- restore ------------------------------------------------------------------------------------------
    def restorable(self, vals):
        """Can :meth:`load` take ``vals`` whole?  (every parameter present; a slot either complete or absent)"""
        marker = vals.get(_saver.SLOT_LAYOUT_KEY)
        if marker is not None and int(marker) != _saver.SLOT_LAYOUT_LOGICAL:
            return False
        for g in self.flat:
            if self.opt is None and g.state:
                return False
            if any(n not in vals for n in g.names):
                return False
            for k in self._ckpt_slots(g, vals) | set(g.state if self.opt is not None else ()):
                have = ["%s/%s" % (n, k) in vals for n in g.names]
                if any(have) and not all(have):
                    return False
        return True

    @staticmethod
    def _ckpt_slots(g, vals):
        found = set()
        for n in g.names:
            for key in vals:
                if key.startswith(n + "/") and "/" not in key[len(n) + 1:]:
                    found.add(key[len(n) + 1:])
        return found

    def load(self, vals, what="checkpoint"):
        """Load the arrays of a checkpoint (name -> ndarray): each image goes to the device ONCE, ``state_unpack``
        writes masters and slots (their alignment padding untouched: slots are created through
        ``optimizer.new_slot``), the mirrors are refreshed, the buffers and the optimizer's step count loaded."""
        marker = vals.get(_saver.SLOT_LAYOUT_KEY)
        if marker is not None and int(marker) != _saver.SLOT_LAYOUT_LOGICAL:
            raise ValueError("%s: slot layout %d is not the logical layout this restore reads" % (what, int(marker)))
        with torch.no_grad():
            if self.opt is not None:
                for g in self.flat:
                    for k in sorted(self._ckpt_slots(g, vals)):
                        if k not in g.state:
                            self.opt.new_slot(g, k) if hasattr(self.opt, "new_slot") else g.state_buffer(k)
            self.ensure()
            for g in self.flat:
                slots = [k for k in self._slots(g) if any("%s/%s" % (n, k) in vals for n in g.names)]
                img = self.host_img[g.name].numpy()
                rowof = {k: 1 + j for j, k in enumerate(self._slots(g))}
                for n, p, o, numel in g.param_slices():
                    for key, r in [(n, 0)] + [("%s/%s" % (n, k), rowof[k]) for k in slots]:
                        if key not in vals:
                            raise KeyError("Key %s not found in %s" % (key, what))
                        img[r, o:o + numel] = np.asarray(vals[key], dtype=np.float32).reshape(-1)
                bufs = [g.master] + [g.state[k] for k in slots]
                rows = [0] + [rowof[k] for k in slots]
                if self.cuda:
                    self.dev_img[g.name].copy_(self.host_img[g.name], non_blocking=True)
                dimg = self.dev_img[g.name]
                # consecutive image rows go in one launch (all of them, unless the checkpoint lacks a slot)
                i = 0
                while i < len(rows):
                    j = i + 1
                    while j < len(rows) and j - i < S.MAX_STATE_SRCS and rows[j] == rows[j - 1] + 1:
                        j += 1
                    S.state_unpack(self.plans[g.name], bufs[i:j], dimg[rows[i]:rows[i] + (j - i)])
                    i = j
                g.refresh_mirror()
            fb = self.flat.buffers
            inflat = self._flat_buffer_names()
            if fb is not None:
                hb = self.host_buf.numpy()
                hb[:] = fb.flat.detach().cpu().numpy()  # keys the checkpoint lacks keep their values
                for n, o, v in zip(fb.names, fb.offsets, fb.views):
                    if n in vals:
                        hb[o:o + v.numel()] = np.asarray(vals[n], dtype=np.float32).reshape(-1)
                fb.flat.copy_(self.host_buf, non_blocking=True)
            for n, b in self.flat.module.named_buffers():
                if n not in inflat and n in vals:
                    b.copy_(torch.from_numpy(np.asarray(vals[n])).view(b.shape))
        opt = self.opt
        if opt is not None and "optimizer/step" in vals and hasattr(opt, "step_count"):
            opt.step_count = int(vals["optimizer/step"])
            if hasattr(opt, "hyper"):
                opt.hyper[1].fill_(float(opt.step_count))


class PSCheckpointer:
    """Periodic checkpoints of a parameter server's FlatParams state, off the serve thread (module docstring).

    ``every_n``: save when ``step`` is a multiple of it; ``every_secs``: save when that long has passed since the
    last save was started.  Counters: ``saved`` (steps whose bundle is complete and named by the state file),
    ``skipped`` (saves that came due while the previous one was in flight)."""

    def __init__(self, flat, optimizer, ckpt_dir, every_n=None, every_secs=None, max_to_keep=5, basename="model.ckpt"):
        self.flat, self.opt = flat, optimizer
        self.dir = os.path.abspath(ckpt_dir)
        os.makedirs(self.dir, exist_ok=True)
        self.every_n = int(every_n) if every_n else None
        self.every_secs = float(every_secs) if every_secs else None
        self.max_to_keep = max_to_keep
        self.basename = basename
        self.snap = FlatSnapshot(flat, optimizer)
        self.cuda = self.snap.cuda
        self._copy_stream = torch.cuda.Stream(self.snap.dev) if self.cuda else None
        self._idle = threading.Event()
        self._idle.set()
        self._q = None
        self._thread = None
        self.error = None
        self.saved = []
        self.skipped = 0
        self.restored = None
        self._last_started = None
        self._last_seen = None
        self._last_time = time.monotonic()
        st = _saver.get_checkpoint_state(self.dir)
        self._paths = list(st.all_model_checkpoint_paths) if st else []

    # ---- the writer thread ---------------------------------------------------------------------------------
    def _start(self):
        if self._thread is None:
            self._q = queue.Queue()
            self._thread = threading.Thread(target=self._run, name="dtg-ps-ckpt", daemon=True)
            self._thread.start()

    def _run(self):
        while True:
            job = self._q.get()
            if job is None:
                return
            step, extra, step_count, ev = job
            try:
                if ev is not None:
                    ev.synchronize()  # the images are in pinned host memory
                arrays = self.snap.arrays(step_count)
                arrays.append(("global_step", np.array(int(step), dtype=np.int64)))
                for k, v in (extra or {}).items():
                    arrays.append((k, np.asarray(v)))
                prefix = os.path.join(self.dir, "%s-%d" % (self.basename, int(step)))
                _saver.write_tensors_inplace(prefix, arrays)
                self._paths = [p for p in self._paths if p != prefix] + [prefix]
                while self.max_to_keep and len(self._paths) > self.max_to_keep:
                    old = self._paths.pop(0)
                    for suf in (".index", ".data-00000-of-00001", ".meta"):
                        try:
                            os.remove(old + suf)
                        except OSError:
                            pass
                # only now: the state file never names an incomplete bundle (temp file + os.replace)
                _saver.update_checkpoint_state(self.dir, prefix, self._paths)
                self.saved.append(int(step))
            except Exception as e:  # surfaced by the next maybe_save() / flush()
                self.error = e
            finally:
                self._idle.set()

    def _check(self):
        if self.error is not None:
            e, self.error = self.error, None
            raise RuntimeError("PS checkpoint writer failed") from e

    # ---- the serve thread ----------------------------------------------------------------------------------
    def _due(self, step):
        if step == self._last_started:
            return False
        if self.every_n and step > 0 and step % self.every_n == 0:
            return True
        return bool(self.every_secs) and time.monotonic() - self._last_time >= self.every_secs

    def _save(self, step, extra):
        self._start()
        self._idle.clear()
        self._last_started = step
        self._last_time = time.monotonic()
        self.snap.capture()  # on the apply (current) stream: the state after update `step`
        ev2 = None
        if self.cuda:
            cur = torch.cuda.current_stream(self.snap.dev)
            ev1 = torch.cuda.Event()
            ev1.record(cur)
            self._copy_stream.wait_event(ev1)
            with torch.cuda.stream(self._copy_stream):
                self.snap.to_host(non_blocking=True)
                ev2 = torch.cuda.Event()
                ev2.record(self._copy_stream)
        self._q.put((int(step), dict(extra or {}), int(getattr(self.opt, "step_count", 0)), ev2))
    def maybe_save(self, step, extra=None):
        """Between two requests, on the serve thread: start a checkpoint of the state after update ``step`` if one
        is due.  Never waits: returns True if a save was started, False if none was due or the previous one is
        still in flight (counted in ``skipped``)."""
        self._check()
        self._last_seen = (int(step), dict(extra or {}))
        if not self._due(step):
            return False
        if not self._idle.is_set():
            self.skipped += 1
            return False
        self._save(step, extra)
        return True

    def wait(self):
        """Block until no snapshot is in flight (tools and tests; the servers never call this)."""
        self._idle.wait()
        self._check()

    def flush(self, step=None, extra=None):
        """A final snapshot (of ``step``, default: the last step ``maybe_save`` saw, unless that one was saved
        already), then wait for the writer and stop it."""
        if step is None and self._last_seen is not None:
            step, extra = self._last_seen
        if self._thread is not None:
            self._idle.wait()
        if step is not None and step != self._last_started and self.error is None:
            self._save(step, extra)
            self._idle.wait()
        if self._thread is not None:
            self._q.put(None)
            self._thread.join()
            self._thread = None
        self._check()

    # ---- restart -------------------------------------------------------------------------------------------
    def latest(self):
        return _saver.latest_checkpoint(self.dir)

    def restore_latest(self):
        """Load the latest checkpoint of the directory into the model and the optimizer; returns its global step
        (None when the directory holds no checkpoint).  ``restored`` keeps (prefix, the bundle's scalar extras)."""
        prefix = self.latest()
        self.restored = None
        if prefix is None:
            return None
        vals = _saver.read_tensors(prefix)
        self.snap.load(vals, prefix)
        if self.cuda:
            torch.cuda.current_stream(self.snap.dev).synchronize()  # once, before serving starts
        step = int(vals["global_step"]) if "global_step" in vals else 0
        self.restored = (prefix, {k: v for k, v in vals.items() if k.startswith("dtg/") and np.ndim(v) == 0})
        self._last_started = step
        return step
