"""Asynchronous parameter server on GPUs: one PS rank keeps the parameters in HBM, workers push
gradients and pull parameters; every gradient is applied as soon as it arrives.  The transport (RCCL point-to-point
payloads, request framing, failure detection, GPU-ready request order) and the server / worker base classes are
parallel/ps_core.py's; this module is the asynchronous protocol on top of them.

This is the GPU-scale form of the reference's between-graph async training (SURVEY §2.3 Hogwild,
DOWNPOUR, ADAG; §2.4 (b); BASELINE.json config 4 "ResNet-50 async parameter-server, 1 PS + 7
workers intra-node (RCCL send/recv)").  Reference semantics kept:

* Hogwild (``Hogwild/Hogwild.py:44-57``): every worker gradient is applied on the PS as soon as it
  arrives, no locking across workers; a worker computes on whatever parameters it last pulled.
* DOWNPOUR / ADAG window (``DOWNPOUR/DOWNPOUR.py:63-102``, ``ADAG/ADAG.py:69-90``): a worker runs
  ``window`` local steps (optionally applying a local optimizer), accumulates their gradients and
  pushes the sum (DOWNPOUR) or the mean (ADAG); the PS applies it with the global optimizer.
* Dynamic SGD (the reference README's TODO list, ``README.md:40``): ``staleness_scaling="dyn"``
  scales every update by 1/(tau+1), tau = the number of PS updates since the pushing worker last
  pulled (DynSGD, Jiang et al., SIGMOD 2017), so stale gradients from slow workers move the
  parameters less.

MI355X design (the transport's part of it is in parallel/ps_core.py):

* **bounded queue**: the PS bounds how many requests' device work it has queued (``max_inflight``; the host
  waits on the oldest request's completion event beyond it), so its pair streams cannot pile up.
* **staleness** tau of an update = the number of PS updates applied between the pushing worker's last pull
  (the parameter snapshot its gradient was computed on) and this update.  With W workers in round-robin tau is
  about W - 1; ``overlap_pull`` adds one exchange (about W more): the one-card 1 PS + 7 worker rehearsal with
  overlapped pulls measured a mean of 6.0 (``profiles/r04_async_ps``).
* **overlap** (``overlap_pull=True``): the worker snapshots its gradients into a send buffer, posts the
  push and the pull, and goes on with its next step on the parameters it already has; the pulled ones
  are swapped in (a device copy) at its next exchange.  That adds one step of staleness, which Hogwild
  semantics allow, and takes the push -> PS apply -> pull round trip off the worker's critical path.
  Without it the worker's GPU waits for the pull (its host does not).
"""
import os
import time

import torch
import torch.distributed as dist

from ..utils.trace import traced
from .ps_core import (_ELASTIC, _GRAD, _WARM, _Control, _elastic_state, _group_payload_grads, _group_payload_params,
                      _buffers, _irecv, _isend, _PSServer, _PSWorker, _ready_event, _wait_all, init_from_cluster)  # noqa: F401

_VERSION_KEY = "dtg/ps/version"  # the async PS's parameter version in its checkpoints (parallel/ps_ckpt.py)


class AsyncPSWorker(_PSWorker):
    """Worker side.  ``begin()`` pulls the current parameters, ``step_done()`` after every backward
    pushes/pulls every ``window`` steps, ``warm()`` marks the end of a warm-up phase (benchmarks),
    ``finish()`` tells the PS this worker is done (the PS's ``serve()`` returns when all workers finished).
    Under a session (``minimize``) the graph ``global_step`` counts this worker's local steps (the PS counts
    updates)."""

    _op_name = "async_ps_train"

    def __init__(self, flat, ps_rank=0, window=1, window_mode="sum", local_optimizer=None, group=None,
                 overlap_pull=False):
        assert window_mode in ("sum", "mean")
        super().__init__(flat, ps_rank, group)
        self.window = max(1, int(window))
        self.window_mode = window_mode
        self.local_opt = local_optimizer
        self.overlap = bool(overlap_pull)
        self._acc = [torch.zeros_like(g.grad) for g in flat] if (self.window > 1 and local_optimizer) else None
        # overlap: gradient snapshot being sent, parameters being received (double buffers)
        self._gsnap = [torch.empty_like(g.grad) for g in flat] if self.overlap else None
        self._pbuf = [torch.empty_like(t) for t in _group_payload_params(flat)] if self.overlap else None
        self._sends = []
        self._pull = None
        self.local_step = 0
        self.pushes = 0
        self.ps_updates_at_begin = 0  # the PS's update count when this job started (begin(); > 0 after a restart)

    def begin(self):
        """Initial pull (replaces the chief's assign_global + sleep(10) bootstrap,
        DOWNPOUR/DOWNPOUR.py:129-135).  Also reads the update count the PS started from -- 0 on a fresh job, the
        restored checkpoint's after a restart -- so a worker can run "until the PS has applied N updates"."""
        _wait_all([_irecv(t, self.ps, self.pg) for t in _group_payload_params(self.flat)])
        self._pulled()
        store = dist.distributed_c10d._get_default_store()
        self.ps_updates_at_begin = int(store.get(self._ctl.key + ".updates0").decode())

    def _pulled(self):
        super()._pulled()
        if self.local_opt is not None:
            # the local optimizer updates the fp32 master: re-seed it from the pulled parameters
            for g in self.flat:
                if g.mirror is not None:
                    g.master.copy_(g.mirror)

    @traced("dtg.ps.pull")
    def _land_pull(self):
        """Overlap mode: the previous exchange's parameters -> the model (stream-ordered device copy)."""
        if self._pull is None:
            return
        _wait_all(self._pull)
        self._pull = None
        for dst, src in zip(_group_payload_params(self.flat), self._pbuf):
            dst.copy_(src)
        self._pulled()

    @traced("dtg.ps.push")
    def step_done(self):
        """Call once per local step after backward.  Pushes/pulls every ``window`` steps; returns
        True when an exchange with the PS happened."""
        self.local_step += 1
        if self._acc is not None:
            # DOWNPOUR-style: accumulate this step's gradient, then take a local optimizer step -- on the first T - 1
            # steps of the window only, as the reference's graph runs it (DOWNPOUR/DOWNPOUR.py:65-75: the t-th
            # compute_gradients waits for opt_local of step t - 1, and nothing waits for the last one, so a window
            # of T gradient evaluations applies T - 1 local updates).  The last local update
            # would be overwritten by the pull anyway, but it would still feed the local optimizer's state (an
            # Adagrad accumulator, a momentum buffer) a gradient the reference never applies locally.
            for a, g in zip(self._acc, self.flat):
                a.add_(g.grad.to(a.dtype))
            if self.local_step % self.window:
                self.local_opt.step()
        if self.local_step % self.window:
            return False
        self._land_pull()
        grads = self._acc if self._acc is not None else _group_payload_grads(self.flat)
        self._buffer_delta()
        _wait_all(self._sends)  # the previous push's buffers are free again
        if self.overlap:
            for s, g in zip(self._gsnap, grads):
                s.copy_(g)
            grads_out = self._gsnap
        else:
            grads_out = grads
        # the token goes out when the gradient exists on the device (announcer thread), the sends are posted now
        self._ann.submit(self.rank, _GRAD, _ready_event(list(grads_out) + self._bufd))
        self._sends = [_isend(t, self.ps, self.pg) for t in list(grads_out) + self._bufd]
        if self.overlap:
            self._pull = [_irecv(t, self.ps, self.pg) for t in self._pbuf]
        else:
            _wait_all(self._sends)  # (stream-ordered) before the gradients are zeroed below
            self._sends = []
        for t in grads:
            t.zero_()
        if self._acc is not None:
            self.flat.zero_grad()
        if not self.overlap:
            _wait_all([_irecv(t, self.ps, self.pg) for t in _group_payload_params(self.flat)])
            self._pulled()
        self.pushes += 1
        return True

    def _step_global(self, global_step, session):
        if global_step is not None:
            with global_step._lock:
                global_step._local.add_(1)

    def warm(self):
        """Tell the PS this worker has finished its warm-up (``AsyncPSServer.timed`` starts when all have)."""
        self._ann.submit(self.rank, _WARM)

    def finish(self):
        self._land_pull()
        _wait_all(self._sends)
        self._sends = []
        super().finish()


class AsyncPSServer(_PSServer):
    """PS side: ``serve()`` runs until every worker sent DONE (or was lost); returns the number of updates."""

    _mode = "async"

    def __init__(self, flat, optimizer, workers, window=1, window_mode="sum", group=None, staleness_log=False,
                 staleness_scaling=None, worker_timeout=None, max_inflight=None, checkpointer=None):
        assert staleness_scaling in (None, "dyn")
        super().__init__(flat, optimizer, workers, group, worker_timeout, checkpointer)
        self.dyn = staleness_scaling == "dyn"
        self.gscale = 1.0 / window if window_mode == "mean" else 1.0
        self.updates = 0
        self.version = 0
        self.staleness = [] if staleness_log else None
        self.scales = [] if staleness_log else None
        self.per_worker = {w: 0 for w in self.workers}
        self._warm = set()
        self.timed = None  # (updates, time) when every worker reported warm; serve() fills timed_end
        # applied order: (worker, that worker's push index) per update -- what a replay of the PS must follow
        self.order = []
        self._push_idx = {w: 0 for w in self.workers}
        # requests whose device work (receive, apply, snapshot, send) may be queued at once; beyond that the host
        # waits for the oldest one's completion event (one outstanding request per worker by default)
        self.max_inflight = int(max_inflight if max_inflight is not None else
                                os.environ.get("DTG_PS_MAX_INFLIGHT", str(max(1, len(self.workers)))))
        self._inflight = []
        # after a restart the update count and the parameter version continue from the checkpoint.  The update
        # count this server starts from is published for the workers (AsyncPSWorker.ps_updates_at_begin).
        if self.restored_step is not None:
            self.updates = self.restored_step
            self.version = int(checkpointer.restored[1].get(_VERSION_KEY, self.restored_step))
        self._pulled_version = {w: self.version for w in self.workers}
        self.updates_at_begin = self.updates
        dist.distributed_c10d._get_default_store().set(self._ctl.key + ".updates0", str(self.updates))

    def _send_params(self, w):
        super()._send_params(w)
        self._pulled_version[w] = self.version

    @traced("dtg.ps.apply")
    def _apply(self, w):
        tau = self.version - self._pulled_version[w]
        scale = self.gscale / (tau + 1) if self.dyn else self.gscale
        self.opt.step(grad_scale=scale, zero_grad=False, grads=self._recv[w])
        # running statistics: add the worker's update since its pull (lock-free, Hogwild-style, like the
        # reference's unlocked assign_moving_average on PS variables)
        for b, d in zip(_buffers(self.flat), self._recv_buf[w]):
            b.add_(d)
        if self.staleness is not None:
            self.staleness.append(tau)
            self.scales.append(scale)
        self.version += 1
        self.updates += 1
        self.per_worker[w] += 1
        self.order.append((w, self._push_idx[w]))
        self._push_idx[w] += 1

    def _bound_inflight(self, w):
        """Record this request's completion on the apply stream; wait for the oldest beyond max_inflight.

        The wait polls the event against ``worker_timeout`` instead of blocking in ``synchronize()``: a worker that
        died mid-transfer leaves its receive (and so the apply stream behind it) pending forever, and the host must
        still fail-stop with a TimeoutError naming that worker (parallel/ps_core.py, failure detection)."""
        if self.dev.type != "cuda":
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        self._inflight.append((ev, w))
        while len(self._inflight) > self.max_inflight:
            ev0, w0 = self._inflight.pop(0)
            deadline = time.monotonic() + self.worker_timeout
            nap = 5e-5
            while not ev0.query():
                if time.monotonic() > deadline:
                    raise TimeoutError("async PS: the request of worker rank %d has not completed on the device in "
                                       "%.0f s (worker lost mid-transfer?)" % (w0, self.worker_timeout))
                time.sleep(nap)
                nap = min(nap * 2, 2e-3)

    def _grad(self, w):
        self._recv_push(w)
        self._apply(w)
        self._send_params(w)
        self._bound_inflight(w)

    def _elastic(self, w):
        """EASGD exchange (Zhang, Choromanska, LeCun 2015): receive the worker's parameters x_i,
        d = alpha * (x_i - x~), x~ += d, send d back (the worker applies x_i -= d)."""
        bufs = self._recv_elastic[w]
        _wait_all([_irecv(b, w, self.pg) for b in bufs])
        with torch.no_grad():
            for c, b in zip(_elastic_state(self.flat), bufs):
                b.sub_(c).mul_(self.elastic_alpha)
                c.add_(b)
            for g in self.flat:
                g.refresh_mirror()
        _wait_all(self._send_works[w])
        snap = self._snap_elastic[w]
        for s_, b in zip(snap, bufs):
            s_.copy_(b)
        self._send_works[w] = [_isend(s_, w, self.pg) for s_ in snap]
        self.version += 1
        self.updates += 1
        self.per_worker[w] += 1

    def enable_elastic(self, alpha):
        """Serve EASGD exchanges: the PS parameters are the elastic center variable x~."""
        self.elastic_alpha = float(alpha)
        self._recv_elastic = {w: [torch.empty_like(t) for t in _elastic_state(self.flat)] for w in self.workers}
        self._snap_elastic = {w: [torch.empty_like(t) for t in _elastic_state(self.flat)] for w in self.workers}
        return self

    def _request(self, w, kind, arg, live):
        if kind == _WARM:
            self._warm.add(w)
            if self._warm >= set(self.workers) - set(self.lost) and self.timed is None:
                self._sync()
                self.timed = (self.updates, time.perf_counter())
            return
        if kind == _ELASTIC:
            self._elastic(w)
        else:
            self._grad(w)
        self._checkpoint(self.updates, {_VERSION_KEY: self.version})

    def _finish(self):
        self.timed_end = (self.updates, time.perf_counter())
        self._flush(self.updates, {_VERSION_KEY: self.version})
        return self.updates


class ElasticWorker:
    """Asynchronous elastic-averaging SGD worker (AEASGD; AEAMSGD with a momentum local optimizer) --
    the algorithms the reference lists as TODO (README.md:40-42, paper link README.md:99).

    The worker trains its own replica x_i with ``local_optimizer`` every step; every ``tau`` steps it
    exchanges with the PS center x~:  d = alpha (x_i - x~);  x_i -= d;  x~ += d  (moving-average
    coupling instead of gradient pushes; the PS must call ``AsyncPSServer.enable_elastic(alpha)``).
    """

    def __init__(self, flat, local_optimizer, tau=4, ps_rank=0, group=None):
        self.flat = flat
        self.opt = local_optimizer
        self.tau = max(1, int(tau))
        self.ps = ps_rank
        self.pg = group
        self.rank = dist.get_rank()
        self._ctl = _Control(False, self.rank)
        self._d = [torch.empty_like(t) for t in _elastic_state(flat)]
        self.local_step = 0
        self.exchanges = 0

    def begin(self):
        """Start from the center: receive the PS parameters (mirror / fp32 group) into the replica."""
        _wait_all([_irecv(t, self.ps, self.pg) for t in _group_payload_params(self.flat)])
        with torch.no_grad():
            for g in self.flat:
                if g.mirror is not None:
                    g.master.copy_(g.mirror)

    def step_done(self):
        """After backward: local optimizer step; every tau steps an elastic exchange."""
        self.local_step += 1
        self.opt.step()
        if self.local_step % self.tau:
            return False
        self._ctl.request(self.rank, _ELASTIC)
        _wait_all([_isend(t, self.ps, self.pg) for t in _elastic_state(self.flat)])
        _wait_all([_irecv(d, self.ps, self.pg) for d in self._d])
        with torch.no_grad():
            for t, d in zip(_elastic_state(self.flat), self._d):
                t.sub_(d)
            for g in self.flat:
                g.refresh_mirror()
        self.exchanges += 1
        return True

    def finish(self):
        self._ctl.finish(self.rank)
