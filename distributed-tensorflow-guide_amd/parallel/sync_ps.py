"""Synchronous parameter server with backup workers for FlatParams models (ResNet-50, BERT, MNIST).

The reference defines synchronous SGD as "aggregate N of M gradients, drop the M - N stale ones"
(``Synchronous-SGD/README.md:3``, ``ssgd.py:51-60``: ``SyncReplicasOptimizer(replicas_to_aggregate=N,
total_num_replicas=M)``).  For the toy graph dtg keeps that in the C++ PS accumulators (csrc/ps/server.cc
ACC_*); this module is the GPU form: one PS rank owns the parameters in HBM, M workers push gradients, a
global step closes as soon as R = ``replicas_to_aggregate`` FRESH gradients have arrived, and the M - R
gradients that arrive late (computed on an older parameter version) are dropped.

Everything that moves bytes is the async PS's (parallel/async_ps.py): pair-wise RCCL send/recv (gloo with host
staging for one-card rehearsals and CPU tests), the native control channel, the announcer thread that releases a
request token only once the gradient exists on the device, per-worker receive and snapshot buffers, lost-worker
detection through the watched control connection.  New here are the protocol and the PS-side reduce + apply.

Versioning
    The PS owns ``global_step``.  A worker's ``local_step`` is the global step of the parameter version it last
    received; it travels INSIDE the request token (rank, kind, local_step), so the PS host decides freshness
    (``local_step == global_step``) without a device synchronisation.

Push (worker)
    one send per payload tensor (a gradient buffer per dtype group, the BN running-statistics delta), the token
    through the announcer after the gradient's device event; then the worker posts the parameter receives and
    blocks -- GIL released, in the native client -- on its own reply queue for ``(global_step, accepted, stop)``,
    at most ``DTG_SYNC_TIMEOUT`` seconds (:class:`SyncTimeoutError`).  Every push is answered by exactly one reply
    and one parameter send.

Serve (PS)
    the receive of every push is posted (the send is already on the wire), from the apply stream, so it is
    ordered after the previous kernel that read that buffer.  A stale push counts as ``dropped[w]`` and is answered
    at once with the current parameters and ``accepted = 0``.  A fresh push joins the pending list in arrival
    order (so per worker ``contributed + dropped`` = its pushes); when the list holds R pushes the step closes:

    * ``opt.step_sum`` over the R pending receive buffers with ``grad_scale = 1/R`` -- ONE fused k-way sum-apply
      kernel per dtype group (csrc/kernels/optim.hip) reads the R buffers, sums them in fp32 registers in arrival
      order, runs the optimizer rule and writes master, slots and the bf16 mirror.  There is no fp32 accumulator
      round trip: per element of the bf16 compute group with momentum SGD that is 2 R + 18 bytes against
      10 R + 26 for accumulate-as-they-arrive (``axpby`` per push, then the apply);
    * the PS buffers (BN running statistics) take ``1/R`` of the sum of the contributors' deltas (``grad_sum``);
    * ``global_step += 1``, the contributor tuple is appended to ``steps``, and each contributor gets a snapshot of
      the new parameters with ``accepted = 1``.

Lost and finished workers
    a worker whose control connection drops is ``lost`` (as in the async server) and a pending push of it is
    discarded.  Once fewer than R workers are live (neither DONE nor lost) no step can close any more: the pending
    pushes and every later push are answered with ``stop = 1`` and the current parameters (they count as dropped:
    they were not aggregated); such a worker sets
    ``stopped`` and its train op requests the session's stop.  ``serve()`` returns when every worker is DONE or
    lost; ``worker_timeout`` bounds the wait for the next request as in the async server.

Checkpoint and restart
    ``SyncPSServer(..., checkpointer=PSCheckpointer(...))`` (parallel/ps_ckpt.py): the constructor restores the
    directory's latest checkpoint (``global_step`` continues from it; the workers receive it with their initial
    pull), ``maybe_save`` runs after every closed step -- it only enqueues on the apply stream -- and ``serve()``
    ends with ``flush()``.  Recovery from a PS fault is a restart of the whole job; workers that lose the PS fail
    as before.
"""
import os
import sys

import torch
import torch.distributed as dist

from .. import fault
from ..graph import Op
from ..ops import optim_kernels as K
from ..train.hooks import SessionRunHook
from ..utils.trace import traced
from .async_ps import (_DONE, _GRAD, _KINDS, _Announcer, _Control, _buffers, _group_payload_grads,
                       _group_payload_params, _irecv, _isend, _ready_event, _wait_all, init_from_cluster)  # noqa: F401

_SREQ = "dtg.sps.req"
_STEP_SHIFT = 24  # token = local_step << 24 | rank * _KINDS + kind


def _reply_queue(rank):
    return "dtg.sps.rep.%d" % rank


class _SyncControl(_Control):
    """The async PS's control channel on a request queue of its own, with the step in the token and one reply
    queue per worker.  A worker blocks on its reply queue through a SECOND connection: its announcer thread sends
    request tokens through the first one meanwhile."""

    def __init__(self, is_ps, rank):
        super().__init__(is_ps, rank, _SREQ)
        self.rank = rank
        self._rcli = None
        if not is_ps:
            from .. import _runtime
            self._rcli = _runtime.PSClient(self.addr[0], self.addr[1], 60.0)

    def request(self, rank, kind):
        kind, step = kind if isinstance(kind, tuple) else (kind, 0)
        self.cli.q_enqueue(_SREQ, [(int(step) << _STEP_SHIFT) | (rank * _KINDS + kind)])

    @staticmethod
    def decode(tok):
        """(rank, kind, local_step) of a request token."""
        w, kind = divmod(tok & ((1 << _STEP_SHIFT) - 1), _KINDS)
        return w, kind, tok >> _STEP_SHIFT

    def reply(self, rank, global_step, accepted, stop):
        self.cli.q_enqueue(_reply_queue(rank), [int(global_step) * 4 + (2 if accepted else 0) + (1 if stop else 0)])

    def wait_reply(self, timeout):
        """(global_step, accepted, stop), or None after ``timeout`` seconds."""
        v = self._rcli.q_dequeue(_reply_queue(self.rank), float(timeout))
        if v is None:
            return None
        return v >> 2, bool(v & 2), bool(v & 1)

    def close(self):
        if self._rcli is not None:
            self._rcli.close()
            self._rcli = None
        super().close()


def _sync_timeout():
    return float(os.environ.get("DTG_SYNC_TIMEOUT", "600"))


class SyncPSWorker:
    """Worker side.  ``begin()`` pulls the initial parameters and their version, ``step_done()`` after every
    backward pushes the gradient and waits for the PS's answer (True if it was aggregated, False if it was dropped
    as stale or the job is stopping), ``finish()`` tells the PS this worker is done."""

    def __init__(self, flat, ps_rank=0, group=None, timeout=None):
        self.flat = flat
        self.ps = ps_rank
        self.pg = group
        self.rank = dist.get_rank()
        self.timeout = float(timeout) if timeout is not None else _sync_timeout()
        self._ctl = _SyncControl(False, self.rank)
        self._ann = _Announcer(self._ctl)
        self._buf0 = [torch.empty_like(b) for b in _buffers(flat)]
        self._bufd = [torch.empty_like(b) for b in _buffers(flat)]
        self.local_step = 0    # the global step of the parameters this worker computes on
        self.global_step = 0   # the PS's global step as of the last reply
        self.pushes = 0
        self.contributed = 0
        self.dropped = 0
        self.stopped = False   # the PS said no further step can close (fewer than R live workers)

    def _wait_reply(self):
        from ..train.sync_replicas import SyncTimeoutError
        r = self._ctl.wait_reply(self.timeout)
        if r is None:
            raise SyncTimeoutError(
                "sync PS: worker rank %d got no answer from the PS (rank %d) in %.0f s -- fewer than "
                "replicas_to_aggregate workers are pushing, or the PS is gone" % (self.rank, self.ps, self.timeout))
        return r

    def _pulled(self):
        for b0, b in zip(self._buf0, _buffers(self.flat)):
            b0.copy_(b)

    def begin(self):
        """Initial pull: the PS's parameters and the global step they belong to."""
        recvs = [_irecv(t, self.ps, self.pg) for t in _group_payload_params(self.flat)]
        step, _, stop = self._wait_reply()
        _wait_all(recvs)
        self._pulled()
        self.local_step = self.global_step = step
        self.stopped = stop

    @traced("dtg.sps.push")
    def step_done(self):
        """Call once per local step after backward: push, wait for the PS's verdict, take the parameters it sent.
        Returns True when this gradient was one of the R aggregated into a global step."""
        if self.stopped:
            self.flat.zero_grad()
            return False
        grads = _group_payload_grads(self.flat)
        for d, b, b0 in zip(self._bufd, _buffers(self.flat), self._buf0):
            torch.sub(b, b0, out=d)
        payload = list(grads) + self._bufd
        # the token (with the version this gradient was computed on) leaves when the gradient exists on the device
        self._ann.submit(self.rank, (_GRAD, self.local_step), _ready_event(payload))
        _wait_all([_isend(t, self.ps, self.pg) for t in payload])  # (stream-ordered) before the gradients are zeroed
        for t in grads:
            t.zero_()
        recvs = [_irecv(t, self.ps, self.pg) for t in _group_payload_params(self.flat)]
        step, accepted, stop = self._wait_reply()
        _wait_all(recvs)
        self._pulled()
        self.pushes += 1
        self.local_step = self.global_step = step
        if accepted:
            self.contributed += 1
        else:
            self.dropped += 1  # stale, or released unaggregated because the job is stopping
        self.stopped = stop
        return accepted

    # ---- session surface (train/eager.py) ------------------------------------------------------------------
    def minimize(self, loss_fn, global_step=None, inputs=(), name="sync_ps_train"):
        """A train op for ``sess.run``: forward + backward of ``loss_fn(*inputs)``, then :meth:`step_done`; the
        graph ``global_step`` is SET to the step the PS returned, so ``StopAtStepHook(last_step=N)`` stops every
        worker at global step N -- a backup worker whose last push was dropped included.  When the PS answers
        ``stop`` the op requests the session's stop."""
        from ..train.eager import EagerGradients
        return _SyncPSApply(EagerGradients(loss_fn, inputs, name + "/gradients"), self, global_step, name)

    def make_session_run_hook(self):
        """after_create_session: the initial pull (:meth:`begin`); end: :meth:`finish`."""
        return _SyncPSHook(self)

    def finish(self):
        self._ann.close()  # every GRAD token is out before DONE
        self._ctl.unwatch()
        try:
            self._ctl.request(self.rank, _DONE)
        except RuntimeError as e:
            # the last worker's DONE lets the PS leave serve() and close its control service, which can go down
            # before the reply to that enqueue is flushed; this worker has no further requests
            if "connection lost" not in str(e):
                raise
        self._ctl.close()


class _SyncPSApply(Op):
    """The worker's train op (SyncPSWorker.minimize)."""

    def __init__(self, grads, worker, global_step, name):
        self.grads, self.worker, self.global_step = grads, worker, global_step
        super().__init__(lambda c, *a: None, [grads], name)

    def _eval(self, ctx):
        ctx.eval(self.grads)
        self.worker.step_done()
        gs = self.global_step
        if gs is not None:
            with gs._lock:
                gs._local.fill_(self.worker.global_step)
        if self.worker.stopped and ctx.session is not None:
            ctx.session.request_stop()
        return None

    @property
    def loss(self):
        """The step's loss as a fetchable tensor (fetching it synchronises the device)."""
        return self.grads


class _SyncPSHook(SessionRunHook):
    """SyncPSWorker.make_session_run_hook: initial pull once the session exists, finish() at its end."""

    def __init__(self, worker, global_step=None):
        self.worker = worker
        self.global_step = global_step
        self._begun = False

    def after_create_session(self, session, coord):
        if not self._begun:
            self.worker.begin()
            self._begun = True
            gs = self.global_step
            if gs is not None:
                with gs._lock:
                    gs._local.fill_(self.worker.global_step)

    def end(self, session):
        if self._begun:
            self.worker.finish()
            self._begun = False


class SyncPSServer:
    """PS side: ``serve()`` runs until every worker sent DONE (or was lost); returns the number of global steps.

    Counters: ``contributed[w]`` / ``dropped[w]`` per worker, ``steps`` (the contributor tuple of every global
    step, in the order their gradients were summed), ``lost``."""

    def __init__(self, flat, optimizer, workers, replicas_to_aggregate, group=None, worker_timeout=None,
                 global_step=0, checkpointer=None):
        self.flat = flat
        self.opt = optimizer
        self.workers = list(workers)
        self.R = int(replicas_to_aggregate)
        if not 1 <= self.R <= len(self.workers):
            raise ValueError("replicas_to_aggregate=%d with %d worker(s)" % (self.R, len(self.workers)))
        self.pg = group
        self.worker_timeout = worker_timeout if worker_timeout is not None else float(
            os.environ.get("DTG_PS_WORKER_TIMEOUT", "600"))
        self.dev = next(iter(flat)).master.device
        self._ctl = _SyncControl(True, dist.get_rank())
        self._recv = {w: [torch.empty_like(g.grad) for g in flat] for w in self.workers}
        self._recv_buf = {w: [torch.empty_like(b) for b in _buffers(flat)] for w in self.workers}
        self._snap = {w: [torch.empty_like(t) for t in _group_payload_params(flat)] for w in self.workers}
        self._send_works = {w: [] for w in self.workers}
        self.global_step = int(global_step)
        self.steps = []
        self.contributed = {w: 0 for w in self.workers}
        self.dropped = {w: 0 for w in self.workers}
        self.lost = []
        self._pending = []
        self._stopping = False
        # parallel/ps_ckpt.py::PSCheckpointer: restart from the directory's latest checkpoint (the workers get the
        # restored global step with their initial pull), then checkpoint after a closed step when one is due
        self.ckpt = checkpointer
        self.restored_step = None
        if checkpointer is not None:
            self.restored_step = checkpointer.restore_latest()
            if self.restored_step is not None:
                self.global_step = self.restored_step

    def _answer(self, w, accepted, stop=False):
        """The current parameters (a snapshot of this worker's own) and the verdict."""
        _wait_all(self._send_works[w])  # the snapshot buffer is about to be overwritten (stream wait)
        snap = self._snap[w]
        for s, p in zip(snap, _group_payload_params(self.flat)):
            s.copy_(p)
        self._send_works[w] = [_isend(s, w, self.pg) for s in snap]
        self._ctl.reply(w, self.global_step, accepted, stop)

    @traced("dtg.sps.apply")
    def _close_step(self):
        ws = self._pending
        self._pending = []
        inv = 1.0 / len(ws)
        self.opt.step_sum([self._recv[w] for w in ws], grad_scale=inv)
        # running statistics: the mean of the contributors' updates since their pull
        for i, b in enumerate(_buffers(self.flat)):
            deltas = [self._recv_buf[w][i] for w in ws]
            for c in range(0, len(deltas), K.MAX_SRCS):
                K.grad_sum(b, deltas[c:c + K.MAX_SRCS], first=False, scale=inv)
        self.global_step += 1
        self.steps.append(tuple(ws))
        for w in ws:
            self.contributed[w] += 1
        for w in ws:
            self._answer(w, True)
        if self.ckpt is not None:
            self.ckpt.maybe_save(self.global_step)  # enqueues on the apply stream, never waits
        if fault.kill_ps_step() is not None:
            fault.maybe_kill_gpu_ps(self.global_step)

    def _push(self, w, local_step):
        # the receive is always posted (the send is already on the wire) and from the apply (current) stream, so
        # the pair stream first waits for the previous kernel that read these buffers
        _wait_all([_irecv(b, w, self.pg) for b in self._recv[w] + self._recv_buf[w]])
        if self._stopping:
            self.dropped[w] += 1
            self._answer(w, False, stop=True)
        elif local_step != self.global_step:
            self.dropped[w] += 1
            self._answer(w, False)
        else:
            self._pending.append(w)
            if len(self._pending) == self.R:
                self._close_step()

    def _check_quorum(self, live):
        """Fewer than R live workers: no step can close any more -- release whoever waits."""
        if self._stopping or len(live) >= self.R:
            return
        self._stopping = True
        for w in self._pending:
            self.dropped[w] += 1
            self._answer(w, False, stop=True)
        self._pending = []

    def _sync(self):
        if self.dev.type == "cuda":
            torch.cuda.current_stream(self.dev).synchronize()

    def serve(self):
        """Serve pushes in arrival order until every worker is done or lost; returns ``len(self.steps)``."""
        live = set(self.workers)
        for w in self.workers:
            self._answer(w, False)  # the initial pull: parameters + their version
        while live:
            tok = self._ctl.next(self.worker_timeout)
            if tok is None:
                raise TimeoutError("sync PS: no request from workers %s in %.0f s" % (sorted(live),
                                                                                      self.worker_timeout))
            if tok < 0:
                w = -tok - 1
                if w in live:
                    live.discard(w)
                    self.lost.append(w)
                    if w in self._pending:
                        self._pending.remove(w)
                    print("[dtg.sync_ps] worker rank %d lost (its control connection closed); continuing with %s"
                          % (w, sorted(live)), file=sys.stderr, flush=True)
                    self._check_quorum(live)
                continue
            w, kind, local_step = _SyncControl.decode(tok)
            if kind == _DONE:
                live.discard(w)
                self._check_quorum(live)
            elif kind == _GRAD and w in live:
                self._push(w, local_step)
        for w in self.workers:
            if w not in self.lost:
                _wait_all(self._send_works[w])
            self._send_works[w] = []
        self._sync()
        if self.ckpt is not None:
            self.ckpt.flush(self.global_step)
        return len(self.steps)

    def summary(self):
        """The PS's one-line report."""
        return "[ps] %d steps, contributed %s, dropped %s, lost %s" % (len(self.steps), dict(self.contributed),
                                                                      dict(self.dropped), list(self.lost))

    def close(self):
        self._ctl.close()
