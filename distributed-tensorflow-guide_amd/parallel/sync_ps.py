"""Synchronous parameter server with backup workers for FlatParams models (ResNet-50, BERT, MNIST).

The reference defines synchronous SGD as "aggregate N of M gradients, drop the M - N stale ones"
(``Synchronous-SGD/README.md:3``, ``ssgd.py:51-60``: ``SyncReplicasOptimizer(replicas_to_aggregate=N,
total_num_replicas=M)``).  For the toy graph dtg keeps that in the C++ PS accumulators (csrc/ps/server.cc
ACC_*); this module is the GPU form: one PS rank owns the parameters in HBM, M workers push gradients, a
global step closes as soon as R = ``replicas_to_aggregate`` FRESH gradients have arrived, and the M - R
gradients that arrive late (computed on an older parameter version) are dropped.

Everything that moves bytes is parallel/ps_core.py's, shared with the async PS: pair-wise RCCL send/recv (gloo with
host staging for one-card rehearsals and CPU tests), the native control channel, the announcer thread that releases
a request token only once the gradient exists on the device, per-worker receive and snapshot buffers, lost-worker
detection through the watched control connection, the ``serve()`` loop.  Here are the protocol and the PS-side
reduce + apply.

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

from ..ops import optim_kernels as K
from ..utils.trace import traced
from .ps_core import (_GRAD, _KINDS, _Control, _buffers, _group_payload_grads, _group_payload_params, _irecv, _isend,
                      _PSServer, _PSWorker, _ready_event, _wait_all, init_from_cluster)  # noqa: F401

_SREQ = "dtg.sps.req"
_STEP_SHIFT = 24  # token = local_step << 24 | rank * _KINDS + kind


def _reply_queue(rank):
    return "dtg.sps.rep.%d" % rank


class _SyncControl(_Control):
    """The control channel on a request queue of its own, with the step in the token and one reply
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


class SyncPSWorker(_PSWorker):
    """Worker side.  ``begin()`` pulls the initial parameters and their version, ``step_done()`` after every
    backward pushes the gradient and waits for the PS's answer (True if it was aggregated, False if it was dropped
    as stale or the job is stopping), ``finish()`` tells the PS this worker is done.  Under a session
    (``minimize``) the graph ``global_step`` is SET to the step the PS returned, so ``StopAtStepHook(last_step=N)``
    stops every worker at global step N -- a backup worker whose last push was dropped included; when the PS
    answers ``stop`` the train op requests the session's stop."""

    _control = _SyncControl
    _op_name = "sync_ps_train"

    def __init__(self, flat, ps_rank=0, group=None, timeout=None):
        super().__init__(flat, ps_rank, group)
        self.timeout = float(timeout) if timeout is not None else _sync_timeout()
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
        payload = list(grads) + self._buffer_delta()
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

    def _step_global(self, global_step, session):
        if global_step is not None:
            with global_step._lock:
                global_step._local.fill_(self.global_step)
        if self.stopped and session is not None:
            session.request_stop()


class SyncPSServer(_PSServer):
    """PS side: ``serve()`` runs until every worker sent DONE (or was lost); returns the number of global steps.

    Counters: ``contributed[w]`` / ``dropped[w]`` per worker, ``steps`` (the contributor tuple of every global
    step, in the order their gradients were summed), ``lost``."""

    _mode = "sync"
    _control = _SyncControl

    def __init__(self, flat, optimizer, workers, replicas_to_aggregate, group=None, worker_timeout=None,
                 global_step=0, checkpointer=None):
        workers = list(workers)
        self.R = int(replicas_to_aggregate)
        if not 1 <= self.R <= len(workers):
            raise ValueError("replicas_to_aggregate=%d with %d worker(s)" % (self.R, len(workers)))
        super().__init__(flat, optimizer, workers, group, worker_timeout, checkpointer)
        # after a restart the global step continues from the checkpoint (the workers get it with their initial pull)
        self.global_step = int(global_step) if self.restored_step is None else self.restored_step
        self.steps = []
        self.contributed = {w: 0 for w in self.workers}
        self.dropped = {w: 0 for w in self.workers}
        self._pending = []
        self._stopping = False

    def _send_params(self, w, accepted=False, stop=False):
        """The current parameters (a snapshot of this worker's own) and the verdict; the initial pull (no
        verdict yet) carries the parameters' version the same way."""
        super()._send_params(w)
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
            self._send_params(w, True)
        self._checkpoint(self.global_step)

    def _push(self, w, local_step):
        self._recv_push(w)  # always: the send is already on the wire
        if self._stopping:
            self.dropped[w] += 1
            self._send_params(w, False, stop=True)
        elif local_step != self.global_step:
            self.dropped[w] += 1
            self._send_params(w, False)
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
            self._send_params(w, False, stop=True)
        self._pending = []

    def _lost(self, w, live):
        if w in self._pending:
            self._pending.remove(w)
        self._check_quorum(live)

    def _done(self, w, live):
        self._check_quorum(live)

    def _request(self, w, kind, local_step, live):
        if kind == _GRAD and w in live:
            self._push(w, local_step)

    def _finish(self):
        self._flush(self.global_step)
        return len(self.steps)

    def summary(self):
        """The PS's one-line report."""
        return "[ps] %d steps, contributed %s, dropped %s, lost %s" % (len(self.steps), dict(self.contributed),
                                                                      dict(self.dropped), list(self.lost))
