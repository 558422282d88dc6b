"""What the GPU parameter servers share: the transport between one PS rank and its workers, and the server and
worker base classes that the asynchronous (parallel/async_ps.py) and the synchronous (parallel/sync_ps.py) PS build
their protocols on.

One PS rank keeps the parameters in HBM; workers push gradients and pull parameters with point-to-point RCCL
send/recv (``torch.distributed`` "nccl" backend = RCCL over xGMI; "gloo" on the CPU for tests).

Transport:

* **payloads** go over RCCL point-to-point: torch's RCCL process group gives every PS<->worker pair its
  own 2-rank communicator and HIP stream, so the pairs move gradients and parameters concurrently.  With
  one process per GPU and every device visible to every process (examples/ResNet50/run_async.sh,
  ``bench.py --mode async_ps``) each pair is a distinct GPU pair, which on MI355X's fully connected xGMI
  mesh has a direct link of its own (7 per GPU); that the 7 transfers then run link-parallel has not been
  traced on an 8-GPU node yet (the one-card rehearsals stage through host memory over gloo).  A push is one
  send per dtype group (bf16 compute grads, fp32 norm/bias grads, the BN running-statistics delta); a pull
  is the bf16 compute mirror, the fp32 group and the module buffers.
* **request framing** goes over dtg's native TCP service (csrc/ps/server.cc, the same one the CPU PS
  uses): a worker enqueues a (rank, kind) token on one queue and the PS blocks in ``q_dequeue`` with
  the GIL released.  So the PS serves requests in arrival order with no busy spin and no device
  synchronisation: its host loop only enqueues GPU work (post the receive, make the apply stream wait
  for it, apply with the fused HIP optimizer kernel, snapshot, send), all ordered by streams and events.
* **failure detection**: each worker's control connection carries a watch (``PSClient.watch``); if the
  worker process dies, the service enqueues its "lost" token and ``serve()`` finishes with the
  survivors (``lost`` lists who dropped out).  ``worker_timeout`` bounds how long the PS waits with no
  request from any live worker (TimeoutError naming them).  A worker that dies in the middle of a
  transfer leaves an RCCL kernel waiting on its pair stream; RCCL communicators cannot shrink, so that
  case is fail-stop (the other workers' pulls stall and the PS times out), like sync DP.
* **GPU-ready request order**: a worker's host enqueues a step long before its GPU has the gradient.  Its
  request token therefore goes out from a small announcer thread only once a device event recorded after the
  gradient has completed (:class:`_Announcer`), so the PS -- which posts the receive and makes its apply stream
  wait for it as soon as it dequeues a token -- serves workers in the order their gradients EXIST, never
  stalls its apply stream behind a worker that is still in backward, and fast workers take proportionally
  more updates than a slow one (``test_async_ps_slow_worker_does_not_hold_back_fast_ones``).

Base classes: :class:`_PSServer` owns the per-worker receive / snapshot buffers, the checkpoint restore and the
``serve()`` loop (initial send, blocking dequeue, lost workers, final drain, flush); a server adds how it decodes a
token and what a request, a lost worker and a finished worker mean to it.  :class:`_PSWorker` owns the control
connection, the announcer, the BN running-statistics bookkeeping, ``finish()`` and the session surface (one train
op, :class:`_PSApply`, and one hook, :class:`_PSHook`).
"""
import os
import queue
import sys
import threading

import torch
import torch.distributed as dist

from .. import fault
from ..graph import Op
from ..train.hooks import SessionRunHook

_GRAD, _DONE, _ELASTIC, _WARM = 1, 2, 3, 4
_KINDS = 16
_REQ = "dtg.aps.req"
_instances = [0]  # per-process count of control objects: the same on every rank (construction order)


# gloo moves CPU tensors only for point-to-point; with DTG_BACKEND=gloo DTG_GLOO_DEVICE=cuda (the
# one-card rehearsal of this GPU path, see parallel/comm.py) device tensors are staged through host
# memory.  RCCL sends/receives HBM buffers directly; these helpers are then plain dist calls.
def _staged(t, group):
    return t.is_cuda and dist.get_backend(group) == "gloo"


class _HostSend:
    """isend of a host copy; keeps the copy alive until wait()."""

    def __init__(self, t, dst, group):
        self._h = t.cpu()
        self._w = dist.isend(self._h, dst=dst, group=group)

    def wait(self):
        self._w.wait()
        self._h = None


class _HostRecv:
    """irecv into a host buffer; wait() lands it in the device tensor."""

    def __init__(self, t, src, group):
        self._t = t
        self._h = torch.empty_like(t, device="cpu")
        self._w = dist.irecv(self._h, src=src, group=group)

    def wait(self):
        self._w.wait()
        self._t.copy_(self._h)
        self._h = None


def _isend(t, dst, group=None):
    return _HostSend(t, dst, group) if _staged(t, group) else dist.isend(t, dst=dst, group=group)


def _irecv(t, src, group=None):
    """Post a receive.  RCCL: ``wait()`` makes the CURRENT stream wait for it (no host block)."""
    return _HostRecv(t, src, group) if _staged(t, group) else dist.irecv(t, src=src, group=group)


def _wait_all(works):
    for w in works:
        w.wait()


def _group_payload_grads(flat):
    return [g.grad for g in flat]


def _buffers(flat):
    fb = getattr(flat, "buffers", None)
    return [fb.flat] if fb is not None else []


def _group_payload_params(flat):
    # what the model reads: the bf16 mirror of the compute group, the fp32 master of the fp32 group,
    # and the module buffers (BN running statistics: PS variables in the reference's TF setup)
    return [g.mirror if g.mirror is not None else g.master for g in flat] + _buffers(flat)


def _elastic_state(flat):
    return [g.master for g in flat] + _buffers(flat)


class _Control:
    """Request framing between the PS rank and its workers over the native TCP service.  The PS hosts it
    and publishes its address in the process group's store; workers connect and watch their connection."""

    def __init__(self, is_ps, rank, queue=_REQ):
        from .. import _runtime
        from . import comm
        # a lost worker is survivable here (serve() continues with the rest): the fail-stop rank watchdog that
        # comm.init starts for multi-rank jobs would instead end every rank DTG_RANK_TIMEOUT after the loss
        comm.stop_watchdog()
        _instances[0] += 1
        key = "dtg.aps.ctl.%d" % _instances[0]
        store = dist.distributed_c10d._get_default_store()
        self.svc = None
        self.key = key
        self.queue = queue  # the request queue (the sync PS, parallel/sync_ps.py, frames on one of its own)
        if is_ps:
            host = os.environ.get("MASTER_ADDR", "127.0.0.1")
            bind = "127.0.0.1" if host in ("127.0.0.1", "localhost") else "0.0.0.0"
            self.svc = _runtime.PSServer(bind, 0, 0)
            self.svc.start()
            self.addr = ("127.0.0.1", self.svc.port)
            self.cli = _runtime.PSClient("127.0.0.1", self.svc.port, 60.0)
            store.set(key, "%s:%d" % ("127.0.0.1" if bind == "127.0.0.1" else host, self.svc.port))
        else:
            addr = store.get(key).decode()
            h, p = addr.rsplit(":", 1)
            self.addr = (h, int(p))
            self.cli = _runtime.PSClient(h, int(p), 60.0)
            self.cli.watch(queue, -(rank + 1))  # dies with the process -> the PS sees a lost token

    def request(self, rank, kind):
        self.cli.q_enqueue(self.queue, [rank * _KINDS + kind])

    @staticmethod
    def decode(tok):
        """(rank, kind, argument) of a request token; these tokens carry no argument."""
        return divmod(tok, _KINDS) + (0,)

    def next(self, timeout):
        return self.cli.q_dequeue(self.queue, -1.0 if timeout is None else float(timeout))

    def unwatch(self):
        self.cli.unwatch()

    def finish(self, rank):
        """A worker's last request: stop the watch, send DONE, close."""
        self.unwatch()
        try:
            self.request(rank, _DONE)
        except RuntimeError as e:
            # the last worker's DONE lets the PS leave serve() and close its control service; the service can go
            # down before the reply to that enqueue is flushed.  A lost connection here loses nothing: this worker
            # has no further requests, and a PS that died earlier already failed the pushes above.
            if "connection lost" not in str(e):
                raise
        self.close()

    def close(self):
        if self.cli is not None:
            self.cli.close()
            self.cli = None
        if self.svc is not None:
            self.svc.stop()
            self.svc = None


class _Announcer:
    """Sends a worker's request tokens from a background thread, each only after the device event it carries
    has completed (None: at once), in submission order.  The worker's host thread never blocks on its own GPU
    for this, and the PS sees a gradient's token only when the gradient is on the device."""

    def __init__(self, ctl):
        self._ctl = ctl
        self._q = queue.Queue()
        self.error = None
        self._t = threading.Thread(target=self._run, name="dtg-aps-announce", daemon=True)
        self._t.start()

    def _run(self):
        while True:
            item = self._q.get()
            if item is None:
                return
            rank, kind, ev = item
            try:
                if ev is not None:
                    ev.synchronize()
                self._ctl.request(rank, kind)
            except Exception as e:  # surfaced by the next submit()/close()
                self.error = e
                return

    def _check(self):
        if self.error is not None:
            raise RuntimeError("async PS request announcer failed") from self.error

    def submit(self, rank, kind, event=None):
        self._check()
        self._q.put((rank, kind, event))

    def close(self):
        """Flush every queued token (in order) and stop the thread."""
        self._q.put(None)
        self._t.join()
        self._check()


def _ready_event(tensors):
    """A device event after the work that produces ``tensors`` (None for host tensors)."""
    t = next((t for t in tensors if t.is_cuda), None)
    if t is None:
        return None
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(t.device))
    return ev


class _PSServer:
    """PS side of both servers: the per-worker buffers, the checkpoint restore and the ``serve()`` loop.  A
    subclass sets ``_mode`` ("async" / "sync": the prefix of its error and log lines) and ``_control``, and
    implements :meth:`_request`, :meth:`_finish` and, where it needs them, :meth:`_lost` and :meth:`_done`."""

    _mode = None
    _control = _Control

    def __init__(self, flat, optimizer, workers, group=None, worker_timeout=None, checkpointer=None):
        self.flat = flat
        self.opt = optimizer
        self.workers = list(workers)
        self.pg = group
        self.worker_timeout = worker_timeout if worker_timeout is not None else float(
            os.environ.get("DTG_PS_WORKER_TIMEOUT", "600"))
        self.dev = next(iter(flat)).master.device
        self._ctl = self._control(True, dist.get_rank())
        self._recv = {w: [torch.empty_like(g.grad) for g in flat] for w in self.workers}
        self._recv_buf = {w: [torch.empty_like(b) for b in _buffers(flat)] for w in self.workers}
        self._snap = {w: [torch.empty_like(t) for t in _group_payload_params(flat)] for w in self.workers}
        self._send_works = {w: [] for w in self.workers}
        self.lost = []
        # parallel/ps_ckpt.py::PSCheckpointer: restart from the directory's latest checkpoint (the subclass continues
        # its counters from ``restored_step``), then checkpoint after an update when one is due
        self.ckpt = checkpointer
        self.restored_step = checkpointer.restore_latest() if checkpointer is not None else None

    def _checkpoint(self, step, extra=None):
        if self.ckpt is not None:
            self.ckpt.maybe_save(step, extra)  # enqueues on the apply stream, never waits
        if fault.kill_ps_step() is not None:
            fault.maybe_kill_gpu_ps(step)

    def _flush(self, step, extra=None):
        if self.ckpt is not None:
            self.ckpt.flush(step, extra)

    def _recv_push(self, w):
        # the receive is posted (the send is already on the wire) from the apply (current) stream, so RCCL's pair
        # stream first waits for the previous kernel that read these buffers; the apply then waits for the receive
        # (stream events only).  The worker sent this token only once its gradient was on its device (_Announcer),
        # so the receive completes as soon as the pair's transfer does.
        _wait_all([_irecv(b, w, self.pg) for b in self._recv[w] + self._recv_buf[w]])

    def _send_params(self, w):
        """Snapshot the current parameters into this worker's own buffers and send them to it."""
        _wait_all(self._send_works[w])  # the snapshot buffer is about to be overwritten (stream wait)
        snap = self._snap[w]
        for s, p in zip(snap, _group_payload_params(self.flat)):
            s.copy_(p)
        self._send_works[w] = [_isend(s, w, self.pg) for s in snap]

    def _sync(self):
        """Wait for the apply stream only: a device-wide synchronize would also wait on every pair stream,
        and a parameter send to a worker that was lost mid-run never completes with RCCL (those sends are
        deliberately left unjoined)."""
        if self.dev.type == "cuda":
            torch.cuda.current_stream(self.dev).synchronize()

    def _request(self, w, kind, arg, live):
        """Serve worker ``w``'s request ``kind`` (anything but DONE); ``arg`` is what its token carried."""
        raise NotImplementedError

    def _lost(self, w, live):
        """Worker ``w`` was just lost (it is already out of ``live`` and in ``lost``)."""

    def _done(self, w, live):
        """Worker ``w`` just finished (it is already out of ``live``)."""

    def _finish(self):
        """After the final drain and ``_sync()``: :meth:`_flush` this server's step; returns what ``serve()``
        returns."""
        raise NotImplementedError

    def serve(self):
        """Serve requests in arrival order until every worker is done or lost.  The loop blocks in the native
        queue and never polls."""
        live = set(self.workers)
        for w in self.workers:
            self._send_params(w)  # the initial pull
        while live:
            tok = self._ctl.next(self.worker_timeout)
            if tok is None:
                raise TimeoutError("%s PS: no request from workers %s in %.0f s" % (self._mode, sorted(live),
                                                                                    self.worker_timeout))
            if tok < 0:
                w = -tok - 1
                if w in live:
                    live.discard(w)
                    self.lost.append(w)
                    print("[dtg.%s_ps] worker rank %d lost (its control connection closed); continuing with %s"
                          % (self._mode, w, sorted(live)), file=sys.stderr, flush=True)
                    self._lost(w, live)
                continue
            w, kind, arg = self._ctl.decode(tok)
            if kind == _DONE:
                live.discard(w)
                self._done(w, live)
            else:
                self._request(w, kind, arg, live)
        for w in self.workers:
            if w not in self.lost:
                _wait_all(self._send_works[w])
            self._send_works[w] = []
        self._sync()
        return self._finish()

    def close(self):
        self._ctl.close()


class _PSWorker:
    """Worker side of both servers: the control connection and its announcer, the module buffers as pulled (the
    push carries current - pulled, the worker's running-statistics update since the pull), ``finish()`` and the
    session surface.  A subclass sets ``_control`` and ``_op_name`` and implements ``begin()``, ``step_done()``
    and :meth:`_step_global`."""

    _control = _Control
    _op_name = None

    def __init__(self, flat, ps_rank=0, group=None):
        self.flat = flat
        self.ps = ps_rank
        self.pg = group
        self.rank = dist.get_rank()
        self._ctl = self._control(False, self.rank)
        self._ann = _Announcer(self._ctl)
        self._buf0 = [torch.empty_like(b) for b in _buffers(flat)]
        self._bufd = [torch.empty_like(b) for b in _buffers(flat)]

    def _pulled(self):
        """Remember the module buffers as they were pulled."""
        for b0, b in zip(self._buf0, _buffers(self.flat)):
            b0.copy_(b)

    def _buffer_delta(self):
        """The module buffers' change since the pull, as the push sends it."""
        for d, b, b0 in zip(self._bufd, _buffers(self.flat), self._buf0):
            torch.sub(b, b0, out=d)
        return self._bufd

    def _step_global(self, global_step, session):
        """After a ``step_done()`` of the train op: advance the graph ``global_step`` (None: there is none) the
        way this mode counts, and ask ``session`` (None: do not) to stop when the job is over."""
        raise NotImplementedError

    # ---- session surface (train/eager.py): the reference's worker loop, sess.run(train_op) under a session ----------
    def minimize(self, loss_fn, global_step=None, inputs=(), name=None):
        """A train op for ``sess.run``: forward + backward of ``loss_fn(*inputs)``, then ``step_done()`` and
        :meth:`_step_global` -- the worker loop of /root/reference/Hogwild/Hogwild.py:44-57 and
        DOWNPOUR/DOWNPOUR.py:116-140 with the parameters in the PS's HBM."""
        from ..train.eager import EagerGradients
        name = name or self._op_name
        return _PSApply(EagerGradients(loss_fn, inputs, name + "/gradients"), self, global_step, name)

    def make_session_run_hook(self):
        """after_create_session: the initial pull (``begin()``); end: :meth:`finish` (the PS's ``serve()``
        returns once every worker finished, the ``Server.join()`` of the reference's PS task)."""
        return _PSHook(self)

    def finish(self):
        self._ann.close()  # every queued token is out before DONE
        self._ctl.finish(self.rank)


class _PSApply(Op):
    """The worker's train op (_PSWorker.minimize)."""

    def __init__(self, grads, worker, global_step, name):
        self.grads, self.worker, self.global_step = grads, worker, global_step
        super().__init__(lambda c, *a: None, [grads], name)

    def _eval(self, ctx):
        ctx.eval(self.grads)
        self.worker.step_done()
        self.worker._step_global(self.global_step, ctx.session)
        return None

    @property
    def loss(self):
        """The step's loss as a fetchable tensor (fetching it synchronises the device)."""
        return self.grads


class _PSHook(SessionRunHook):
    """_PSWorker.make_session_run_hook: initial pull once the session exists, finish() at its end.  With a graph
    ``global_step`` (train/sync_replicas.py) that starts at the step the pull came with."""

    def __init__(self, worker, global_step=None):
        self.worker = worker
        self.global_step = global_step
        self._begun = False

    def after_create_session(self, session, coord):
        if not self._begun:
            self.worker.begin()
            self._begun = True
            if self.global_step is not None:
                self.worker._step_global(self.global_step, None)

    def end(self, session):
        if self._begun:
            self.worker.finish()
            self._begun = False


def init_from_cluster(cluster, job_name, task_index, backend=None, port_offset=1):
    """Bootstrap the RCCL/gloo process group from a TF-style ClusterSpec: the PS task 0 is rank 0
    (its ``host:port`` + ``port_offset`` is the rendezvous), worker i is rank 1 + i.  One process per
    GPU: rank r uses device r % (visible devices), with every device left visible to every process
    (examples/ResNet50/run_async.sh) -- RCCL can only use the direct xGMI peer links between GPUs a process
    can see, so pinning each process to one device with HIP_VISIBLE_DEVICES would hide its peers.  On one
    card (the gloo rehearsal) every rank lands on device 0.  Returns (rank, world, device)."""
    import datetime

    spec = cluster.as_dict() if hasattr(cluster, "as_dict") else dict(cluster)
    ps_host, ps_port = spec["ps"][0].rsplit(":", 1)
    n_workers = len(spec["worker"])
    rank = 0 if job_name == "ps" else 1 + int(task_index)
    world = 1 + n_workers
    backend = os.environ.get("DTG_BACKEND") or backend
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    gloo_cuda = backend == "gloo" and os.environ.get("DTG_GLOO_DEVICE") == "cuda" and torch.cuda.is_available()
    if backend == "nccl" or gloo_cuda:
        device = torch.device("cuda", rank % max(1, torch.cuda.device_count()))
    else:
        device = torch.device("cpu")
    if device.type == "cuda":
        torch.cuda.set_device(device)
    os.environ["MASTER_ADDR"] = "127.0.0.1" if ps_host in ("localhost", "") else ps_host
    os.environ["MASTER_PORT"] = str(int(ps_port) + port_offset)
    kw = {"device_id": device} if backend == "nccl" else {}
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=600), **kw)
    return rank, world, device
