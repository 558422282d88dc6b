"""Synchronous PS with backup workers (parallel/sync_ps.py) exercised with gloo ranks on the CPU: fp32 compute, a
fixed batch per worker (so a replay depends on the PS's step log alone), every process under a timeout.

* 1 PS + 3 workers, R = 2, one slow worker: every step has 2 distinct contributors, the slow worker's stale
  pushes are dropped, and the PS parameters equal a replay of the logged steps;
* R = M = 2 equals the all-reduce mode (a DataParallel loop);
* a worker that dies (M = 3, R = 2) is survived; a worker that finishes early (M = R = 2) stops the other; a worker
  that stays silent makes ``serve()`` time out naming it;
* the SyncReplicasOptimizer surface: R < M without ``ps_rank`` is refused as before, with it the session-driven
  example runs to ``--steps`` global steps.
"""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 0.1


def _model():
    import dtg  # noqa: F401
    from dtg.models.layers import Linear

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = Linear(8, 16, act="relu")
            self.b = Linear(16, 3)

        def forward(self, x):
            return self.b(self.a(x))
    torch.manual_seed(0)
    return M()


def _data(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(32, 8, generator=g), torch.randint(0, 3, (32,), generator=g)


def _rank(rank, world, port, q, R, steps, momentum=0.0, sleep=None, die=None, max_pushes=None, worker_timeout=None,
          silent=None):
    """Rank 0: the PS.  Workers push until the PS reports global step ``steps`` (or stop).  ``sleep``: {rank:
    seconds per gradient}; ``die`` = (rank, pushes): that worker vanishes (os._exit) after so many pushes;
    ``max_pushes``: {rank: n}, that worker finishes after n pushes; ``silent``: that worker pulls and then sends
    nothing, alive for as long as the PS is; ``worker_timeout``: the PS's, and a TimeoutError of its ``serve()``
    is reported as its result."""
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank), DTG_SYNC_TIMEOUT="60", DTG_PS_WORKER_TIMEOUT="60")
        import time
        import dtg  # noqa: F401
        from dtg import ops
        from dtg.optim import FusedSGD
        from dtg.parallel import FlatParams, comm
        from dtg.parallel.sync_ps import SyncPSServer, SyncPSWorker
        comm.init("gloo")
        model = _model()
        flat = FlatParams(model, compute_dtype=torch.float32)
        if rank == 0:
            ps = SyncPSServer(flat, FusedSGD(flat, lr=LR, momentum=momentum), workers=range(1, world),
                              replicas_to_aggregate=R, worker_timeout=worker_timeout)
            try:
                n = ps.serve()
            except TimeoutError as e:
                q.put((rank, "ok", {"timeout": str(e)}))
                q.close()
                q.join_thread()  # flush before the hard exit
                os._exit(0)
            # numpy payloads: torch CPU tensors would travel by fd-sharing, which races the child's exit
            q.put((rank, "ok", {"n": n, "steps": list(ps.steps), "contributed": dict(ps.contributed),
                                "dropped": dict(ps.dropped), "lost": list(ps.lost), "line": ps.summary(),
                                "w": [g.master.clone().numpy() for g in flat]}))
            ps.close()
        else:
            w = SyncPSWorker(flat, ps_rank=0)
            w.begin()
            if rank == silent:
                q.put((rank, "ok", {"silent": True}))
                q.close()
                q.join_thread()
                try:
                    w._ctl.wait_reply(60)  # no reply ever comes: returns when the PS, gone, drops the connection
                except RuntimeError:
                    pass
                os._exit(0)
            x, y = _data(rank)
            losses = []
            while w.global_step < steps and not w.stopped:
                if max_pushes and w.pushes >= max_pushes.get(rank, 1 << 30):
                    break
                loss = ops.softmax_cross_entropy(model(x), y)
                loss.backward()
                if sleep and rank in sleep:
                    time.sleep(sleep[rank])  # this worker's gradient takes that much longer to exist
                w.step_done()
                losses.append(loss.item())
                if die is not None and rank == die[0] and w.pushes == die[1]:
                    q.put((rank, "ok", {"died": True}))
                    q.close()
                    q.join_thread()
                    os._exit(3)  # no finish(), no shutdown: the process just disappears
            w.finish()
            q.put((rank, "ok", {"pushes": w.pushes, "contributed": w.contributed, "dropped": w.dropped,
                                "stopped": w.stopped, "global_step": w.global_step, "losses": losses}))
        comm.shutdown()
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc(), None))
        raise


def _run(world, **kw):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _cluster import free_ports
    port = free_ports(1)[0]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q), kwargs=kw) for r in range(world)]
    for p in procs:
        p.start()
    out = {}
    try:
        for _ in range(world):
            r, status, payload = q.get(timeout=120)
            assert status == "ok", status
            out[r] = payload
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    return out


def _ps_params_by_name(ws):
    import dtg  # noqa: F401
    from dtg.parallel import FlatParams
    model = _model()
    flat = FlatParams(model, compute_dtype=torch.float32)
    for g, w in zip(flat, ws):
        g.master.copy_(torch.as_tensor(w))
    return {n: v.clone() for n, v in flat.named_masters()}


def _replay(steps):
    """Plain SGD over the PS's step log: every contributor of a step computed its gradient on that step's
    parameters (it was fresh) and on its own fixed batch; the gradients are summed in the logged order, scaled
    by 1/R and applied."""
    import dtg  # noqa: F401
    from dtg import ops
    model = _model()
    params = list(model.parameters())
    for contributors in steps:
        total = None
        for w in contributors:
            x, y = _data(w)
            grads = torch.autograd.grad(ops.softmax_cross_entropy(model(x), y), params)
            total = [g.clone() for g in grads] if total is None else [t + g for t, g in zip(total, grads)]
        with torch.no_grad():
            for p, t in zip(params, total):
                p.sub_(LR * (t * (1.0 / len(contributors))))
    return {n: p.detach() for n, p in model.named_parameters()}


def test_sync_ps_backup_worker_is_dropped_and_steps_replay():
    N, R = 10, 2
    out = _run(4, R=R, steps=N, sleep={1: 0.05, 2: 0.05, 3: 0.25})
    ps = out[0]
    assert ps["n"] == N and len(ps["steps"]) == N and ps["lost"] == []
    for c in ps["steps"]:
        assert len(c) == R and len(set(c)) == R and set(c) <= {1, 2, 3}
    for w in (1, 2, 3):
        assert out[w]["contributed"] + out[w]["dropped"] == out[w]["pushes"], out[w]
        assert ps["contributed"][w] == out[w]["contributed"] == sum(w in c for c in ps["steps"])
        assert ps["dropped"][w] == out[w]["dropped"]
        assert out[w]["global_step"] == N
    assert ps["dropped"][3] >= 1
    assert re.match(r"\[ps\] 10 steps, contributed \{.*\}, dropped \{.*\}, lost \[\]$", ps["line"]), ps["line"]
    got = _ps_params_by_name(ps["w"])
    ref = _replay(ps["steps"])
    for n, v in ref.items():
        assert torch.allclose(got[n], v, atol=1e-5), (n, (got[n] - v).abs().max())


def _dp_rank(rank, world, port, q, steps, momentum):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        import dtg  # noqa: F401
        from dtg import ops
        from dtg.optim import FusedSGD
        from dtg.parallel import DataParallel, FlatParams, comm
        comm.init("gloo")
        model = _model()
        flat = FlatParams(model, compute_dtype=torch.float32)
        dp = DataParallel(flat)
        dp.broadcast_parameters(0)
        opt = FusedSGD(flat, lr=LR, momentum=momentum)
        x, y = _data(rank + 1)  # the batches of PS workers 1 and 2
        for _ in range(steps):
            ops.softmax_cross_entropy(model(x), y).backward()
            dp.step(opt)
        q.put((rank, "ok", {"w": [g.master.clone().numpy() for g in flat]}))
        comm.shutdown()
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc(), None))
        raise


def test_sync_ps_all_replicas_equals_allreduce_mode():
    """R = M = 2: nobody is ever stale, so the PS computes what the all-reduce mode does.  Within
    test_optim_apply's tolerance; in fact bit-equal here -- the sum of two gradients does not depend on their
    arrival order, and both paths scale it by 1/2 inside the same apply rule."""
    N = 6
    out = _run(3, R=2, steps=N, momentum=0.9)
    assert out[0]["n"] == N and out[0]["dropped"] == {1: 0, 2: 0}
    assert out[1]["contributed"] == out[2]["contributed"] == N
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _cluster import free_ports
    port = free_ports(1)[0]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_rank, args=(r, 2, port, q, N, 0.9)) for r in range(2)]
    for p in procs:
        p.start()
    ref = {}
    try:
        for _ in range(2):
            r, status, payload = q.get(timeout=120)
            assert status == "ok", status
            ref[r] = payload
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for a, b in zip(out[0]["w"], ref[0]["w"]):
        a, b = torch.as_tensor(a), torch.as_tensor(b)
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), (a - b).abs().max()


def test_sync_ps_survives_a_dead_worker():
    """M = 3, R = 2, worker 3 vanishes after 2 pushes: the survivors reach N global steps, ``lost`` names it."""
    N = 8
    out = _run(4, R=2, steps=N, sleep={1: 0.02, 2: 0.02, 3: 0.02}, die=(3, 2))
    assert out[3] == {"died": True}
    ps = out[0]
    assert ps["n"] == N and ps["lost"] == [3]
    for c in ps["steps"]:
        assert len(set(c)) == 2
    for w in (1, 2):
        assert out[w]["global_step"] == N and not out[w]["stopped"]


def test_sync_ps_early_finisher_stops_the_rest():
    """M = R = 2 and worker 2 finishes after 3 pushes: no step can close any more, so worker 1's pending push is
    answered with stop and everything exits (well within the timeouts)."""
    out = _run(3, R=2, steps=50, max_pushes={2: 3})
    assert out[0]["n"] == 3 and out[0]["lost"] == []
    assert out[2]["pushes"] == 3 and out[2]["contributed"] == 3 and not out[2]["stopped"]
    assert out[1]["stopped"] and out[1]["contributed"] == 3 and out[1]["global_step"] == 3
    assert out[1]["contributed"] + out[1]["dropped"] == out[1]["pushes"] == 4


def test_sync_ps_worker_timeout_names_silent_workers():
    """A worker that pulls and then stays silent: ``serve()`` gives up after ``worker_timeout`` and names it."""
    out = _run(2, R=1, steps=5, worker_timeout=1.5, silent=1)
    assert out[1] == {"silent": True}
    assert "no request from workers [1]" in out[0]["timeout"]


def test_sync_replicas_without_ps_rank_still_refuses_backup_workers():
    import dtg  # noqa: F401
    from dtg.optim import FusedSGD
    from dtg.parallel import FlatParams
    from dtg.train import SyncReplicasOptimizer
    flat = FlatParams(_model(), compute_dtype=torch.float32)
    sro = SyncReplicasOptimizer(FusedSGD(flat, lr=LR), replicas_to_aggregate=2, total_num_replicas=3)
    with pytest.raises(ValueError, match=r"replicas_to_aggregate=2 < total_num_replicas=3 \(backup workers\) needs "
                                         r"the PS-accumulator mode"):
        sro.minimize(lambda: None, global_step=None)
    assert sro.mode is None and sro.ps_worker is None


def test_resnet_sync_ps_example_session_driven():
    """examples/ResNet50/resnet50_sync_ps.py (tiny ResNet, gloo, CPU): 1 PS + 3 workers, R = 2; the workers run
    SyncReplicasOptimizer(ps_rank=0)'s train op under a MonitoredTrainingSession until StopAtStepHook(last_step=5),
    and the PS reports 5 global steps."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _cluster import free_ports
    base = free_ports(1)[0]
    script = os.path.join(ROOT, "examples", "ResNet50", "resnet50_sync_ps.py")
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1", DTG_BACKEND="gloo",
               DTG_SYNC_TIMEOUT="120", DTG_PS_WORKER_TIMEOUT="120")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    args = ["--tiny", "--workers", "3", "--replicas_to_aggregate", "2", "--steps", "5", "--batch", "2", "--image", "32",
            "--base_port", str(base)]
    procs = [subprocess.Popen([sys.executable, script, "--job_name", "ps", "--task_index", "0"] + args, env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)]
    procs += [subprocess.Popen([sys.executable, script, "--job_name", "worker", "--task_index", str(i)] + args,
                               env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for i in range(3)]
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=240)
            outs.append((p.returncode, o, e))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for rc, o, e in outs:
        assert rc == 0, o + e[-3000:]
    assert re.search(r"^\[ps\] 5 steps, contributed \{.*\}, dropped \{.*\}, lost \[\]$", outs[0][1], re.M), outs[0][1]
    for rc, o, e in outs[1:]:
        assert "global step 5" in o or "stopped=True" in o, o
