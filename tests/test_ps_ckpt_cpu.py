"""Checkpoint and restart of the GPU parameter servers (parallel/ps_ckpt.py) with gloo ranks on the CPU: fp32
compute, the fixed per-worker batches of test_sync_ps_cpu.py, every process under a timeout.  When the PS has
exited the harness ends the surviving workers, as a launcher would.

* sync PS, R = M = 2: the PS dies at global step 4 (``DTG_FAULT=kill_ps_at_step:4``, exit code 23); the whole job
  is restarted and runs to step 8; masters and momentum are bit-equal to an uninterrupted 8-step run (a two-term
  fp32 sum is commutative, so arrival order cannot change it; this holds whichever checkpoint was the last
  complete one);
* async PS, 1 worker: the same with updates instead of steps;
* interoperation with save_flat / restore_flat, the Adagrad slot padding, and the in-place bundle writer.
"""
import os
import sys

import numpy as np
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 0.1
MU = 0.9


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


def _rank(rank, world, port, q, kind, steps, ckpt_dir, fault):
    """Rank 0: the PS (sync or async) with a PSCheckpointer on ``ckpt_dir`` (every_n = 1).  Workers push until the
    global step (sync) or ``ps_updates_at_begin + pushes`` (async) reaches ``steps``."""
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank), DTG_SYNC_TIMEOUT="60", DTG_PS_WORKER_TIMEOUT="60")
        os.environ.pop("DTG_FAULT", None)
        if fault and rank == 0:
            os.environ["DTG_FAULT"] = fault
        import time
        import dtg  # noqa: F401
        from dtg import ops
        from dtg.optim import FusedSGD
        from dtg.parallel import FlatParams, comm
        from dtg.parallel.async_ps import AsyncPSServer, AsyncPSWorker
        from dtg.parallel.ps_ckpt import PSCheckpointer
        from dtg.parallel.sync_ps import SyncPSServer, SyncPSWorker
        comm.init("gloo")
        model = _model()
        flat = FlatParams(model, compute_dtype=torch.float32)
        if rank == 0:
            opt = FusedSGD(flat, lr=LR, momentum=MU)
            ck = PSCheckpointer(flat, opt, ckpt_dir, every_n=1) if ckpt_dir else None
            if kind == "sync":
                ps = SyncPSServer(flat, opt, workers=range(1, world), replicas_to_aggregate=world - 1, checkpointer=ck)
            else:
                ps = AsyncPSServer(flat, opt, workers=range(1, world), checkpointer=ck)
            w0 = [g.master.clone().numpy() for g in flat]
            n = ps.serve()
            q.put((rank, "ok", {"n": n, "restored": ps.restored_step, "w0": w0,
                                "step": ps.global_step if kind == "sync" else ps.updates,
                                "version": getattr(ps, "version", None), "step_count": opt.step_count,
                                "saved": list(ck.saved) if ck else None,
                                "w": [g.master.clone().numpy() for g in flat],
                                "m": [g.state["momentum"].clone().numpy() for g in flat]}))
            ps.close()
        else:
            x, y = _data(rank)
            if kind == "sync":
                w = SyncPSWorker(flat, ps_rank=0)
                w.begin()
                begin = w.global_step
                while w.global_step < steps and not w.stopped:
                    ops.softmax_cross_entropy(model(x), y).backward()
                    time.sleep(0.05)
                    w.step_done()
            else:
                w = AsyncPSWorker(flat, ps_rank=0, window=1, overlap_pull=False)
                w.begin()
                begin = w.ps_updates_at_begin
                while w.ps_updates_at_begin + w.pushes < steps:
                    ops.softmax_cross_entropy(model(x), y).backward()
                    w.step_done()
            w.finish()
            q.put((rank, "ok", {"begin": begin, "pushes": w.pushes}))
        comm.shutdown()
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc(), None))
        raise


def _job(kind, world, steps, ckpt_dir, fault=None):
    """Run one job.  Returns (PS exit code, {rank: payload}).  With ``fault`` the PS is expected to die: the
    workers are ended as soon as it has exited."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _cluster import free_ports
    port = free_ports(1)[0]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q, kind, steps, ckpt_dir, fault)) for r in range(world)]
    for p in procs:
        p.start()
    out = {}
    try:
        if fault:
            procs[0].join(timeout=120)
            assert not procs[0].is_alive(), "the PS outlived its fault"
        else:
            for _ in range(world):
                r, status, payload = q.get(timeout=120)
                assert status == "ok", status
                out[r] = payload
            for p in procs:
                p.join(timeout=30)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
            p.join(timeout=30)
    return procs[0].exitcode, out


def _latest_step(d):
    from dtg.train.saver import latest_checkpoint, read_tensors
    prefix = latest_checkpoint(str(d))
    assert prefix is not None, os.listdir(str(d))
    vals = read_tensors(prefix, verify=True)  # CRC32C of every tensor and every index block
    return prefix, vals, int(vals["global_step"])


def _save_flat_keys(tmp):
    from dtg.optim import FusedSGD
    from dtg.parallel import FlatParams
    from dtg.train.saver import read_tensors, save_flat
    flat = FlatParams(_model(), compute_dtype=torch.float32)
    opt = FusedSGD(flat, lr=LR, momentum=MU)
    for g in flat:
        g.state_buffer("momentum")
    return set(read_tensors(save_flat(flat, str(tmp / "ref.ckpt"), global_step=1, optimizer=opt)))


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def test_sync_ps_killed_and_restarted_equals_uninterrupted(tmp_path):
    d, dref = tmp_path / "job", tmp_path / "ref"
    rc, _ = _job("sync", 3, 8, str(d), fault="kill_ps_at_step:4")
    assert rc == 23
    prefix, vals, k = _latest_step(d)
    assert 1 <= k <= 4
    rc, out = _job("sync", 3, 8, str(d))
    assert rc == 0
    ps = out[0]
    assert ps["restored"] == k and ps["step"] == 8 and ps["n"] == 8 - k and ps["step_count"] == 8
    assert out[1]["begin"] == out[2]["begin"] == k  # the restarted PS's first reply carries the restored step
    rc, ref = _job("sync", 3, 8, str(dref))
    assert rc == 0 and ref[0]["restored"] is None and ref[0]["n"] == 8
    assert _same(ps["w"], ref[0]["w"]) and _same(ps["m"], ref[0]["m"])
    # the final checkpoints: step 8, the keys of save_flat for this model and optimizer
    for dd in (d, dref):
        _, v, s = _latest_step(dd)
        assert s == 8 and set(v) == _save_flat_keys(tmp_path)

    # a PS checkpoint loads with restore_flat
    import dtg  # noqa: F401
    from dtg.optim import FusedSGD
    from dtg.parallel import FlatParams
    from dtg.train.saver import restore_flat
    flat = FlatParams(_model(), compute_dtype=torch.float32)
    for g in flat:
        g.master.zero_()
    opt = FusedSGD(flat, lr=LR, momentum=MU)
    assert restore_flat(flat, _latest_step(d)[0], optimizer=opt) == 8
    assert opt.step_count == 8
    assert _same([g.master.numpy() for g in flat], ps["w"])
    assert _same([g.state["momentum"].numpy() for g in flat], ps["m"])


def test_async_ps_killed_and_restarted_equals_uninterrupted(tmp_path):
    d, dref = tmp_path / "job", tmp_path / "ref"
    rc, _ = _job("async", 2, 8, str(d), fault="kill_ps_at_step:4")
    assert rc == 23
    _, vals, k = _latest_step(d)
    assert 1 <= k <= 4 and int(vals["dtg/ps/version"]) == k
    rc, out = _job("async", 2, 8, str(d))
    assert rc == 0
    ps = out[0]
    assert ps["restored"] == k and ps["step"] == 8 and ps["version"] == 8 and ps["n"] == 8
    assert out[1]["begin"] == k and out[1]["pushes"] == 8 - k
    rc, ref = _job("async", 2, 8, str(dref))
    assert rc == 0 and ref[1]["begin"] == 0 and ref[1]["pushes"] == 8
    assert _same(ps["w"], ref[0]["w"]) and _same(ps["m"], ref[0]["m"])
    _, v, s = _latest_step(d)
    assert s == 8 and int(v["dtg/ps/version"]) == 8
    assert set(v) == _save_flat_keys(tmp_path) | {"dtg/ps/version"}


def test_save_flat_checkpoint_starts_a_sync_ps(tmp_path):
    import dtg  # noqa: F401
    from dtg.optim import FusedSGD
    from dtg.parallel import FlatParams
    from dtg.train.saver import save_flat
    flat = FlatParams(_model(), compute_dtype=torch.float32)
    opt = FusedSGD(flat, lr=LR, momentum=MU)
    with torch.no_grad():
        for g in flat:
            g.master.mul_(0.5)
            g.state_buffer("momentum").copy_(0.01 * g.master)
    opt.step_count = 3
    d = tmp_path / "seed"
    os.makedirs(str(d))
    save_flat(flat, str(d / "model.ckpt"), global_step=3, optimizer=opt)
    rc, out = _job("sync", 3, 5, str(d))
    assert rc == 0
    ps = out[0]
    assert ps["restored"] == 3 and ps["n"] == 2 and ps["step"] == 5 and ps["step_count"] == 5
    assert out[1]["begin"] == out[2]["begin"] == 3
    assert _same(ps["w0"], [g.master.numpy() for g in flat])
    assert _latest_step(d)[2] == 5


def test_adagrad_slot_padding_survives_restore(tmp_path):
    import dtg  # noqa: F401
    from dtg.optim import FusedAdagrad
    from dtg.parallel import FlatParams
    from dtg.parallel.ps_ckpt import PSCheckpointer
    flat = FlatParams(_model(), compute_dtype=torch.float32)
    opt = FusedAdagrad(flat, lr=LR)
    x, y = _data(1)
    from dtg import ops
    ops.softmax_cross_entropy(flat.module(x), y).backward()
    opt.step()
    ck = PSCheckpointer(flat, opt, str(tmp_path), every_n=1)
    assert ck.maybe_save(1) and not ck.maybe_save(1)
    ck.flush()
    assert ck.saved == [1] and ck.skipped == 0

    flat2 = FlatParams(_model(), compute_dtype=torch.float32)
    for g in flat2:
        g.master.zero_()
    opt2 = FusedAdagrad(flat2, lr=LR)
    assert PSCheckpointer(flat2, opt2, str(tmp_path)).restore_latest() == 1
    assert opt2.step_count == 1 and float(opt2.hyper[1]) == 1.0
    some_padding = False
    for g, g2 in zip(flat, flat2):
        assert torch.equal(g.master, g2.master)
        pad = torch.ones(g.numel, dtype=torch.bool)
        for _, p, o, numel in g.param_slices():
            pad[o:o + numel] = False
            assert torch.equal(g.state["acc"][o:o + numel], g2.state["acc"][o:o + numel])
        some_padding |= bool(pad.any())
        # the checkpoint does not hold the padding: it keeps the initial accumulator value of optimizer.new_slot
        assert (g2.state["acc"][pad] == opt2.init_acc).all()
    assert some_padding


def test_legacy_marked_checkpoint_is_refused(tmp_path):
    import pytest
    import dtg  # noqa: F401
    from dtg.optim import FusedSGD
    from dtg.parallel import FlatParams
    from dtg.parallel.ps_ckpt import PSCheckpointer
    from dtg.train.saver import SLOT_LAYOUT_KEY, flat_arrays, update_checkpoint_state, write_tensors
    flat = FlatParams(_model(), compute_dtype=torch.float32)
    opt = FusedSGD(flat, lr=LR, momentum=MU)
    arrays = [(n, np.array(0, dtype=np.int64) if n == SLOT_LAYOUT_KEY else a) for n, a in flat_arrays(flat, opt)]
    prefix = str(tmp_path / "model.ckpt-1")
    write_tensors(prefix, arrays)
    update_checkpoint_state(str(tmp_path), prefix, [prefix])
    with pytest.raises(ValueError, match="slot layout"):
        PSCheckpointer(flat, opt, str(tmp_path)).restore_latest()


def test_inplace_bundle_writer_is_byte_identical(tmp_path):
    import dtg  # noqa: F401
    from dtg.train.saver import read_tensors, write_tensors, write_tensors_inplace
    rng = np.random.default_rng(0)
    big = rng.standard_normal(70001).astype(np.float32)
    arrays = [("z/w", rng.standard_normal((7, 13)).astype(np.float32)),
              ("a", big[3:60000]),                                   # a view at an odd offset
              ("global_step", np.array(12, dtype=np.int64)),         # 0-d
              ("m/bits", rng.integers(0, 1 << 16, (5, 3)).astype(np.uint16)),
              ("d", rng.standard_normal(9)), ("i", np.arange(6, dtype=np.int32).reshape(2, 3)),
              ("empty", np.zeros((0, 4), dtype=np.float32))]
    arrays += [("k%03d" % i, rng.standard_normal(i + 1).astype(np.float32)) for i in range(300)]
    a, b = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    write_tensors(a, arrays)
    write_tensors_inplace(b, arrays)
    for suf in (".index", ".data-00000-of-00001"):
        with open(a + suf, "rb") as fa, open(b + suf, "rb") as fb:
            assert fa.read() == fb.read(), suf
    got = read_tensors(b)
    for n, v in arrays:
        assert got[n].dtype == v.dtype and got[n].shape == v.shape and np.array_equal(got[n], v), n
