"""PSCheckpointer (parallel/ps_ckpt.py) on the device: round trip against the per-parameter oracle, the stream
ordering of a snapshot, and a one-card checkpoint / restart rehearsal of the sync PS (clean exits only)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _tiny(dev, zero=False):
    import dtg  # noqa: F401
    from dtg.models import resnet
    from dtg.parallel import FlatParams
    torch.manual_seed(1234)
    model = resnet.resnet18_like_tiny(10).to(dev).to(memory_format=torch.channels_last)
    if zero:
        with torch.no_grad():
            for p in model.parameters():
                p.zero_()
            for b in model.buffers():
                b.zero_()
    return model, FlatParams(model)


def _make_opt(kind, flat):
    from dtg.optim import FusedAdam, FusedSGD
    return FusedSGD(flat, lr=0.1, momentum=0.9, weight_decay=5e-5) if kind == "momentum" else FusedAdam(flat, lr=1e-3)


def _steps(model, flat, opt, n, dev):
    from dtg import ops
    from dtg.models import resnet
    x, y = resnet.synthetic_batch(8, dev, torch.bfloat16, 32, 10)
    for _ in range(n):
        ops.softmax_cross_entropy(model(x), y).backward()
        opt.step()


def _oracle(flat, opt):
    from dtg.train.saver import flat_arrays_per_param
    return [(n, np.array(a, order="C")) for n, a in flat_arrays_per_param(flat, opt)]


@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_checkpoint_round_trip(tmp_path, kind):
    from dtg.parallel.ps_ckpt import PSCheckpointer
    from dtg.train.saver import flat_arrays, latest_checkpoint, read_tensors
    dev = torch.device("cuda", 0)
    model, flat = _tiny(dev)
    opt = _make_opt(kind, flat)
    _steps(model, flat, opt, 2, dev)
    want = _oracle(flat, opt)
    # the saver's packed route gives the oracle's arrays, keys and order
    got = flat_arrays(flat, opt)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), n

    ck = PSCheckpointer(flat, opt, str(tmp_path), every_n=2)
    assert not ck.maybe_save(1) and ck.maybe_save(2, {"dtg/ps/version": 2})
    ck.flush()
    assert ck.saved == [2] and ck.skipped == 0
    prefix = latest_checkpoint(str(tmp_path))
    assert prefix.endswith("model.ckpt-2")
    vals = read_tensors(prefix)
    assert list(vals) == sorted([n for n, _ in want] + ["global_step", "dtg/ps/version"])
    assert int(vals["global_step"]) == 2 and int(vals["dtg/ps/version"]) == 2
    for n, b in want:
        a = vals[n]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), n

    model2, flat2 = _tiny(dev, zero=True)
    opt2 = _make_opt(kind, flat2)
    assert PSCheckpointer(flat2, opt2, str(tmp_path)).restore_latest() == 2
    assert opt2.step_count == opt.step_count == 2 and float(opt2.hyper[1]) == 2.0
    for g, g2 in zip(flat, flat2):
        assert torch.equal(g.master, g2.master), g.name
        if g.mirror is not None:
            assert torch.equal(g.mirror, g2.mirror), g.name
        assert set(g.state) == set(g2.state) and g.state
        for k in g.state:
            assert torch.equal(g.state[k], g2.state[k]), (g.name, k)  # slot padding is zero on both sides
    for (n, b), (_, b2) in zip(model.named_buffers(), model2.named_buffers()):
        assert torch.equal(b, b2), n
    for (n, p), (_, p2) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p, p2), n


def test_snapshot_is_the_state_before_the_next_apply(tmp_path):
    """maybe_save, then at once an optimizer step on the same stream, then flush: the file holds the pre-step
    state (it would not if the host copy read the live buffers)."""
    from dtg.parallel.ps_ckpt import PSCheckpointer
    from dtg.train.saver import latest_checkpoint, read_tensors
    dev = torch.device("cuda", 0)
    model, flat = _tiny(dev)
    opt = _make_opt("momentum", flat)
    _steps(model, flat, opt, 2, dev)
    from dtg import ops
    from dtg.models import resnet
    x, y = resnet.synthetic_batch(8, dev, torch.bfloat16, 32, 10)
    ops.softmax_cross_entropy(model(x), y).backward()  # the next step's gradient, ready before the save
    torch.cuda.synchronize()
    want = _oracle(flat, opt)
    ck = PSCheckpointer(flat, opt, str(tmp_path), every_n=1)
    assert ck.maybe_save(2)
    opt.step()
    ck.flush()
    after = dict(_oracle(flat, opt))
    vals = read_tensors(latest_checkpoint(str(tmp_path)))
    changed = 0
    for n, b in want:
        assert np.array_equal(vals[n], b), n
        changed += int(not np.array_equal(after[n], b))
    assert changed > 10 and int(vals["optimizer/step"]) == 2 and ck.saved == [2]


def _rehearsal(d, steps):
    cmd = ["bash", os.path.join(ROOT, "tools", "sync_ps_rehearsal.sh"), "3", "--tiny", "--replicas_to_aggregate", "2",
           "--steps", str(steps), "--batch", "8", "--image", "32", "--ckpt_dir", d, "--save_every", "2"]
    env = dict(os.environ, DTG_SYNC_TIMEOUT="60", DTG_PS_WORKER_TIMEOUT="60")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DTG_FAULT"):
        env.pop(k, None)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_sync_ps_rehearsal_restarts_from_its_checkpoint(tmp_path):
    from dtg.train.saver import latest_checkpoint, read_tensors
    d = str(tmp_path / "ckpt")
    out = _rehearsal(d, 6)
    assert re.search(r"^\[ps\] 6 steps,", out, re.M) and "restored" not in out, out
    assert latest_checkpoint(d).endswith("model.ckpt-6")
    out = _rehearsal(d, 10)
    assert re.search(r"^\[ps\] restored .*model\.ckpt-6 at step 6$", out, re.M), out
    assert re.search(r"^\[ps\] 4 steps,", out, re.M), out
    prefix = latest_checkpoint(d)
    assert prefix.endswith("model.ckpt-10")
    vals = read_tensors(prefix)
    assert int(vals["global_step"]) == 10 and int(vals["optimizer/step"]) == 10
    dev = torch.device("cuda", 0)
    model, flat = _tiny(dev)
    opt = _make_opt("momentum", flat)
    for g in flat:
        g.state_buffer("momentum")
    assert set(vals) == {n for n, _ in _oracle(flat, opt)} | {"global_step"}
