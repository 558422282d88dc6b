"""Evaluation off the GPU: the every-record-once sampler and loader, the PyTorch mirrors of the metric kernels against
per-row Python, the Evaluator's invariance to how the set is cut into batches and ranks, what it leaves untouched,
and the two ResNet-50 examples end to end."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import dtg  # noqa: F401
from dtg.data import DeviceLoader, EvalSampler, eval_params, synthetic_image_set, write_image_shards
from dtg.ops.augment import crop_resize_norm_ref, norm_constants
from dtg.ops.metrics import metric_accumulate, metric_accumulate_ref, xent_topk, xent_topk_ref
from dtg.train import EvalHook, Evaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SIZE, S, CLASSES = 50, 24, 16, 10


# ---- sampler ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch,world", [(50, 7, 1), (50, 3, 2), (50, 4, 3), (5, 4, 2), (48, 8, 2)])
def test_eval_sampler_every_record_once(n, batch, world):
    ranks = [EvalSampler(n, batch, world, r) for r in range(world)]
    steps = math.ceil(n / (batch * world))
    assert all(s.steps == steps and s.steps_per_epoch == steps for s in ranks)
    seen, padding = [], 0
    for step in range(steps):
        for s in ranks:
            idx, valid = s.at(step)
            assert idx.dtype == np.int64 and idx.shape == (batch,) and 0 <= valid <= batch
            assert (idx[valid:] == 0).all()  # padding repeats record 0
            seen.extend(idx[:valid].tolist())
            padding += batch - valid
    assert sorted(seen) == list(range(n)) and padding == steps * batch * world - n
    # in order: the ranks' valid slices of a step, rank-major, are consecutive records
    assert [i for st in range(steps) for s in ranks for i in s.at(st)[0][:s.at(st)[1]].tolist()] == list(range(n))
    for bad in (-1, steps):
        with pytest.raises(ValueError):
            ranks[0].at(bad)


# ---- the mirrors -----------------------------------------------------------------------------------------------
def _row_python(row, label):
    """(loss, rank) of one row by the definition, in Python floats"""
    V = len(row)
    if label < 0:
        return 0.0, -1
    if label >= V:
        return 0.0, -2
    xl = row[label]
    rank = sum(1 for j, v in enumerate(row) if v > xl or (v == xl and j < label))
    if any(math.isnan(v) for v in row):
        return float("nan"), V
    fin = [v for v in row if v != -math.inf]
    m = max(fin)
    lse = m + math.log(sum(math.exp(v - m) for v in fin))
    return lse - xl, rank


def _mirror_case():
    g = torch.Generator().manual_seed(0)
    B, V = 40, 13
    x = torch.randint(-4, 5, (B, V), generator=g).float()
    labels = torch.randint(0, V, (B,), generator=g)
    labels[0], labels[1], labels[2], labels[3] = -1, V, 0, V - 1
    labels[4], labels[5] = 3, 3
    x[4, 3] = float("nan")          # the label's logit is NaN
    x[5, 7] = float("nan")          # a NaN elsewhere in the row
    x[6:12, 1::3] = float("-inf")   # masked columns (the MLM vocabulary mask)
    labels[6:12] = torch.tensor([0, 2, 3, 5, 6, 12])
    x[12], labels[12] = 2.0, 5      # every column ties: the rank is the label itself
    return x, labels


def test_mirror_equals_per_row_python():
    x, labels = _mirror_case()
    B, V = x.shape
    loss, rank = xent_topk_ref(x, labels)
    assert loss.dtype == torch.float32 and rank.dtype == torch.int32
    want = [_row_python(x[r].tolist(), int(labels[r])) for r in range(B)]
    assert rank.tolist() == [w[1] for w in want]
    assert rank[0] == -1 and rank[1] == -2 and rank[4] == V and rank[5] == V and rank[12] == 5
    ties = sum(1 for r in range(B) if 0 <= int(labels[r]) < V and (x[r] == x[r, labels[r]]).sum() > 1)
    assert ties >= B // 2  # integer logits in [-4, 4] over 13 columns: the tie rule is exercised
    for r, (l, _) in enumerate(want):
        if math.isnan(l):
            assert math.isnan(loss[r].item()), r
        else:  # an fp32 logsumexp of 13 terms against Python doubles
            assert abs(loss[r].item() - l) <= 16 * 2.0 ** -24 * max(1.0, abs(l)), (r, loss[r].item(), l)
    assert loss[0] == 0 and loss[1] == 0
    # the public ops on CPU tensors are the mirrors; bf16 logits too (integers are exact in bf16)
    l2, r2 = xent_topk(x.bfloat16(), labels)
    assert torch.equal(r2, rank) and torch.equal(torch.isnan(l2), torch.isnan(loss))

    ks = (1, 5, 13)
    acc = torch.full((8,), 100.0, dtype=torch.float64)
    assert metric_accumulate(acc, loss[6:], rank[6:], ks, V) is acc  # the rows without NaN losses
    ranks6 = [w[1] for w in want[6:]]
    assert acc[0] == 100 + len(ranks6) and acc[2] == 100 and acc[3] == 100 and acc[7] == 100
    assert [acc[4 + i].item() - 100 for i in range(3)] == [sum(1 for q in ranks6 if q < k) for k in ks]
    assert abs(acc[1].item() - 100 - loss[6:].double().sum().item()) <= 1e-12
    acc2 = torch.zeros(8, dtype=torch.float64)
    metric_accumulate_ref(acc2, loss, rank, (1,), V)
    assert acc2[0] == B - 2 and acc2[2] == 1 and acc2[3] == 2 and math.isnan(acc2[1].item())
    for bad_ks in ((), (1, 2, 3, 4, 5), (0,)):
        with pytest.raises(ValueError):
            metric_accumulate(acc, loss, rank, bad_ks, V)
    with pytest.raises(ValueError):
        metric_accumulate(torch.zeros(8), loss, rank, (1,), V)  # acc must be fp64
    with pytest.raises(ValueError):
        xent_topk(x, labels.int())


# ---- the Evaluator ------------------------------------------------------------------------------------------------
class StubModel(torch.nn.Module):
    """logits = a fixed fp32 linear map of the mean-pooled image, written so that a record's logits cannot depend on
    the batch it is in: the pooling sums bf16-valued pixels in fp64, which is exact in any order, and the map is three
    element-wise multiply-adds."""

    def __init__(self, classes=CLASSES):
        super().__init__()
        g = torch.Generator().manual_seed(12)  # 9 of the 50 records land in the top 1, 31 in the top 5
        self.register_buffer("w", torch.randn(3, classes, generator=g) * 40)
        # centred on the set's mean colour, so that the winning class changes from record to record
        self.register_buffer("b", -(torch.tensor([0.08, 0.17, 0.35]) @ self.w) + torch.randn(classes, generator=g))

    def forward(self, x):
        p = x.double().sum((2, 3)).float() / float(x.shape[2] * x.shape[3])
        return (p[:, 0:1] * self.w[0] + p[:, 1:2] * self.w[1]) + (p[:, 2:3] * self.w[2] + self.b)


@pytest.fixture(scope="module")
def eval_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("val")
    images, labels = synthetic_image_set(N, size=SIZE, classes=CLASSES, seed=8)
    write_image_shards(str(d), images, labels, per_shard=20)
    # the per-record reference: one record at a time through the augmentation mirror, the stub and the row definition
    model = StubModel()
    scale, shift = norm_constants()
    p = torch.from_numpy(eval_params(1, SIZE, SIZE))
    losses, ranks = [], []
    for i in range(N):
        x = crop_resize_norm_ref(torch.from_numpy(images[i:i + 1]), p, S, scale, shift).float()
        l, r = xent_topk_ref(model(x), torch.tensor([int(labels[i])]))
        losses.append(l[0].double().item())
        ranks.append(int(r[0]))
    ref = {"n": N, "top1": sum(r < 1 for r in ranks), "top5": sum(r < 5 for r in ranks),
           "loss": math.fsum(losses) / N}
    assert 0 < ref["top1"] < ref["top5"] < N  # the counts can go wrong in either direction
    return str(d), ref


def _evaluate(d, batch, world=1, rank=0):
    with DeviceLoader(d, batch, S, "cpu", world=world, rank=rank, train=False, drop_last=False,
                      dtype=torch.float32) as loader:
        assert loader.steps_per_epoch == math.ceil(N / (batch * world))
        return Evaluator(StubModel(), loader, ks=(1, 5)).run()


def _check_result(res, ref, what):
    err = abs(res["loss"] - ref["loss"]) / abs(ref["loss"])
    print("[eval] %s: n=%d top1=%d top5=%d loss=%.12f rel err=%.3e bound=%.3e" % (
        what, res["n"], res["top1_count"], res["top5_count"], res["loss"], err, (N + 8) * 2.0 ** -53))
    assert res["n"] == ref["n"] and res["bad_labels"] == 0 and res["nonfinite"] == 0
    assert res["top1_count"] == ref["top1"] and res["top5_count"] == ref["top5"]
    assert res["top1"] == ref["top1"] / N and res["top5"] == ref["top5"] / N
    assert err <= (N + 8) * 2.0 ** -53  # fp64 sums of the same fp32 terms
    assert res["seconds"] > 0 and res["images_per_sec"] > 0


@pytest.mark.parametrize("batch", [7, 50])
def test_evaluator_equals_per_record_reference(eval_set, batch):
    d, ref = eval_set
    _check_result(_evaluate(d, batch), ref, "1 rank x %d" % batch)


def _gloo_rank(rank, world, port, d, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        import dtg  # noqa: F401
        from dtg.parallel import comm
        comm.init("gloo")
        res = _evaluate(d, 3, world, rank)
        comm.shutdown()
        q.put((rank, res))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, traceback.format_exc()))
        raise


def test_evaluator_two_gloo_ranks(eval_set):
    d, ref = eval_set
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _cluster import free_ports
    port = free_ports(1)[0]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_rank, args=(r, 2, port, d, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    res = dict(q.get(timeout=5) for _ in range(2))
    assert all(isinstance(v, dict) for v in res.values()), res
    for r in (0, 1):
        _check_result(res[r], ref, "2 gloo ranks x 3, rank %d" % r)
    assert res[0]["loss_sum"] == res[1]["loss_sum"]  # one all-reduce: every rank holds the same sums


def test_loader_pads_with_ignored_labels(eval_set):
    d, _ = eval_set
    with DeviceLoader(d, 8, S, "cpu", train=False, drop_last=False, dtype=torch.float32) as loader:
        assert loader.steps_per_epoch == 7
        seen = []
        for step in range(7):
            x, y, i = loader.next()
            valid = 8 if step < 6 else 2
            assert (y[valid:] == -1).all() and (y[:valid] >= 0).all() and (i[valid:] == 0).all()
            seen.extend(i[:valid].tolist())
        assert seen == list(range(N))
        with pytest.raises(StopIteration):
            loader.next()
        loader.seek(0)
        assert loader.next()[2].tolist() == list(range(8))
    with pytest.raises(ValueError):
        DeviceLoader(d, 8, S, "cpu", train=True, drop_last=False)
    with DeviceLoader(d, 8, S, "cpu", train=False) as dropping:  # the default is unchanged
        assert dropping.steps_per_epoch == 6 and dropping.drop_last
        with pytest.raises(ValueError):
            Evaluator(StubModel(), dropping)


@pytest.mark.parametrize("training", [True, False])
def test_evaluator_leaves_the_model_as_it_was(eval_set, training):
    from dtg.models import resnet
    d, _ = eval_set
    torch.manual_seed(3)
    model = resnet.resnet18_like_tiny(CLASSES)
    with torch.no_grad():
        for m in model.modules():  # running statistics away from (0, 1)
            if hasattr(m, "running_mean"):
                m.running_mean.normal_(0, 0.5)
                m.running_var.uniform_(0.5, 2.0)
    model.train(training)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with DeviceLoader(d, 16, 32, "cpu", train=False, drop_last=False, dtype=torch.float32) as loader:
        res = Evaluator(model, loader).run()
    assert res["n"] == N and math.isfinite(res["loss"]) and model.training is training
    assert all(m.training is training for m in model.modules())
    after = model.state_dict()
    assert before.keys() == after.keys() and len(before) > 20
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert not any(p.grad is not None for p in model.parameters())


def test_evaluator_refuses_out_of_range_labels(tmp_path):
    images, labels = synthetic_image_set(20, size=SIZE, classes=CLASSES, seed=9)
    labels = labels.copy()
    labels[13] = CLASSES
    write_image_shards(str(tmp_path), images, labels, per_shard=20)
    with DeviceLoader(str(tmp_path), 8, S, "cpu", train=False, drop_last=False, dtype=torch.float32) as loader:
        with pytest.raises(ValueError, match="1 records"):
            Evaluator(StubModel(), loader).run()


def test_eval_hook_schedule():
    class Ev:
        ks, calls, closed = (1,), 0, False

        def run(self):
            self.calls += 1
            return {"n": 1, "loss": 0.5, "top1": 1.0}

        def close(self):
            self.closed = True

    class Values:
        def __init__(self, v):
            self.results = v

    class Sess:
        def _read(self, gs):
            return 7

    ev = Ev()
    hook = EvalHook(ev, 3, "gs", log=False)
    for step in (1, 2, 3, 3, 4, 5, 6, 7):  # a run that does not advance the step evaluates nothing again
        hook.after_run(None, Values(step))
    hook.end(Sess())
    assert [s for s, _ in hook.results] == [3, 6, 7] and ev.calls == 3 and ev.closed
    ev2 = Ev()
    hook2 = EvalHook(ev2, 7, "gs", log=False)
    hook2.after_run(None, Values(7))
    hook2.end(Sess())
    assert [s for s, _ in hook2.results] == [7]  # the last step was just evaluated


# ---- the examples, end to end -------------------------------------------------------------------------------------
def _clean_env():
    e = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DTG_FAULT"):
        e.pop(k, None)
    return e


def test_examples_train_with_eval_then_eval_script(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _cluster import free_ports
    train_dir, val_dir, ck = str(tmp_path / "train"), str(tmp_path / "val"), str(tmp_path / "ck")
    images, labels = synthetic_image_set(40, size=36, classes=10, seed=1)
    write_image_shards(train_dir, images, labels, per_shard=16)
    images, labels = synthetic_image_set(30, size=36, classes=10, seed=2)  # 30 records at 2 x 4: the last step pads
    write_image_shards(val_dir, images, labels, per_shard=16)
    ex = os.path.join(ROOT, "examples", "ResNet50")

    def launch(nproc, script, *args):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(free_ports(1)[0]), os.path.join(ex, script), *args]
        return subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=_clean_env())

    r = launch(2, "resnet50_train.py", "--tiny", "--batch", "4", "--steps", "5", "--save_every", "100", "--log_every",
               "1", "--ckpt_dir", ck, "--data_dir", train_dir, "--eval_dir", val_dir, "--eval_every", "2")
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("eval step ")]
    print("\n".join(lines))
    assert [int(re.match(r"eval step (\d+):", l).group(1)) for l in lines] == [2, 4, 5], r.stdout
    assert all(re.fullmatch(r"eval step \d+: n=30 loss=\d+\.\d{6} top1=\d\.\d{6} top5=\d\.\d{6}", l) for l in lines)
    assert "done at global step 5" in r.stdout

    e = launch(2, "resnet50_eval.py", "--tiny", "--batch", "4", "--ckpt_dir", ck, "--data_dir", val_dir)
    assert e.returncode == 0, e.stdout + e.stderr[-3000:]
    got = [l for l in e.stdout.splitlines() if l.startswith("eval step ")]
    print("\n".join(got))
    assert got == lines[-1:], (got, lines)  # the same counts, the loss to the printed digits

    none = launch(1, "resnet50_eval.py", "--tiny", "--ckpt_dir", str(tmp_path / "empty"), "--data_dir", val_dir)
    assert none.returncode == 1 and "no checkpoint" in none.stderr
