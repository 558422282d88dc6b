"""Gradient accumulation over micro-batches (parallel/accum.py, train/eager.py ``accum_steps``) on the CPU, fp32 compute:

* the mirrors ``grad_fold_ref`` / ``grad_unfold_ref`` against per-element Python;
* ``accum_steps=1`` is the plain path, bit for bit, and allocates nothing;
* one rank x ``accum_steps=2`` x batch 2B == two gloo ranks x batch B, bit for bit (masters and slots);
* ``accum_steps=3`` and two gloo ranks x ``accum_steps=2`` against explicit loops that sum the micro-gradients in fp32;
* the loader's rows: ``DeviceLoader(batch=A*B)`` chunked by A == the ranks of a ``world * A`` job;
* BERT's masked-LM normalisation over the whole step; the examples; the refusals.
"""
import dataclasses
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import dtg
from dtg import graph as G
from dtg import ops
from dtg.models import bert, resnet
from dtg.ops import optim_kernels as K
from dtg.optim import FusedAdam, FusedLAMB, FusedSGD
from dtg.parallel import FlatParams, GradAccumulator, GraphedStep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4          # micro-batch
SEQ, P = 16, 4


@pytest.fixture(autouse=True)
def _one_thread():
    """one CPU thread everywhere (the spawned ranks too): a reduction's order must not depend on the process"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ---- 1. the mirrors against per-element Python ---------------------------------------------------------------------
def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _bf16_rne_bits(x):
    """fp32 value -> bf16 bits, round to nearest even (NaN -> None)"""
    if x != x:
        return None
    u = _f32_bits(x)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


BF16_MAX = float(torch.finfo(torch.bfloat16).max)
VALUES = [1.5, -2.25, -0.0, 0.0, BF16_MAX, -BF16_MAX, float("inf"), float("-inf"), float("nan"), 1e-3, 3.0e-39,
          257.0, 0.1]
ACCS = [0.75, 2.25, 0.0, -0.0, BF16_MAX, 1.0, 1.0, float("inf"), 2.0, 1.0 + 2.0 ** -9, 1.0, 1.0 + 2.0 ** -8, float("nan")]


def _add32(a, b):
    return float(np.float32(a) + np.float32(b))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_mirrors_equal_per_element_python(dt):
    g0 = torch.tensor(VALUES, dtype=torch.float32).to(dt)
    gl = [float(v) for v in g0.float().tolist()]  # the values g really holds
    for first in (True, False):
        acc, g = torch.tensor(ACCS, dtype=torch.float32), g0.clone()
        K.grad_fold_ref(acc, g, first)
        with np.errstate(all="ignore"):
            want = [gv if first else _add32(a, gv) for a, gv in zip(ACCS, gl)]
        for got, w in zip(acc.tolist(), want):
            assert (got != got and w != w) or _f32_bits(got) == _f32_bits(w), (first, got, w)
        assert g.dtype == dt and g.view(torch.int16 if dt == torch.bfloat16 else torch.int32).eq(0).all()
    a = torch.ones(1)
    K.grad_fold_ref(a, torch.tensor([-0.0]).to(dt), True)
    assert _f32_bits(a.item()) == 0x80000000  # a first fold keeps the sign of a zero
    # unfold over [2, 11): outside the range g keeps its bits, acc keeps all of them
    acc, g = torch.tensor(ACCS, dtype=torch.float32), g0.clone()
    K.grad_unfold_ref(g, acc, 2, 11)
    iv = torch.int16 if dt == torch.bfloat16 else torch.int32
    assert torch.equal(g[:2].view(iv), g0[:2].view(iv)) and torch.equal(g[11:].view(iv), g0[11:].view(iv))
    nan = torch.isnan(torch.tensor(ACCS))
    assert torch.equal(torch.isnan(acc), nan) and torch.equal(acc[~nan], torch.tensor(ACCS)[~nan])
    for i in range(2, 11):
        with np.errstate(all="ignore"):
            s = _add32(ACCS[i], gl[i])
        got = g[i:i + 1]
        if s != s:
            assert torch.isnan(got).all(), i
        elif dt == torch.bfloat16:
            assert int(got.view(torch.int16).item()) & 0xFFFF == _bf16_rne_bits(s), (i, s)
        else:
            assert _f32_bits(got.item()) == _f32_bits(s), (i, s)
    # the per-element rounding itself: 1 + 2^-8 and 1 + 3 * 2^-8 lie halfway between two bf16 values (ties to even)
    assert _bf16_rne_bits(1.0 + 2.0 ** -8) == 0x3F80 and _bf16_rne_bits(1.0 + 3 * 2.0 ** -8) == 0x3F82


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_first_fold_never_reads_the_accumulator(dt):
    acc = torch.full((37,), float("nan"))
    g = torch.arange(37, dtype=torch.float32).to(dt)
    K.grad_fold(acc, g, True)
    assert not torch.isnan(acc).any() and torch.equal(acc, torch.arange(37, dtype=torch.float32))
    assert not g.any()
    K.grad_unfold(g, acc)  # the whole buffer by default
    assert torch.equal(g.float(), torch.arange(37, dtype=torch.float32))
    with pytest.raises(RuntimeError):
        K.grad_unfold(g, acc, 3, 38)
    with pytest.raises(RuntimeError):
        K.grad_fold(acc.bfloat16(), g, True)


# ---- models, optimizers, records ------------------------------------------------------------------------------------
def _bert_cfg():
    return dataclasses.replace(bert.BertConfig.tiny(), dropout=0.0, attn_dropout=0.0)


def _make(kind, seed=11):
    torch.manual_seed(seed)
    if kind == "resnet":
        m = resnet.resnet18_like_tiny(10).to(memory_format=torch.channels_last)
    else:
        m = bert.BertForPreTraining(_bert_cfg())
    m.train()
    return m, FlatParams(m, compute_dtype=torch.float32)


def _opt(name, flat):
    if name == "momentum":
        return FusedSGD(flat, lr=0.05, momentum=0.9, weight_decay=1e-4)
    if name == "adam":
        return FusedAdam(flat, lr=1e-3)
    return FusedLAMB(flat, lr=1e-3, clip_norm=1.0)


def _loss_fn(kind, m):
    if kind == "resnet":
        return lambda x, y: ops.softmax_cross_entropy(m(x), y)
    return lambda *b: m(*b)  # the synthetic batch: num_valid=None, every slot counts


def _records(kind, step, n):
    """the step's global batch of n records: every job reads its rows of this one"""
    if kind == "resnet":
        return resnet.synthetic_batch(n, "cpu", torch.float32, 32, 10, seed=100 + step)
    return bert.synthetic_batch(n, SEQ, _bert_cfg(), "cpu", max_predictions=P, seed=100 + step)


def _rows(batch, lo, hi):
    return [t[lo:hi] for t in batch]


def _snapshot(flat, buffers=False):
    s = {"master": [g.master.clone() for g in flat],
         "slots": [{k: v.clone() for k, v in sorted(g.state.items())} for g in flat]}
    if buffers:
        s["buffers"] = flat.buffers.flat.clone() if flat.buffers is not None else torch.zeros(0)
    return s


def _assert_same(a, b, what):
    for i, (x, y) in enumerate(zip(a["master"], b["master"])):
        assert torch.equal(x, y), "%s: master of group %d differs (max |d| %g)" % (what, i, (x - y).abs().max())
    for i, (x, y) in enumerate(zip(a["slots"], b["slots"])):
        assert list(x) == list(y) and len(x) > 0, (what, list(x), list(y))
        for k in x:
            assert torch.equal(x[k], y[k]), "%s: slot %s of group %d differs" % (what, k, i)
    if "buffers" in a:
        assert torch.equal(a["buffers"], b["buffers"]), what + ": module buffers differ"


def _train(kind, optname, accum_steps, rows, steps, total, rank=0, world=1, sync=False, buffers=False):
    """``steps`` global steps through a session; this job feeds rows [rank*rows, (rank+1)*rows) of each step's
    ``total`` records.  accum_steps None: minimize() without the keyword."""
    G.reset_default_graph()
    m, flat = _make(kind)
    opt = _opt(optname, flat)
    n_in = 2 if kind == "resnet" else 6
    phs = [dtg.placeholder() for _ in range(n_in)]
    gs = dtg.train.get_or_create_global_step()
    kw = {} if accum_steps is None else {"accum_steps": accum_steps}
    hooks = []
    if sync:
        sro = dtg.train.SyncReplicasOptimizer(opt, world, world, bucket_mb=0.001)
        op = sro.minimize(_loss_fn(kind, m), global_step=gs, inputs=phs, **kw)
        assert len(sro.dp.buckets) > 2
        hooks.append(sro.make_session_run_hook(rank == 0))
    else:
        op = opt.minimize(_loss_fn(kind, m), global_step=gs, inputs=phs, **kw)
    losses = []
    with dtg.train.MonitoredTrainingSession(is_chief=rank == 0, hooks=hooks) as sess:
        for step in range(steps):
            feed = dict(zip(phs, _rows(_records(kind, step, total), rank * rows, (rank + 1) * rows)))
            _, loss = sess.run([op, op.loss], feed_dict=feed)
            losses.append(float(loss))
        assert int(sess.run(gs)) == steps
    assert opt.step_count == steps
    return _snapshot(flat, buffers), op, losses


# ---- 2. accum_steps=1 is the plain path -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,optname", [("resnet", "momentum"), ("bert", "lamb")])
def test_accum_steps_1_is_the_plain_path(kind, optname):
    plain, _, la = _train(kind, optname, None, 2 * B, 3, 2 * B, buffers=True)
    one, op, lb = _train(kind, optname, 1, 2 * B, 3, 2 * B, buffers=True)
    _assert_same(plain, one, kind)
    assert la == lb
    assert op.accum is None and op.grads.accum is None  # no accumulator, so nothing it could have allocated
    acc = GradAccumulator(_make(kind)[1], 1)
    acc.begin()
    acc.end()
    assert acc.acc == {} and acc.micro == 0


# ---- 3. one rank x A=2 x 2B == two ranks x B ------------------------------------------------------------------------
def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DTG_WATCHDOG="0")
    torch.set_num_threads(1)
    from dtg.parallel import comm
    comm.init("gloo")


def _spawn(fn, *args, world=2):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _cluster import free_ports
    port = free_ports(1)[0]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=fn, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    res = dict(q.get(timeout=5) for _ in range(world))
    for p in procs:
        if p.is_alive():
            p.kill()
    return res


OPTS = ("momentum", "adam", "lamb")


def _rank_two_by_one(rank, world, port, q, kind, out):
    try:
        _init(rank, world, port)
        from dtg.parallel import comm
        res = {o: _train(kind, o, 1, B, 3, 2 * B, rank, world, sync=True)[0] for o in OPTS}
        if rank == 0:
            torch.save(res, out)
        comm.shutdown()
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("kind", ["resnet", "bert"])
def test_one_rank_two_micro_batches_equal_two_ranks(kind, tmp_path):
    """Bit-equal masters and optimizer slots: every micro-gradient is the same deterministic CPU code on the same
    rows, a two-term fp32 sum commutes, and both jobs scale by 0.5.  BatchNorm normalises per micro-batch here and per
    rank there -- the same rows -- so the gradients agree; the RUNNING statistics are left out: the one rank's buffers
    see both halves of the batch in turn, rank 0's only its own half."""
    out = str(tmp_path / "two.pt")
    assert _spawn(_rank_two_by_one, kind, out) == {0: "ok", 1: "ok"}
    two = torch.load(out, weights_only=True)
    for o in OPTS:
        one, op, _ = _train(kind, o, 2, 2 * B, 3, 2 * B)
        assert op.accum.steps == 2 and sorted(op.accum.acc) == ["compute", "fp32"] and op.accum.micro == 0
        assert all(a.dtype == torch.float32 for a in op.accum.acc.values())
        _assert_same(one, two[o], "%s/%s" % (kind, o))


# ---- 4. explicit loops ----------------------------------------------------------------------------------------------
def _micro_grads(kind, m, flat, chunk):
    """one micro-batch's gradient, taken from a zeroed flat buffer, as fp32 clones"""
    assert all(not g.grad.any() for g in flat)
    _loss_fn(kind, m)(*chunk).backward()
    out = [g.grad.float().clone() for g in flat]
    flat.zero_grad()
    return out


def _loop(kind, optname, steps, total, groups_of_rows, scale):
    """the reference: per step, the micro-gradients of every (lo, hi) of ``groups_of_rows`` (a list of lists: the
    inner lists are summed left to right first, then the outer one), applied with ``grads=``"""
    m, flat = _make(kind)
    opt = _opt(optname, flat)
    for step in range(steps):
        rec = _records(kind, step, total)
        outer = None
        for rows in groups_of_rows:
            inner = None
            for lo, hi in rows:
                g = _micro_grads(kind, m, flat, _rows(rec, lo, hi))
                inner = g if inner is None else [a.add_(b) for a, b in zip(inner, g)]
            outer = inner if outer is None else [a.add_(b) for a, b in zip(outer, inner)]
        opt.step(grad_scale=scale, grads=outer)
    return _snapshot(flat)


@pytest.mark.parametrize("kind,optname", [("resnet", "momentum"), ("bert", "adam"), ("bert", "lamb")])
def test_three_micro_batches_equal_the_explicit_loop(kind, optname):
    """1/3 is no power of two: the scale must be applied once, to the fp32 sum (c0 + c1) + c2"""
    got, op, _ = _train(kind, optname, 3, 3 * B, 3, 3 * B)
    want = _loop(kind, optname, 3, 3 * B, [[(0, B), (B, 2 * B), (2 * B, 3 * B)]], 1.0 / 3)
    _assert_same(got, want, "%s/%s" % (kind, optname))


def _rank_two_by_two(rank, world, port, q, out):
    try:
        _init(rank, world, port)
        from dtg.parallel import comm
        got, op, _ = _train("bert", "lamb", 2, 2 * B, 2, 4 * B, rank, world, sync=True)
        assert op.dp is op.accum.dp and op.dp._comm and op.accum.micro == 0
        torch.save(got, out % rank)
        comm.shutdown()
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def test_two_ranks_two_micro_batches_equal_the_explicit_loop(tmp_path):
    out = str(tmp_path / "r%d.pt")
    assert _spawn(_rank_two_by_two, out) == {0: "ok", 1: "ok"}
    r0, r1 = (torch.load(out % r, weights_only=True) for r in (0, 1))
    _assert_same(r0, r1, "rank 0 / rank 1")
    want = _loop("bert", "lamb", 2, 4 * B, [[(0, B), (B, 2 * B)], [(2 * B, 3 * B), (3 * B, 4 * B)]], (1.0 / 2) * (1.0 / 2))
    _assert_same(r0, want, "2 ranks x 2 micro-batches")


# ---- 5. the loader's rows -------------------------------------------------------------------------------------------
def test_loader_rows_of_a_micro_batch_are_a_rank_of_the_larger_job(tmp_path):
    from dtg.data import DeviceLoader, synthetic_image_set, write_image_shards
    images, labels = synthetic_image_set(60, size=24, classes=10, seed=3)
    write_image_shards(str(tmp_path), images, labels, per_shard=25)
    A, W, b = 3, 2, 2
    big = [DeviceLoader(str(tmp_path), A * b, 16, "cpu", world=W, rank=r, seed=5, depth=2) for r in range(W)]
    small = [DeviceLoader(str(tmp_path), b, 16, "cpu", world=W * A, rank=r, seed=5, depth=2) for r in range(W * A)]
    try:
        assert big[0].steps_per_epoch == small[0].steps_per_epoch == 5
        for step in range(7):  # into the second epoch
            parts = [s.next() for s in small]
            for r in range(W):
                x, y, idx = big[r].next()
                for i in range(A):
                    px, py, pidx = parts[r * A + i]
                    assert torch.equal(idx[i * b:(i + 1) * b], pidx), (step, r, i)
                    assert torch.equal(y[i * b:(i + 1) * b], py)
                    chunk = x[i * b:(i + 1) * b]
                    assert chunk.is_contiguous(memory_format=torch.channels_last)
                    assert torch.equal(chunk.view(torch.int16), px.view(torch.int16))
    finally:
        for l in big + small:
            l.close()


# ---- 6. BERT's masked-LM normalisation ------------------------------------------------------------------------------
def test_mlm_loss_is_normalised_by_the_steps_prediction_count():
    """A x B with each micro-batch passing num_valid / A == 1 x A*B with num_valid, up to fp32 summation.  Both
    losses are sums of the same n = A*B*P + A*B non-negative cross-entropy terms (masked-LM rows, next-sentence rows)
    in different orders and groupings, each with a few more roundings for the divisions and the final adds; a
    length-n fp32 sum of non-negative terms is within n * 2^-24 of its exact value relatively, so the two differ by at
    most 2 * (n + 8) * 2^-24 * loss."""
    A = 4
    rec = list(bert.synthetic_batch(A * B, SEQ, _bert_cfg(), "cpu", max_predictions=P, seed=5))
    rec[4] = rec[4].clone()
    rec[4][::3, 0] = -1   # unequal prediction counts per micro-batch
    rec[4][1, :] = -1
    nv = int((rec[4] >= 0).sum())
    assert nv < A * B * P and len({int((rec[4][i * B:(i + 1) * B] >= 0).sum()) for i in range(A)}) > 1
    losses = {}
    for steps in (1, A):
        G.reset_default_graph()
        m, flat = _make("bert")
        opt = FusedSGD(flat, lr=0.0, momentum=0.0)
        phs = [dtg.placeholder() for _ in range(6)]
        seen = []

        def loss_fn(*b, micro=(0, 1)):
            seen.append(micro)
            return m(*b, num_valid=nv if micro[1] == 1 else nv / micro[1])
        op = opt.minimize(loss_fn, global_step=dtg.train.get_or_create_global_step(), inputs=phs, accum_steps=steps)
        with dtg.train.MonitoredTrainingSession(hooks=[]) as sess:
            _, loss = sess.run([op, op.loss], feed_dict=dict(zip(phs, rec)))
        losses[steps] = float(loss)
        assert seen == ([(0, 1)] if steps == 1 else [(i, A) for i in range(A)])
    n = A * B * P + A * B
    bound = 2 * (n + 8) * 2.0 ** -24 * losses[1]
    print("[mlm norm] 1 x %d: %.9g   %d x %d: %.9g   |d| %.3g   bound %.3g" % (
        A * B, losses[1], A, B, losses[A], abs(losses[1] - losses[A]), bound))
    assert abs(losses[1] - losses[A]) <= bound


def test_float_num_valid_in_softmax_cross_entropy():
    logits = torch.randn(6, 5, generator=torch.Generator().manual_seed(1))
    labels = torch.tensor([0, 1, -1, 2, 3, 4])
    s = ops.softmax_cross_entropy(logits, labels, num_valid=1)
    assert torch.equal(ops.softmax_cross_entropy(logits, labels, num_valid=5), s / 5.0)  # ints: as before
    assert torch.equal(ops.softmax_cross_entropy(logits, labels, num_valid=2.5), s / 2.5)
    with pytest.raises(ValueError):
        ops.softmax_cross_entropy(logits, labels, num_valid=0.0)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def _accum_op(A):
    G.reset_default_graph()
    m, flat = _make("resnet")
    opt = _opt("momentum", flat)
    phs = [dtg.placeholder(), dtg.placeholder()]
    op = opt.minimize(_loss_fn("resnet", m), global_step=dtg.train.get_or_create_global_step(), inputs=phs,
                      accum_steps=A)
    return op, phs, flat, opt


def test_batch_not_divisible_raises_before_anything_runs():
    op, phs, flat, opt = _accum_op(3)
    before = _snapshot(flat, buffers=True)
    x, y = _records("resnet", 0, 8)
    with dtg.train.MonitoredTrainingSession(hooks=[]) as sess:
        with pytest.raises(ValueError, match="divisible by 3"):
            sess.run(op, feed_dict={phs[0]: x, phs[1]: y})
    assert opt.step_count == 0 and op.accum.acc == {} and op.accum.micro == 0
    assert torch.equal(before["buffers"], flat.buffers.flat)  # no forward ran: BN's running statistics are untouched
    assert all(torch.equal(a, g.master) for a, g in zip(before["master"], flat))
    with pytest.raises(ValueError):
        _accum_op(0)


def test_graphed_step_refuses_an_accumulating_step():
    op, phs, flat, opt = _accum_op(2)
    with pytest.raises(RuntimeError, match="accumulates gradients over 2 micro-batches"):
        GraphedStep(lambda: G.RunContext().eval(op))()
    acc = GradAccumulator(flat, 2)
    with pytest.raises(RuntimeError, match="accumulates gradients"):
        GraphedStep(acc.begin)()

    def window():
        acc.begin()
    with pytest.raises(RuntimeError, match="accumulates gradients"):
        GraphedStep(window).capture()


def test_window_protocol():
    m, flat = _make("resnet")
    acc = GradAccumulator(flat, 2)
    with pytest.raises(RuntimeError):
        acc.end()
    with pytest.raises(RuntimeError):
        acc.step(_opt("momentum", flat))
    acc.begin()
    with pytest.raises(RuntimeError):
        acc.begin()
    x, y = _records("resnet", 0, B)
    ops.softmax_cross_entropy(m(x), y).backward()
    acc.end()
    assert acc.micro == 1 and all(not g.grad.any() for g in flat)  # folded: the next backward starts from zero
    assert any(a.any() for a in acc.acc.values())
    acc.reset()
    assert acc.micro == 0
    with pytest.raises(ValueError):
        GradAccumulator(flat, 0)


# ---- 8. the examples, end to end ------------------------------------------------------------------------------------
def _clean_env():
    e = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DTG_FAULT"):
        e.pop(k, None)
    return e


def _example(script, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), *args], capture_output=True, text=True,
                       timeout=300, env=_clean_env())
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    return r.stdout


def _check_resume(first, second, ck):
    assert "done at global step 2" in first and "resumed from" not in first, first
    assert "resumed from" in second and "(global step 2)" in second and "done at global step 4" in second, second
    assert [int(s) for s in re.findall(r"^step (\d+) loss ", second, re.M)] == [3, 4], second
    r = dtg.train.NewCheckpointReader(dtg.train.latest_checkpoint(ck))
    assert int(r.get_tensor("global_step")) == 4 and int(r.get_tensor("optimizer/step")) == 4
    assert not [k for k in r.get_variable_to_shape_map() if "accum" in k]  # a window never spans a checkpoint


def test_bert_example_accumulates_checkpoints_and_resumes(tmp_path):
    from dtg.data import synthetic_token_set, write_token_meta, write_token_shards
    data, ck = str(tmp_path / "data"), str(tmp_path / "ck")
    write_token_shards(data, synthetic_token_set(48, seq=32, vocab_hi=68, seed=1, strides=(1, 2, 3, 5)), 20)
    write_token_meta(data, pad_id=0, cls_id=1, sep_id=2, mask_id=3, vocab_lo=4, vocab_hi=68)
    args = ["--tiny", "--batch", "4", "--accum_steps", "2", "--total_steps", "4", "--warmup", "2", "--opt", "lamb",
            "--clip_norm", "1.0", "--save_every", "2", "--log_every", "1", "--ckpt_dir", ck, "--data_dir", data,
            "--max_predictions", "5"]
    first = _example("BERT/bert_train.py", "--steps", "2", *args)
    second = _example("BERT/bert_train.py", "--steps", "4", *args)
    _check_resume(first, second, ck)
    assert "loader: {'batches': 2" in first  # one loader batch of accum_steps * batch rows per global step


def test_resnet_example_accumulates_checkpoints_and_resumes(tmp_path):
    ck = str(tmp_path / "ck")
    args = ["--tiny", "--batch", "4", "--accum_steps", "2", "--save_every", "2", "--log_every", "1", "--ckpt_dir", ck]
    first = _example("ResNet50/resnet50_train.py", "--steps", "2", *args)
    second = _example("ResNet50/resnet50_train.py", "--steps", "4", *args)
    _check_resume(first, second, ck)
