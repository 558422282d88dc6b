"""Gradient accumulation on the card: the grad_fold / grad_unfold kernels (csrc/include/dtg/grad_fold.cuh) against
their CPU mirrors bit for bit -- vector body, tail, scalar path, a repeated grid-stride loop, fenced views -- and the
GradAccumulator on bf16 models: the unfolded flat gradient is bf16(sum_i float(g_i)) of the micro-gradients the
backward kernels really left in the flat buffer, and the step is the existing apply on it with scale 1/A."""
import os
import re
import subprocess
import sys

import pytest
import torch

import dtg
from dtg import graph as G
from dtg import ops
from dtg.models import bert, resnet
from dtg.models.layers import Linear
from dtg.ops import optim_kernels as K
from dtg.optim import FusedLAMB, FusedSGD
from dtg.parallel import FlatParams, GradAccumulator, overlap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
FENCE = 16   # sentinel elements on both sides of every view (32 B of bf16, 64 B of fp32: the view stays aligned)
ODD = 3      # ... and an odd offset on top of it: no 16-byte alignment, the scalar kernels
IV = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


def _sweep():
    """elements one sweep of the capped grid covers, from the launch code: cap x block x 8 per lane"""
    src = open(os.path.join(ROOT, "csrc", "include", "dtg", "grad_fold.cuh")).read()
    cap = int(re.search(r"kFoldGridCap = (\d+);", src).group(1))
    block = int(re.search(r"kFoldBlock = (\d+);", src).group(1))
    return cap * block * 8


SIZES = [1, 7, 8, 9, 63, 64, 2049, _sweep() + 9]  # the last one repeats the grid-stride loop (and has a tail)
BF16_MAX = float(torch.finfo(torch.bfloat16).max)
SPECIAL_G = [float("inf"), float("-inf"), float("nan"), -0.0, BF16_MAX, 1.0, 257.0, 0.0]
SPECIAL_A = [1.0, float("inf"), 2.0, 0.0, BF16_MAX, float("nan"), 1.0 + 2.0 ** -8, -0.0]


def _values(n, seed, special, dtype):
    v = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 4
    if n >= 64:
        v[5:5 + len(special)] = torch.tensor(special)
    return v.to(dtype)


def _fenced(values, off, sentinel):
    """values on the card as a view at FENCE + off elements into a parent filled with the sentinel"""
    n = values.numel()
    parent = torch.full((FENCE + off + n + FENCE,), sentinel, dtype=values.dtype, device=DEV)
    view = parent[FENCE + off:FENCE + off + n]
    view.copy_(values)
    assert view.data_ptr() % 16 == (0 if off == 0 else (off * values.element_size()) % 16)
    return parent, view


def _fence_intact(parent, off, n, sentinel):
    p = parent.cpu()
    return bool((p[:FENCE + off] == sentinel).all() and (p[FENCE + off + n:] == sentinel).all())


def _same_bits(got, want):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = torch.isnan(want)
    return bool(torch.equal(torch.isnan(got), nan) and torch.equal(got.view(IV[got.dtype])[~nan],
                                                                   want.view(IV[want.dtype])[~nan]))


OFFSETS = [(0, 0), (ODD, ODD), (0, ODD), (ODD, 0)]  # (acc, g): aligned, both odd, one odd each


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", SIZES)
def test_grad_fold_equals_the_mirror(n, dtype):
    gv = _values(n, n, SPECIAL_G, dtype)
    av = _values(n, n + 1, SPECIAL_A, torch.float32)
    want = {}
    for first in (True, False):
        a, g = (torch.full((n,), float("nan")) if first else av.clone()), gv.clone()
        K.grad_fold_ref(a, g, first)
        want[first] = a
    for aoff, goff in OFFSETS:
        for first in (True, False):
            # with first the accumulator starts as NaN everywhere: it must not be read
            pa, a = _fenced(torch.full((n,), float("nan")) if first else av, aoff, 777.0)
            pg, g = _fenced(gv, goff, -13.0)
            K.grad_fold(a, g, first)
            what = (n, dtype, aoff, goff, first)
            assert _same_bits(a, want[first]), what
            assert bool(g.view(IV[dtype]).eq(0).all()), what  # +0.0 everywhere
            assert _fence_intact(pa, aoff, n, 777.0) and _fence_intact(pg, goff, n, -13.0), what


def _ranges(n):
    r = [(0, 0), (0, n), (n, n), (n - 1, n), (0, 1)]
    if n >= 2049:
        r += [(64, 1984), (64, 64), (5, 2000), (1, n - 3), (1024, n)]
    if n > 4096:
        r += [(64, n - n % 64), (3, n - 5)]
    return sorted(set(r))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", SIZES)
def test_grad_unfold_equals_the_mirror(n, dtype):
    gv = _values(n, n + 2, SPECIAL_G, dtype)
    av = _values(n, n + 3, SPECIAL_A, torch.float32)
    offsets = OFFSETS if n < 4096 else OFFSETS[:2]
    for lo, hi in _ranges(n):
        want = gv.clone()
        K.grad_unfold_ref(want, av, lo, hi)
        assert _same_bits(want[:lo], gv[:lo]) and _same_bits(want[hi:], gv[hi:])
        for aoff, goff in offsets:
            pa, a = _fenced(av, aoff, 777.0)
            pg, g = _fenced(gv, goff, -13.0)
            K.grad_unfold(g, a, lo, hi)
            what = (n, dtype, lo, hi, aoff, goff)
            assert _same_bits(g, want), what             # the range, and the elements outside it unchanged
            assert _same_bits(a, av), what               # acc is left as it is
            assert _fence_intact(pa, aoff, n, 777.0) and _fence_intact(pg, goff, n, -13.0), what


def test_bindings_refuse_bad_operands():
    a = torch.zeros(64, device=DEV)
    g = torch.zeros(64, device=DEV, dtype=torch.bfloat16)
    for bad in (lambda: K.grad_fold(a, g[:63], True), lambda: K.grad_unfold(g, a, 3, 65), lambda: K.grad_unfold(g, a, 9, 8),
                lambda: dtg.ops.lib().grad_fold(a, a, True), lambda: dtg.ops.lib().grad_fold(a, g.half(), True),
                lambda: dtg.ops.lib().grad_unfold(g, a[::2], 0, 32)):
        with pytest.raises(RuntimeError):
            bad()


# ---- model level, bf16 ----------------------------------------------------------------------------------------------
def _model(kind, seed=5):
    torch.manual_seed(seed)
    if kind == "resnet":
        m = resnet.resnet18_like_tiny(10).to(DEV).to(memory_format=torch.channels_last)
    elif kind == "bert":
        m = bert.BertForPreTraining(bert.BertConfig.tiny()).to(DEV)
    else:
        # a stack whose backward has no float atomics: two runs of it give the same bits (BatchNorm's and BERT's
        # bias / LayerNorm gradients reduce with float atomics, so whole runs of those models are not comparable)
        m = torch.nn.Sequential(Linear(64, 128, act="relu"), Linear(128, 128, act="relu"), Linear(128, 16)).to(DEV)
    m.train()
    return m, FlatParams(m)


def _batch(kind, n, seed):
    if kind == "resnet":
        return resnet.synthetic_batch(n, DEV, torch.bfloat16, 32, 10, seed=seed)
    if kind == "bert":
        return bert.synthetic_batch(n, 64, bert.BertConfig.tiny(), DEV, max_predictions=8, seed=seed)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 64, generator=g).to(DEV, torch.bfloat16), torch.randint(0, 16, (n,), generator=g).to(DEV)


def _loss(kind, m, b):
    return m(*b) if kind == "bert" else ops.softmax_cross_entropy(m(b[0]), b[1])


def _opt(kind, flat):
    if kind == "resnet":
        return FusedSGD(flat, lr=0.05, momentum=0.9, weight_decay=1e-4)
    return FusedLAMB(flat, lr=1e-3, clip_norm=1.0)


def _state(flat):
    s = []
    for g in flat:
        s += [g.master.clone()] + ([g.mirror.clone()] if g.mirror is not None else [])
        s += [v.clone() for _, v in sorted(g.state.items())]
    torch.cuda.synchronize()
    return s


def _expected_grad(flat, clones):
    """bf16(sum_i float(clone_i)), left to right in fp32 (the identity cast for the fp32 group)"""
    out = []
    for j, g in enumerate(flat):
        s = clones[0][j].float()
        for c in clones[1:]:
            s = s + c[j].float()
        out.append(s.to(g.grad.dtype))
    return out


@pytest.mark.parametrize("kind,A", [("resnet", 3), ("bert", 4)])
def test_window_gradient_is_the_once_rounded_sum_and_the_step_is_the_existing_apply(kind, A):
    m, flat = _model(kind)
    opt = _opt(kind, flat)
    twin_m, twin_flat = _model(kind)
    twin = _opt(kind, twin_flat)
    acc = GradAccumulator(flat, A)
    seen = []
    step = opt.step

    def hooked(*a, **kw):  # after the window's unfold, before the apply
        seen.append([g.grad.clone() for g in flat])
        return step(*a, **kw)
    opt.step = hooked
    for window in range(2):
        b = _batch(kind, 4 * A, seed=window)
        clones = []
        for i in range(A):
            acc.begin()
            _loss(kind, m, [t[4 * i:4 * (i + 1)] for t in b]).backward()
            overlap.join()
            clones.append([g.grad.clone() for g in flat])  # what the backward kernels left, before the fold
            acc.end()
            assert acc.micro == i + 1
            if i < A - 1:
                assert all(not bool(g.grad.any()) for g in flat)
        assert all(bool(c[0].any()) for c in clones)
        acc.step(opt)
        want = _expected_grad(flat, clones)
        for g, got, w in zip(flat, seen[-1], want):
            assert got.dtype == g.grad.dtype and _same_bits(got, w), (kind, window, g.name)
        # the existing apply on that gradient with scale 1/A
        for g, w in zip(twin_flat, want):
            g.grad.copy_(w)
        twin.step(grad_scale=1.0 / A)
        for x, y in zip(_state(flat), _state(twin_flat)):
            assert _same_bits(x, y), (kind, window)
        assert acc.micro == 0 and opt.step_count == twin.step_count == window + 1
        assert all(not bool(g.grad.any()) for g in flat)  # the apply zeroed it: the next window starts clean
    assert sorted(acc.acc) == ["compute", "fp32"] and all(a.dtype == torch.float32 for a in acc.acc.values())


# ---- the forced one-rank DataParallel (its own process: DTG_DDP_FORCE is read when the group is built) --------------
def test_forced_one_rank_data_parallel_buckets():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _cluster import free_ports
    env = dict(os.environ, DTG_DDP_FORCE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_ports(1)[0]), RANK="0",
               WORLD_SIZE="1", LOCAL_RANK="0")
    env.pop("DTG_COMM_EMULATE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "jobs", "accum_ddp_job.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "accum ddp ok" in r.stdout and "buckets=" in r.stdout, r.stdout[-2000:]


# ---- A = 1 on the card ----------------------------------------------------------------------------------------------
def _session_run(accum_steps):
    G.reset_default_graph()
    m, flat = _model("mlp")
    opt = FusedSGD(flat, lr=0.05, momentum=0.9, weight_decay=1e-4)
    phs = [dtg.placeholder(), dtg.placeholder()]
    kw = {} if accum_steps is None else {"accum_steps": accum_steps}
    op = opt.minimize(lambda x, y: ops.softmax_cross_entropy(m(x), y), global_step=dtg.train.get_or_create_global_step(),
                      inputs=phs, **kw)
    losses = []
    with dtg.train.MonitoredTrainingSession(hooks=[]) as sess:
        for step in range(2):
            _, loss = sess.run([op, op.loss], feed_dict=dict(zip(phs, _batch("mlp", 32, seed=step))))
            losses.append(float(loss))
    return _state(flat), losses, op


def test_accum_steps_1_on_the_card_is_the_plain_path():
    plain, la, _ = _session_run(None)
    one, lb, op = _session_run(1)
    assert op.accum is None and la == lb
    for x, y in zip(plain, one):
        assert _same_bits(x, y)
    two, lc, op2 = _session_run(2)  # and the accumulating op runs through the session on the card
    assert op2.accum.steps == 2 and all(v == v for v in lc) and op2.accum.micro == 0
