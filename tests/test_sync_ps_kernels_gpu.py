"""The synchronous PS's kernels (csrc/kernels/optim.hip): ``grad_sum`` and the k-way fused sum-apply, through
ops/optim_kernels.py, and ``_FlatOptimizer.step_sum`` on a FlatParams model."""
import pytest
import torch

import dtg  # noqa: F401
from dtg import ops
from dtg.ops import optim_kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
WRAP = 8 * 256 * 2048 + 8 + 5  # one grid-stride wrap (2048 workgroups x 256 lanes x 8 elements) plus a tail
RTOL, ATOL = 1e-5, 1e-6        # test_optim_apply's tolerances


def _srcs(k, n, dt, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(n, device=DEV, generator=g).to(dt) for _ in range(k)]


def _seq_sum(srcs, init=None):
    """The sequential fp32 sum in source order (each add rounded to fp32)."""
    s = init.clone() if init is not None else srcs[0].float().clone()
    for t in (srcs if init is not None else srcs[1:]):
        s = s + t.float()
    return s


# ---------------------------------------------------------------- grad_sum
@pytest.mark.parametrize("n", [5, 1001, WRAP])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("k", [1, 2, 7, 8])
def test_grad_sum(k, dt, n):
    srcs = _srcs(k, n, dt)
    keep = [s.clone() for s in srcs]
    ref = _seq_sum(srcs)
    # first: the old accumulator (NaN from an abandoned step) must not be read
    acc = torch.full((n,), float("nan"), device=DEV)
    K.grad_sum(acc, srcs, first=True)
    assert torch.equal(acc, ref)
    # accumulate on top (scale 1: acc + 1 * s is exact whether or not the compiler fuses the multiply-add)
    acc0 = torch.randn(n, device=DEV)
    acc = acc0.clone()
    K.grad_sum(acc, srcs, first=False)
    assert torch.equal(acc, acc0 + ref)
    # with a scale: test_axpby's tolerance (atol 1e-6, default rtol).  |sum| <= ~8 * 5, so scale * sum < 8 and a
    # fused multiply-add differs from multiply-then-add by at most half an ulp of the product, 2.4e-7.
    scale = 1.0 / 7.0
    acc = acc0.clone()
    K.grad_sum(acc, srcs, first=False, scale=scale)
    assert torch.allclose(acc, acc0 + scale * ref, atol=1e-6)
    acc = torch.full((n,), float("inf"), device=DEV)
    K.grad_sum(acc, srcs, first=True, scale=scale)
    assert torch.allclose(acc, scale * ref, atol=1e-6)
    for s, s0 in zip(srcs, keep):
        assert torch.equal(s, s0)


# ---------------------------------------------------------------- k-way sum-apply
def _apply(kind, W, srcs_or_grad, S, H, mir, gscale, acc=None, summed=False):
    """The k-way form (summed=False: srcs + acc) or the existing single-source apply on one gradient."""
    if summed:
        a = ()
        kw = dict(gscale=gscale, zero_grad=False)
        f = {"sgd": K.sgd, "momentum": K.momentum, "adagrad": K.adagrad, "adam": K.adam}[kind]
    else:
        kw = dict(gscale=gscale, acc=acc)
        f = {"sgd": K.sgd_sum, "momentum": K.momentum_sum, "adagrad": K.adagrad_sum, "adam": K.adam_sum}[kind]
    if kind == "sgd":
        f(W, srcs_or_grad, H, mir, wd=0.01, **kw)
    elif kind == "momentum":
        f(W, srcs_or_grad, S[0], H, mir, mu=0.9, wd=1e-4, nesterov=True, **kw)
    elif kind == "adagrad":
        f(W, srcs_or_grad, S[0], H, mir, eps=0.0, **kw)
    else:
        f(W, srcs_or_grad, S[0], S[1], H, mir, wd=0.01, **kw)


def _state(n, seed=11):
    g0 = torch.Generator(device="cpu").manual_seed(seed)
    w = torch.randn(n, generator=g0)
    st = [torch.rand(n, generator=g0) + 0.1 for _ in range(2)]
    acc = torch.randn(n, generator=g0)
    return w, st, acc


def _check_sum_apply(kind, dt, k, with_acc, n):
    w, st, acc0 = _state(n)
    srcs = _srcs(k, n, dt)
    hyper = torch.tensor([0.05, 3.0])
    gscale = 1.0 / k
    res = {}
    for dev in ("cpu", DEV):
        W, S, H = w.clone().to(dev), [s.clone().to(dev) for s in st], hyper.to(dev)
        A = acc0.clone().to(dev) if with_acc else None
        src = [s.clone().to(dev) for s in srcs]
        mir = torch.empty(n, dtype=torch.bfloat16, device=dev)
        _apply(kind, W, src, S, H, mir, gscale, acc=A)
        if dev == DEV:
            for s, s0 in zip(src, srcs):
                assert torch.equal(s, s0)  # the sources (and acc) are only read
            if with_acc:
                assert torch.equal(A, acc0.to(DEV))
        res[dev] = (W.cpu(), mir.cpu(), [s.cpu() for s in S])
    # the existing single-source apply, fed the fp32 sum in the same order
    W, S, H = w.clone().to(DEV), [s.clone().to(DEV) for s in st], hyper.to(DEV)
    mir = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    gsum = _seq_sum(srcs, init=acc0.to(DEV) if with_acc else torch.zeros(n, device=DEV))
    _apply(kind, W, gsum, S, H, mir, gscale, summed=True)
    res["single"] = (W.cpu(), mir.cpu(), [s.cpu() for s in S])
    wg, mg, sg = res[DEV]
    assert torch.equal(mg, wg.to(torch.bfloat16))
    for other in ("cpu", "single"):
        wo, _, so = res[other]
        assert torch.allclose(wg, wo, rtol=RTOL, atol=ATOL), (other, (wg - wo).abs().max())
        for a, b in zip(sg, so):
            assert torch.allclose(a, b, rtol=RTOL, atol=ATOL), (other, (a - b).abs().max())


@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("k", [1, 2, 7])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adagrad", "adam"])
def test_sum_apply(kind, dt, k, with_acc):
    _check_sum_apply(kind, dt, k, with_acc, n=8 * 256 * 3 + 8 + 5)  # several workgroups, a vector remainder, a tail


def test_sum_apply_grid_stride_wrap():
    _check_sum_apply("momentum", torch.bfloat16, 2, False, n=WRAP)


def test_sum_apply_on_offset_views():
    """Every operand a view at a 64-element offset into a larger buffer; nothing outside the views is written."""
    n, off, pad = 4099, 64, 64
    tot = off + n + pad
    g0 = torch.Generator(device=DEV).manual_seed(5)
    mk = lambda dt=torch.float32: torch.randn(tot, device=DEV, generator=g0).to(dt)  # noqa: E731
    Wb, Mb, Ab, mirb = mk(), mk().abs() + 0.1, mk(), mk(torch.bfloat16)
    srcb = [mk(torch.bfloat16) for _ in range(3)]
    before = [t.clone() for t in (Wb, Mb, Ab, mirb)]
    v = lambda t: t[off:off + n]  # noqa: E731
    H = torch.tensor([0.05, 1.0], device=DEV)
    Wr, Mr = v(Wb).clone(), v(Mb).clone()
    gsum = _seq_sum([v(s) for s in srcb], init=v(Ab))
    mir_r = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    K.momentum(Wr, gsum, Mr, H, mir_r, mu=0.9, wd=1e-4, gscale=1.0 / 3, zero_grad=False)
    K.momentum_sum(v(Wb), [v(s) for s in srcb], v(Mb), H, v(mirb), mu=0.9, wd=1e-4, gscale=1.0 / 3, acc=v(Ab))
    assert torch.allclose(v(Wb), Wr, rtol=RTOL, atol=ATOL)
    assert torch.allclose(v(Mb), Mr, rtol=RTOL, atol=ATOL)
    assert torch.equal(v(mirb), v(Wb).to(torch.bfloat16))
    for t, t0 in zip((Wb, Mb, Ab, mirb), before):
        assert torch.equal(t[:off], t0[:off]) and torch.equal(t[off + n:], t0[off + n:])
    assert torch.equal(Ab, before[2])


# ---------------------------------------------------------------- step_sum on a FlatParams model
def _flat_model():
    from dtg.parallel import FlatParams
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(24, 40), torch.nn.Linear(40, 9)).to(DEV)
    return FlatParams(m)


@pytest.mark.parametrize("kind", ["sgd", "momentum", "adagrad", "adam"])
def test_step_sum_spills_beyond_eight_sources(kind):
    """9 contributions (8 in the fused kernel + 1 through the fp32 spill buffer) against step() on the summed fp32
    gradient; both groups (bf16 compute, fp32 biases)."""
    from dtg.optim import make_optimizer
    fa, fb = _flat_model(), _flat_model()
    assert [g.name for g in fa] == ["compute", "fp32"]
    oa, ob = make_optimizer(kind, fa, 0.05), make_optimizer(kind, fb, 0.05)
    R = 9
    gen = torch.Generator(device=DEV).manual_seed(9)
    sources = [[torch.randn(g.numel, device=DEV, generator=gen).to(g.grad.dtype) for g in fa] for _ in range(R)]
    keep = [[t.clone() for t in s] for s in sources]
    for step in range(2):
        oa.step_sum(sources, grad_scale=1.0 / R)
        for i, g in enumerate(fb):
            g.grad = _seq_sum([s[i] for s in sources])
        ob.step(grad_scale=1.0 / R, zero_grad=False)
        assert oa.step_count == ob.step_count == step + 1
        assert torch.equal(oa.hyper, ob.hyper)
        for ga, gb in zip(fa, fb):
            assert torch.allclose(ga.master, gb.master, rtol=RTOL, atol=ATOL), (ga.name, step)
            if ga.mirror is not None:
                assert torch.equal(ga.mirror, ga.master.to(torch.bfloat16))
            assert sorted(ga.state) == sorted(gb.state)
            for key in ga.state:
                assert torch.allclose(ga.state[key], gb.state[key], rtol=RTOL, atol=ATOL), (ga.name, key)
    for s, s0 in zip(sources, keep):
        for t, t0 in zip(s, s0):
            assert torch.equal(t, t0)


def test_step_sum_adagrad_initial_accumulator_covers_the_group():
    from dtg.optim import FusedAdagrad
    flat = _flat_model()
    opt = FusedAdagrad(flat, lr=0.05)
    gen = torch.Generator(device=DEV).manual_seed(2)
    sources = [[torch.randn(g.numel, device=DEV, generator=gen).to(g.grad.dtype) for g in flat] for _ in range(2)]
    opt.step_sum(sources, grad_scale=0.5)
    for i, g in enumerate(flat):
        gs = _seq_sum([s[i] for s in sources]) * 0.5
        assert torch.allclose(g.state["acc"], 0.1 + gs * gs, rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------- bad calls: RuntimeError on the host, no launch
def test_bad_calls_raise_before_any_launch():
    lib = ops.lib()
    n = 64
    w = torch.randn(n, device=DEV)
    w0 = w.clone()
    H = torch.tensor([0.1, 1.0], device=DEV)
    f32 = [torch.ones(n, device=DEV) for _ in range(9)]
    bf = torch.ones(n, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        K.grad_sum(w, [], first=True)  # k = 0
    with pytest.raises(RuntimeError):
        K.sgd_sum(w, [], H)
    with pytest.raises(RuntimeError):
        lib.sgd_sum_apply(w, None, f32, H, 0.0, 1.0, None)  # k = 9 at the kernel binding
    with pytest.raises(RuntimeError):
        lib.grad_sum(w, f32, True, 1.0)
    with pytest.raises(RuntimeError):
        K.momentum_sum(w, [f32[0], bf], torch.zeros(n, device=DEV), H)  # mixed dtypes
    with pytest.raises(RuntimeError):
        K.grad_sum(w, [f32[0], bf], first=True)
    with pytest.raises(RuntimeError):
        K.adam_sum(w, [f32[0], torch.ones(n + 8, device=DEV)], torch.zeros(n, device=DEV),
                   torch.zeros(n, device=DEV), H)  # unequal numel
    with pytest.raises(RuntimeError):
        K.grad_sum(w, [torch.ones(n - 8, device=DEV)], first=False)
    with pytest.raises(RuntimeError):
        K.grad_sum(w[4:], [f32[0][4:]], first=True)  # 16-byte aligned only: fp32 needs 32
    torch.cuda.synchronize()
    assert torch.equal(w, w0)
