"""csrc/kernels/layerwise.hip on the GPU: the per-tensor reductions, the layer-wise applies and whole steps of
FusedLAMB / FusedLARS / clipping, on the smallest shapes at which these kernels can go wrong -- one flat group of
parameters of 1, 63, 64, 65, CHUNK-1, CHUNK, CHUNK+1 and 3*CHUNK+5 elements (a lone element, the 64-element alignment
and the 8-element vector on both sides, a chunk on both sides, several chunks with a scalar tail), in mixed order,
with bf16 and fp32 gradients.  The per-chunk launches do not cap their grid (one workgroup per chunk)."""
import os
import sys

import pytest
import torch

import dtg  # noqa: F401
from dtg.ops import layerwise as L
from dtg.ops import optim_kernels as K
from dtg.optim import FusedAdam, FusedLAMB, FusedLARS
from dtg.parallel import FlatParams, GraphedStep

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_layerwise_optim_cpu import Toy, _grads, _reference, _set_grads  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
C = L.CHUNK
SIZES = [65, 1, 3 * C + 5, C - 1, 64, C + 1, 63, C]
U = 2.0 ** -24  # fp32 unit roundoff


class Bag(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(n)) for n in reversed(SIZES)])


def _bag(dtype, device, seed=0):
    """One flat group (every parameter in ``compute``) holding SIZES in that order, with random master / gradient."""
    flat = FlatParams(Bag(), compute_dtype=dtype, keep_fp32=lambda n, p: False, device=torch.device(device))
    g = flat.groups["compute"]
    assert [p.numel() for p in g.params] == SIZES
    gen = torch.Generator().manual_seed(seed)
    g.master.copy_(torch.randn(g.numel, generator=gen) * 0.3)
    g.grad.copy_(torch.randn(g.numel, generator=gen) * 0.05)
    g.refresh_mirror()
    return flat, g


def _rows(g):
    return [(o, p.numel()) for o, p in zip(g.offsets, g.params)]


def _pad_mask(g):
    m = torch.ones(g.numel, dtype=torch.bool)
    for o, n in _rows(g):
        m[o:o + n] = False
    return m


def test_exported_constants():
    lib = dtg.ops.lib()
    assert (lib.LW_CHUNK, lib.LW_SERIAL, lib.LW_TREE_DEPTH) == (L.CHUNK, L.SERIAL, L.TREE_DEPTH)
    assert L.CHUNK == 256 * L.SERIAL


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_norms_within_fp32_summation_bound_and_deterministic(dtype):
    """Partials and finalized per-tensor sums of squares against fp64.  Allowed relative error: the worst-case fp32
    summation bound of the kernel's own structure, (s + 8 + k) * 2^-24 -- s serial operations per lane per chunk,
    8 tree levels over the 256 lanes, k chunks per parameter (k = 0 for a single chunk's partial)."""
    flat, g = _bag(dtype, DEV)
    plan = L.LayerwisePlan(flat)
    span = plan.span(g)
    assert plan.n_chunks == sum((n + C - 1) // C for n in SIZES) and span.c_hi == plan.n_chunks
    outs = []
    for _ in range(2):
        plan.partials.fill_(float("nan"))  # every chunk writes its own slot: nothing needs zeroing
        L.seg_sqnorm(plan, span, g.master, g.grad)
        L.seg_finalize(plan, L.LAMB, [True], [0.0], clip_norm=0.01, gscale=0.5)
        outs.append([plan.partials.clone(), plan.norms.clone(), plan.ratio.clone(), plan.cfac.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))  # same input, same bits
    part = plan.partials.cpu().double().view(2, -1)
    norms = plan.norms.cpu().double()
    w64, g64 = g.master.cpu().double(), g.grad.cpu().double()
    ci = 0
    worst = 0.0
    for r, (o, n) in enumerate(_rows(g)):
        k = (n + C - 1) // C
        for j in range(k):
            for slot, x in ((0, w64), (1, g64)):
                want = float(x[o + j * C:o + min(n, (j + 1) * C)].square().sum())
                err = abs(float(part[slot, ci]) - want) / want
                print("chunk", ci, "slot", slot, "rel err", err, "bound", (L.SERIAL + L.TREE_DEPTH) * U)
                assert err <= (L.SERIAL + L.TREE_DEPTH) * U
            ci += 1
        for slot, x in ((0, w64), (1, g64)):
            want = float(x[o:o + n].square().sum())
            err = abs(float(norms[r, slot]) - want) / want
            worst = max(worst, err)
            print("row", r, "numel", n, "slot", slot, "rel err", err, "bound", (L.SERIAL + L.TREE_DEPTH + k) * U)
            assert err <= (L.SERIAL + L.TREE_DEPTH + k) * U
        # LAMB ratio over the two slots
        assert float(plan.ratio[r]) == pytest.approx((float(norms[r, 0]) / float(norms[r, 1])) ** 0.5, rel=1e-6)
    gn = 0.5 * float(sum(g64[o:o + n].square().sum() for o, n in _rows(g))) ** 0.5
    assert gn > 0.01 and float(plan.cfac[0]) == pytest.approx(0.01 / gn, rel=1e-5)
    # an absent input leaves its slot alone
    plan.partials.fill_(7.0)
    L.seg_sqnorm(plan, span, None, g.grad)
    assert bool((plan.partials[:plan.n_chunks] == 7.0).all()) and bool((plan.partials[plan.n_chunks:] != 7.0).all())


def _twin(dtype, seed=0):
    """The same group on the GPU and on the CPU, with m / v / momentum slots filled alike."""
    out = []
    for dev in (DEV, "cpu"):
        flat, g = _bag(dtype, dev, seed)
        gen = torch.Generator().manual_seed(seed + 1)
        g.state_buffer("m").copy_(torch.randn(g.numel, generator=gen) * 0.05)
        g.state_buffer("v").copy_(torch.rand(g.numel, generator=gen) * 0.01 + 1e-3)
        g.state_buffer("momentum").copy_(torch.randn(g.numel, generator=gen) * 0.01)
        plan = L.LayerwisePlan(flat)
        plan.ratio.copy_(torch.linspace(0.5, 2.0, plan.n_rows))  # a ratio table computed on the host
        plan.cfac.fill_(0.75)
        hyper = torch.tensor([1e-2, 3.0], device=dev)
        out.append((g, plan, hyper))
    return out


def _close(a, b):
    return torch.allclose(a.cpu().float(), b.float(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("zero_grad", [True, False])
def test_applies_given_ratios_match_cpu_mirror(dtype, zero_grad):
    (gg, gp, gh), (cg, cp, ch) = _twin(dtype)
    grad0 = gg.grad.clone()
    pad = _pad_mask(cg)
    # LAMB: moments (m, v, partials, gradient zeroing), then the apply with the host-made ratios
    for g, p, h in ((gg, gp, gh), (cg, cp, ch)):
        L.lamb_moments(p, p.span(g), g.master, g.grad, g.state["m"], g.state["v"], h, 0.9, 0.999, 1e-6, 0.01, 0.5,
                       clip=True, zero_grad=zero_grad)
    assert _close(gg.state["m"], cg.state["m"]) and _close(gg.state["v"], cg.state["v"])
    assert torch.allclose(gp.partials.cpu(), cp.partials, rtol=1e-5, atol=0)
    if zero_grad:
        assert float(gg.grad[~pad.to(DEV)].abs().sum()) == 0
    else:
        assert torch.equal(gg.grad, grad0)
    for g, p, h in ((gg, gp, gh), (cg, cp, ch)):
        L.lamb_apply(p, p.span(g), g.master, g.mirror, g.state["m"], g.state["v"], h, 0.9, 0.999, 1e-6, 0.01)
    assert _close(gg.master, cg.master)
    if gg.mirror is not None:
        assert torch.equal(gg.mirror, gg.master.to(torch.bfloat16))
    # LARS
    (gg, gp, gh), (cg, cp, ch) = _twin(dtype, seed=5)
    grad0 = gg.grad.clone()
    for g, p, h in ((gg, gp, gh), (cg, cp, ch)):
        L.lars_apply(p, p.span(g), g.master, g.mirror, g.grad, g.state["momentum"], h, 0.9, 1e-4, 0.5, clip=True,
                     zero_grad=zero_grad)
    assert _close(gg.master, cg.master) and _close(gg.state["momentum"], cg.state["momentum"])
    if gg.mirror is not None:
        assert torch.equal(gg.mirror, gg.master.to(torch.bfloat16))
    if zero_grad:
        assert float(gg.grad[~pad.to(DEV)].abs().sum()) == 0
    else:
        assert torch.equal(gg.grad, grad0)


def test_existing_applies_with_clip_scalar():
    """adam / momentum / sgd / adagrad with the device clip scalar == the same apply with gscale * c on the host."""
    n = 1000 * 8 + 5
    gen = torch.Generator().manual_seed(2)
    w0, g0 = torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV, torch.bfloat16)
    clip = torch.tensor([0.25], device=DEV)
    hyper = torch.tensor([1e-2, 2.0], device=DEV)
    for fn, nst in ((lambda w, g, s, **kw: K.adam(w, g, s[0], s[1], hyper, None, **kw), 2),
                    (lambda w, g, s, **kw: K.momentum(w, g, s[0], hyper, None, **kw), 1),
                    (lambda w, g, s, **kw: K.adagrad(w, g, s[0], hyper, None, **kw), 1),
                    (lambda w, g, s, **kw: K.sgd(w, g, hyper, None, **kw), 0)):
        res = []
        for kw in (dict(gscale=2.0, clip=clip), dict(gscale=0.5)):
            w, g = w0.clone(), g0.clone()
            st = [torch.full((n,), 0.1, device=DEV) for _ in range(nst)]
            fn(w, g, st, zero_grad=True, **kw)
            assert float(g.abs().sum()) == 0
            res.append([w] + st)
        assert all(torch.equal(a, b) for a, b in zip(*res))


def _toy(make, device):
    model = Toy()
    flat = FlatParams(model, compute_dtype=torch.bfloat16, device=torch.device(device))
    return model, flat, make(flat)


# lr 1e-3 for Adam: its bias correction (optim.hip) forms 1 - 0.999^t with the fast pow, 6e-5 relative at t = 1,
# which enters the weight as lr * |u| * 3e-5
STEP_CASES = {
    "lamb_clip": (lambda f: FusedLAMB(f, lr=0.01, clip_norm=1.0), dict(kind="lamb", lr=0.01, clip=1.0)),
    "lars_clip": (lambda f: FusedLARS(f, lr=0.5, weight_decay=0.01, eta=0.02, clip_norm=1.0),
                  dict(kind="lars", lr=0.5, wd=0.01, eta=0.02, clip=1.0)),
    "adam_clip": (lambda f: FusedAdam(f, lr=1e-3, clip_norm=1.0), dict(kind="adam", lr=1e-3, clip=1.0)),
}


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_three_steps_against_fp64_reference(name):
    """Three steps on the toy model (both groups, bf16 gradients in ``compute``) against the per-tensor fp64
    reference.  Tolerance: the CPU fp32 mirror's own maximum absolute error against fp64 on these inputs, times 4
    (the GPU sums in another order and fuses multiply-adds).  Mirror errors measured on these inputs:
    lamb_clip 1.56e-7, lars_clip 2.73e-7, adam_clip 1.03e-7 (weights are O(0.1 .. 1)); the test measures them again."""
    make, ref_kw = STEP_CASES[name]
    grads = _grads()
    runs, used, cs = {}, None, None
    for dev in ("cpu", DEV):
        model, flat, opt = _toy(make, dev)
        seen, c = [], []
        for gd in grads:
            _set_grads(model, gd)
            seen.append({n: p.grad.detach().cpu().double().clone() for n, p in model.named_parameters()})
            opt.step(grad_scale=0.5)
            c.append(float(opt._plan().cfac[0]))
        runs[dev] = {n: v.detach().cpu().double() for n, v in flat.named_masters()}
        if dev == "cpu":
            used, cs = seen, c
            assert cs[0] < 1.0 and cs[-1] == 1.0, cs  # clips on the first step, not on the last
        else:
            assert c == pytest.approx(cs, rel=1e-5)
            g = flat.groups["compute"]
            assert torch.equal(g.mirror, g.master.to(torch.bfloat16))
            assert all(float(x.grad.abs().sum()) == 0 for x in flat)
    want, _ = _reference(grads=used, gscale=0.5, **ref_kw)
    err = {dev: max(float((runs[dev][n] - want[n]).abs().max()) for n in want) for dev in runs}
    print(name, "max abs error vs fp64: cpu mirror", err["cpu"], "gpu", err[DEV])
    assert err["cpu"] > 0 and err[DEV] <= 4 * err["cpu"], err


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("kind", ["lamb_clip", "lars"])
def test_padding_is_never_read_or_written(dtype, kind):
    flat, g = _bag(dtype, DEV)
    opt = FusedLAMB(flat, lr=0.01, clip_norm=0.1) if kind == "lamb_clip" else FusedLARS(flat, lr=0.1, eta=0.02)
    pad = _pad_mask(g).to(DEV)
    assert int(pad.sum()) > 0
    slots = ["m", "v"] if kind == "lamb_clip" else ["momentum"]
    g.grad[pad] = float("nan")
    bufs = [g.master] + [g.state_buffer(k) for k in slots] + ([g.mirror] if g.mirror is not None else [])
    for b in bufs:
        b[pad] = 12345.0
    before = g.master.clone()
    opt.step()
    plan = opt._plan()
    assert torch.isfinite(plan.partials).all() and torch.isfinite(plan.norms).all()
    assert torch.isfinite(plan.ratio).all() and torch.isfinite(plan.cfac).all()
    assert torch.isfinite(g.master).all() and not torch.equal(g.master, before)
    for b in bufs:
        assert bool((b[pad] == 12345.0).all())
    assert bool(torch.isnan(g.grad[pad]).all()) and float(g.grad[~pad].abs().sum()) == 0


def _param_ranges(flat, seed=3):
    out = []
    for g in flat:
        offs = list(g.offsets) + [g.numel]
        out += [(g, offs[i], offs[i + 1], lambda: None) for i in range(len(g.offsets))]
    order = torch.randperm(len(out), generator=torch.Generator().manual_seed(seed)).tolist()
    return [out[i] for i in order]


@pytest.mark.parametrize("kind", ["lamb", "lamb_clip", "lars_clip", "adam_clip"])
def test_ranges_bit_equal_to_whole_step(kind):
    make = {"lamb": lambda f: FusedLAMB(f, lr=0.01), "lamb_clip": lambda f: FusedLAMB(f, lr=0.01, clip_norm=0.1),
            "lars_clip": lambda f: FusedLARS(f, lr=0.1, eta=0.02, clip_norm=0.1),
            "adam_clip": lambda f: FusedAdam(f, lr=0.01, clip_norm=0.1)}[kind]
    runs = []
    for ranged in (False, True):
        flat, g = _bag(torch.bfloat16, DEV)
        opt = make(flat)
        for s in range(2):
            g.grad.copy_(torch.randn(g.numel, generator=torch.Generator().manual_seed(40 + s)) * 0.05)
            opt.step(grad_scale=0.5, ranges=_param_ranges(flat) if ranged else None)
        runs.append([g.master.clone(), g.mirror.clone(), g.grad.clone()] + [b.clone() for b in g.state.values()] +
                    [opt._plan().ratio.clone(), opt._plan().cfac.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    with pytest.raises(ValueError, match="cuts parameter"):
        opt.step(ranges=[(g, g.offsets[2], g.offsets[2] + 64, lambda: None)])


def test_graph_capture_lamb_clip_bit_equal_to_eager():
    """An optimizer-only LAMB + clip step captured with GraphedStep (one stream); gradients refilled in place and
    the learning rate changed between replays.  The first call runs one eager warm-up step (which zeroes the
    gradient) and one replay, so the eager twin steps once on the gradient and once on zeros."""
    fills = [torch.randn(sum(-(-n // 64) * 64 for n in SIZES), generator=torch.Generator().manual_seed(60 + i)) *
             (0.5 if i == 0 else 0.002) for i in range(4)]
    runs = []
    for graphed in (False, True):
        flat, g = _bag(torch.bfloat16, DEV)
        opt = FusedLAMB(flat, lr=0.01, clip_norm=1.0)
        g.grad.copy_(fills[0])
        if graphed:
            step = GraphedStep(lambda: opt.step(), warmup=1)
            step()
        else:
            step = opt.step
            step()
            step()
        for i in range(1, 4):
            g.grad.copy_(fills[i])
            opt.set_lr(0.01 / (i + 1))
            step()
        torch.cuda.synchronize()
        # (the fills cover the alignment padding too, which no step zeroes)
        assert float(opt.hyper[1]) == 5.0 and float(g.grad[~_pad_mask(g).to(DEV)].abs().sum()) == 0
        runs.append([g.master.clone(), g.mirror.clone(), g.state["m"].clone(), g.state["v"].clone(),
                     opt._plan().ratio.clone(), opt._plan().cfac.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert torch.isfinite(runs[0][0]).all() and float(runs[0][5]) == 1.0


@pytest.mark.parametrize("kind", ["lamb_clip", "lars"])
def test_step_sum_equals_grad_sum_then_step(kind):
    make = {"lamb_clip": lambda f: FusedLAMB(f, lr=0.01, clip_norm=0.1),
            "lars": lambda f: FusedLARS(f, lr=0.1, eta=0.02)}[kind]
    runs = []
    for mode in ("sum", "grads"):
        flat, g = _bag(torch.bfloat16, DEV)
        opt = make(flat)
        for s in range(2):
            srcs = [(torch.randn(g.numel, generator=torch.Generator().manual_seed(70 + 3 * s + c)) * 0.05)
                    .to(DEV, torch.bfloat16) for c in range(3)]
            if mode == "sum":
                opt.step_sum([[x] for x in srcs], grad_scale=1.0 / 3)
            else:
                acc = torch.empty_like(g.master)
                K.grad_sum(acc, srcs, first=True)
                opt.step(grad_scale=1.0 / 3, zero_grad=False, grads=[acc])
        runs.append([g.master.clone(), g.mirror.clone()] + [b.clone() for b in g.state.values()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert torch.isfinite(runs[0][0]).all()
