"""The next block's conv1 inside BN3's forward apply pass (csrc/kernels/bn_dx_wgrad.hip, bn_apply_gemm_kernel):

    out  = relu(bn3(y3) + identity)   or   relu(bn3(y3) + bn_d(yd))        (stored, with its packed mask bits)
    y1n  = out W1n^T,  sum(y1n),  sum(y1n^2)      (what gemm_bn mode 1 computed from out read back from HBM)

against the unfused apply pass (bit for bit), fp32 torch on that out, and gemm_bn mode 1; then the model path."""
import functools
import os
import sys

import pytest
import torch

import dtg  # noqa: F401
from dtg.ops._native import lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_resnet_gpu import _med, _ref_block, _ref_params, _rel, _seed_bn  # noqa: E402

pytestmark = pytest.mark.gpu
SLOTS = 32
MOM, EPS = 0.1, 1e-5
# (C, N, two-BN form): stage 1's identity and projection blocks into a 64-wide conv1, its last block into stage 2's;
# stage 2's identity and projection blocks (the optional width, _FWD1_S2)
FORMS = [(256, 64, False), (256, 64, True), (256, 128, False), (512, 128, False), (512, 128, True)]
KINDS = ["tail", "min"]


def _rows(kind, C, n, two):
    """tail: 2 G + 8 row blocks over the form's G workgroups -- 8 workgroups run 3 blocks, the rest 2 (the prefetch
    pipeline, the block loaded once more at the end); min: the smallest M bn_apply_gemm_ok accepts, 64 row blocks, so
    most workgroups have no block."""
    if kind == "min":
        return 2048
    return 32 * (2 * lib().bn_apply_gemm_grid(C, n, two) + 8)


def _bn_inputs(x, g, dev):
    """A BN's partial slots holding the true sums of x (slot 0), its parameters and running statistics."""
    C = x.shape[1]
    part = torch.zeros(SLOTS, 2, C, device=dev)
    part[0, 0], part[0, 1] = x.float().sum(0), (x.float() ** 2).sum(0)
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev)
    beta = (torch.randn(C, generator=g) * 0.2).to(dev)
    return part.view(-1), gamma, beta, torch.zeros(C, device=dev), torch.ones(C, device=dev)


@functools.lru_cache(maxsize=None)
def _case(C, n, two, kind):
    """Inputs, the fused call's results and the references, computed once per form and row count."""
    L = lib()
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(17)
    M = _rows(kind, C, n, two)
    assert L.bn_apply_gemm_ok(M, C, n)
    x = torch.randn(M, C, generator=g).to(dev, torch.bfloat16)
    r = torch.randn(M, C, generator=g).to(dev, torch.bfloat16)
    w = torch.randn(n, C, generator=g).mul_(C ** -0.5).to(dev, torch.bfloat16)
    bn, bn2 = _bn_inputs(x, g, dev), _bn_inputs(r, g, dev)

    def run(fused):
        p, ga, be, rm, rv = (t.clone() for t in bn)
        bits = torch.zeros(M, C // 8, device=dev, dtype=torch.uint8)
        kw = dict(next_w=w, next_part=torch.zeros(SLOTS * 2 * n, device=dev)) if fused else {}
        if two:
            p2, ga2, be2, rm2, rv2 = (t.clone() for t in bn2)
            res = L.bn_fwd2_part(x, p, ga, be, rm, rv, r, p2, ga2, be2, rm2, rv2, MOM, EPS, bits=bits, **kw)
            nst, state = 5, [rm, rv, rm2, rv2, p, p2]
        else:
            res = L.bn_fwd_part(x, p, r, ga, be, rm, rv, MOM, EPS, True, bits=bits, **kw)
            nst, state = 3, [rm, rv, p]
        assert len(res) == nst + (1 if fused else 0)
        return dict(out=res[0], stats=list(res[1:nst]) + state, bits=bits, y1n=res[nst] if fused else None,
                    part=kw.get("next_part"))

    t = dict(M=M, w=w, two=run(False), fused=run(True))
    out = t["two"]["out"]
    t["y_gemm"], t["part_gemm"] = L.gemm_bn(out, w, 1)
    t["y_ref"] = out.float() @ w.float().t()
    yr = t["y_ref"].bfloat16().float()  # the statistics are those of the stored values
    t["s_ref"], t["q_ref"] = yr.sum(0), (yr * yr).sum(0)
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C,n,two", FORMS)
def test_apply_gemm_out_bits_and_statistics_are_the_unfused_pass(C, n, two, kind):
    """out, the packed mask bits, the saved and running statistics and the consumed (zeroed) partial slots are
    torch.equal to the unfused apply pass: both evaluate the same device functions."""
    t = _case(C, n, two, kind)
    a, b = t["fused"], t["two"]
    assert a["out"].abs().sum().item() > 0 and a["bits"].sum().item() > 0
    assert torch.equal(a["out"], b["out"])
    assert torch.equal(a["bits"], b["bits"])
    for u, v in zip(a["stats"], b["stats"]):
        assert torch.equal(u, v)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C,n,two", FORMS)
def test_apply_gemm_y1n_and_partials(C, n, two, kind):
    """y1n and the summed slots (sum, sum of squares of the stored values): relative error below 1e-2 against fp32
    torch on the stored out, the bound of tests/test_bn_dx_dgrad*_gpu.py; the difference from gemm_bn mode 1 is
    printed.  At 64 row blocks most workgroups have none: the totals only match if those add nothing."""
    t = _case(C, n, two, kind)
    f = t["fused"]
    y = f["y1n"]
    assert y.shape == (t["M"], n) and y.dtype == torch.bfloat16
    assert torch.isfinite(f["part"]).all().item()
    s, q = f["part"].view(SLOTS, 2, n).sum(0)
    s2, q2 = t["part_gemm"].view(SLOTS, 2, n).sum(0)
    errs = dict(y=_rel(y, t["y_ref"]), s=_rel(s, t["s_ref"]), q=_rel(q, t["q_ref"]))
    vs_gemm = dict(y=_rel(y, t["y_gemm"]), s=_rel(s, s2), q=_rel(q, q2),
                   y_max_abs=(y.float() - t["y_gemm"].float()).abs().max().item())
    print(C, n, two, kind, t["M"], errs, "against gemm_bn mode 1", vs_gemm)
    assert max(errs.values()) < 1e-2, errs


def test_apply_gemm_predicate_and_refusal():
    L = lib()
    assert L.bn_apply_gemm_ok(2048, 256, 64) and L.bn_apply_gemm_ok(2048, 256, 128) and L.bn_apply_gemm_ok(32000, 256, 64)
    assert not L.bn_apply_gemm_ok(2048 + 8, 256, 64) and not L.bn_apply_gemm_ok(2048 + 16, 256, 128)
    assert not L.bn_apply_gemm_ok(1024, 256, 64)
    assert L.bn_apply_gemm_ok(2048, 512, 128) and not L.bn_apply_gemm_ok(2048, 512, 64)
    assert not L.bn_apply_gemm_ok(2048, 512, 256) and not L.bn_apply_gemm_ok(2048, 256, 32)
    assert not L.bn_apply_gemm_ok(2048, 256, 256) and not L.bn_apply_gemm_ok(2048, 128, 64)
    for c, n, two in FORMS:
        assert L.bn_apply_gemm_grid(c, n, two) % 8 == 0
    for bad in ((256, 128, True), (512, 64, False), (256, 32, False)):  # no such form: std::invalid_argument
        with pytest.raises(ValueError):
            L.bn_apply_gemm_grid(*bad)
    dev = torch.device("cuda")
    bf = lambda *s: torch.zeros(*s, device=dev, dtype=torch.bfloat16)  # noqa: E731
    fz = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731

    def one(M, c, n, res=True, relu=True, part=True):
        return L.bn_fwd_part(bf(M, c), fz(SLOTS * 2 * c), bf(M, c) if res else None, fz(c) + 1, fz(c), fz(c), fz(c) + 1,
                             MOM, EPS, relu, next_w=bf(n, c), next_part=fz(SLOTS * 2 * n) if part else None)

    def two(M, c, n):
        return L.bn_fwd2_part(bf(M, c), fz(SLOTS * 2 * c), fz(c) + 1, fz(c), fz(c), fz(c) + 1, bf(M, c),
                              fz(SLOTS * 2 * c), fz(c) + 1, fz(c), fz(c), fz(c) + 1, MOM, EPS, next_w=bf(n, c),
                              next_part=fz(SLOTS * 2 * n))

    assert len(one(2048, 256, 64)) == 4 and len(two(2048, 256, 64)) == 6
    assert len(one(2048, 512, 128)) == 4 and len(two(2048, 512, 128)) == 6
    for bad in (lambda: one(1024, 256, 64),      # too few rows
                lambda: one(2048 + 8, 256, 64),  # not whole row blocks
                lambda: one(2048, 512, 64),      # no such shape
                lambda: one(2048, 1024, 256),    # stages 3-4 are not built
                lambda: one(2048, 256, 32),
                lambda: one(2048, 256, 64, res=False),   # the residual + relu form only
                lambda: one(2048, 256, 64, relu=False),
                lambda: one(2048, 256, 64, part=False),  # the statistics need their slot
                lambda: two(2048, 256, 128),             # no two-BN form at this width
                lambda: two(1024, 256, 64)):
        with pytest.raises(RuntimeError):
            bad()


def _ring_is_zero(like):
    """Every buffer of the pooled partial ring (csrc/bindings/ops.cc bn_part) at its full size."""
    L = lib()
    return all((L.bn_part_alloc(like, 2048, pooled=True) == 0).all().item() for _ in range(16))


# three bottlenecks of a stage, the first with a projection: (cin, width, stride of the first), input H = W
STAGES = {1: ((64, 64, 1), 56), 2: ((256, 128, 2), 64)}


def _stage1_chain(dev, stage=1):
    from dtg.models.resnet import Bottleneck, chain_blocks
    from dtg.parallel import FlatParams
    torch.manual_seed(0)
    (cin, width, st), _ = STAGES[stage]
    chain = torch.nn.Module()
    chain.blocks = torch.nn.Sequential(Bottleneck(cin, width, st), Bottleneck(4 * width, width, 1),
                                       Bottleneck(4 * width, width, 1))
    chain_blocks(chain.blocks)
    chain = chain.to(dev).to(memory_format=torch.channels_last)
    _seed_bn(chain)
    FlatParams(chain)
    chain.train()
    return chain


@pytest.mark.parametrize("stage", [1, 2])
def test_apply_gemm_model_chain(stage, monkeypatch):
    """Three stage-1 bottlenecks (2 x 64 x 56 x 56 in: 6272 rows; the first with a projection) with _FWD1 on and off,
    each against F.conv2d / F.batch_norm in fp32 with dtg's bf16 storage points emulated, within the bounds of
    test_bottleneck_chain_matches_fp32_reference; blocks 2 and 3 take their conv1 output from the block before
    them; the chain adds no state_dict keys; every pooled slot went back zeroed.  Stage 2 (2 x 256 x 64 x 64 in, 2048
    rows after the stride): the same with _FWD1_S2 on and off."""
    from dtg.models import resnet_fused
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(2)
    (cin, width, st), hw = STAGES[stage]
    x0 = torch.randn(2, cin, hw, hw, generator=g).to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(2, 4 * width, hw // st, hw // st, generator=g).to(dev, torch.bfloat16)
    gy = gy.contiguous(memory_format=torch.channels_last)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(resnet_fused, "_FWD1", on if stage == 1 else True)
        monkeypatch.setattr(resnet_fused, "_FWD1_S2", on)
        monkeypatch.setattr(resnet_fused, "_fwd1_calls", 0)
        chain = _stage1_chain(dev, stage)
        assert not any("_next" in k for k in chain.state_dict())
        assert not any("_next" in k for k, _ in chain.named_modules())
        x = x0.clone().requires_grad_()
        out = chain.blocks(x)
        assert resnet_fused._fwd1_calls == (2 if on else 0)
        out.backward(gy)
        torch.cuda.synchronize()
        names = [n for n, _ in chain.named_parameters()]
        P = _ref_params(chain, True)
        xr = x0.float().requires_grad_()
        h = xr
        for i, blk in enumerate(chain.blocks):
            h = _ref_block(P, h, "blocks.%d" % i, blk, bf16=True)
        h.backward(gy.float())
        e = {n: _rel(p.grad.float(), P[n].grad) for n, p in chain.named_parameters()}
        e_out, e_dx = _rel(out.float(), h.detach()), _rel(x.grad.float(), xr.grad)
        worst = sorted(e.items(), key=lambda kv: -kv[1])[:4]
        print("stage", stage, "switch", on, "out %.4f dx %.4f | param grads median %.4f max %.4f %s"
              % (e_out, e_dx, _med(e.values()), worst[0][1], worst[0][0]))
        assert e_out < 1e-2 and e_dx < 6e-2
        assert _med(e.values()) <= 6e-2 and max(e.values()) <= 0.15, worst
        res[on] = (out.float(), x.grad.float(), [p.grad.float().clone() for p in chain.parameters()], names)
        del out, x
        assert _ring_is_zero(x0)
    print("on against off: out %.5f dx %.5f params max %.5f"
          % (_rel(res[True][0], res[False][0]), _rel(res[True][1], res[False][1]),
             max(_rel(a, b) for a, b in zip(res[True][2], res[False][2]))))


def test_apply_gemm_model_fallbacks_leave_the_pool_zeroed(monkeypatch):
    """What a block computed ahead is used only by the very next block on that very tensor and weight.  The next block
    in eval mode: nothing is computed ahead.  The weight modified in between, or the output consumed elsewhere: the
    block runs its own gemm_bn and the pooled slot goes back zeroed."""
    from dtg.models import resnet_fused
    dev = torch.device("cuda")
    monkeypatch.setattr(resnet_fused, "_FWD1", True)
    g = torch.Generator(device="cpu").manual_seed(3)
    x0 = torch.randn(2, 64, 56, 56, generator=g).to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    chain = _stage1_chain(dev)
    b0, b1, b2 = chain.blocks
    with torch.no_grad():
        # the next block in eval mode
        monkeypatch.setattr(resnet_fused, "_fwd1_calls", 0)
        b2.eval()
        y = chain.blocks(x0)
        assert resnet_fused._fwd1_calls == 1 and not hasattr(y, "_dtg_conv1")
        b2.train()
        del y
        assert _ring_is_zero(x0)
        # reference: the chain of two with the switch off
        monkeypatch.setattr(resnet_fused, "_FWD1", False)
        want = b1(b0(x0)).float()
        monkeypatch.setattr(resnet_fused, "_FWD1", True)
        # the weight modified between the two blocks
        monkeypatch.setattr(resnet_fused, "_fwd1_calls", 0)
        y0 = b0(x0)
        ahead = y0._dtg_conv1
        assert ahead.part is not None and ahead.part.abs().sum().item() > 0
        b1.c1.conv.weight.mul_(1.0)
        y1 = b1(y0)
        assert resnet_fused._fwd1_calls == 0 and ahead.part is None
        assert _rel(y1.float(), want) < 1e-2
        del y0, y1, ahead
        assert _ring_is_zero(x0)
        # the output consumed elsewhere: a copy of it reaches the next block
        y0 = b0(x0)
        y1 = b1(y0.clone(memory_format=torch.channels_last))
        assert resnet_fused._fwd1_calls == 0
        assert _rel(y1.float(), want) < 1e-2
        del y0, y1
        assert _ring_is_zero(x0)
