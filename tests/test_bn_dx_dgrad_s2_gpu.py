"""conv3's data gradient inside BN3's dx pass at stage 2's width (csrc/kernels/bn_dx_wgrad.hip, the full-width DG
form: 512 x 128, one workgroup owns all 512 channels of a row block; plain form only -- the dual form is not built):

    dx  = a * dp + bx * x + c                (bf16, kept on chip)
    dW += dx^T act                           (as before)
    dp2 = bits * (dx W3),  sum(dp2),  sum(dp2 * xhat2)     (what gemm_bn mode 3 computed from dx out of HBM)

against fp32 torch on the call's own inputs and against the two-kernel path it replaces."""
import functools

import pytest
import torch

import dtg  # noqa: F401
from dtg.ops._native import lib

pytestmark = pytest.mark.gpu
SLOTS = 32
C, CI = 512, 128


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _chan(n, dev, g):
    mean = (torch.randn(n, generator=g) * 0.3).to(dev)
    inv = (torch.rand(n, generator=g) + 0.5).to(dev)
    gamma = (torch.rand(n, generator=g) + 0.5).to(dev)
    beta = (torch.randn(n, generator=g) * 0.2).to(dev)
    return mean, inv, gamma, beta


def _unpack_bits(bits, n):
    k = torch.arange(8, device=bits.device, dtype=torch.int32)
    return ((bits.to(torch.int32).unsqueeze(-1) >> k) & 1).reshape(bits.shape[0], n).bool()


def _rows(kind):
    """tail: 2 G + 8 row blocks over the form's G workgroups -- 8 workgroups run 3 blocks, the rest 2 (the prefetch
    pipeline, the block loaded once more at the end); min: the smallest M bn_dx_wgrad_ok accepts, 64 row blocks, so
    most workgroups have no block."""
    if kind == "min":
        return 2048
    return 32 * (2 * lib().bn_dx_wgrad_slabs(C, CI, 0, dg=True) + 8)


@functools.lru_cache(maxsize=None)
def _case(kind):
    """Inputs, the fused call's results and both references, computed once per row count."""
    L = lib()
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(13)
    M = _rows(kind)
    assert L.bn_dx_dgrad_full_ok(M, C, CI)
    t = {"M": M}
    t["dp"], t["x"] = (torch.randn(M, C, generator=g).to(dev, torch.bfloat16) for _ in range(2))
    t["act"] = torch.rand(M, CI, generator=g).to(dev, torch.bfloat16)
    mean, inv, gamma, _ = _chan(C, dev, g)
    part = torch.zeros(SLOTS, 2, C, device=dev)
    part[0] = torch.randn(2, C, generator=g).to(dev) * 10  # non-trivial coefficients
    t["bn"] = (mean, inv, gamma, part.view(-1))
    t["w3"] = torch.randn(C, CI, generator=g).mul_(C ** -0.5).to(dev, torch.bfloat16)
    t["y2"] = torch.randn(M, CI, generator=g).to(dev, torch.bfloat16)
    t["m2"], t["i2"], t["g2"], t["b2"] = _chan(CI, dev, g)
    t["bits"] = torch.randint(0, 256, (M, CI // 8), generator=g, dtype=torch.int32).to(dev, torch.uint8)
    z = lambda: torch.zeros(C, device=dev)  # noqa: E731
    m1, i1, g1, p1 = t["bn"]
    dg = dict(dgw=t["w3"], dgy=t["y2"], dgmean=t["m2"], dginv=t["i2"], dgbits=t["bits"], dgfull=True)

    def fused(gdtype):
        w0 = (torch.randn(C, CI, generator=torch.Generator(device="cpu").manual_seed(5)) * 0.1).to(dev, gdtype)
        wg = w0.clone()
        part = torch.zeros(SLOTS * 2 * CI, device=dev)
        r = L.bn_bwd_part(t["dp"], t["x"], p1.clone(), g1, m1, i1, False, z(), z(), wact=t["act"], wgrad=wg,
                          dgpart=part, **dg)
        assert r[0] is None and len(r) == 6
        return dict(w0=w0, wg=wg, dp2=r[4], part=r[5])

    t["f32"], t["bf16"] = fused(torch.float32), fused(torch.bfloat16)
    # the path it replaces: the dx pass with the fused weight gradient only, then gemm_bn mode 3 with the packed mask
    wg_two = t["f32"]["w0"].clone()
    t["dx"] = L.bn_bwd_part(t["dp"], t["x"], p1.clone(), g1, m1, i1, False, z(), z(), wact=t["act"], wgrad=wg_two)[0]
    t["wg_two"] = wg_two
    t["dp2_two"], t["part_two"] = L.gemm_bn(t["dx"], t["w3"], 3, t["y2"], t["m2"], t["i2"], t["g2"], t["b2"],
                                            mask=t["bits"])
    # fp32 torch from the call's inputs: dx = gamma inv (dp - s / M - xhat q / M), never rounded to bf16
    keep = _unpack_bits(t["bits"], CI)
    t["keep"] = keep
    t["dp2_ref"] = torch.where(keep, _dx_f32(t) @ t["w3"].float(), torch.zeros((), device=dev))
    t["s_ref"] = t["dp2_ref"].sum(0)
    t["q_ref"] = (t["dp2_ref"] * ((t["y2"].float() - t["m2"]) * t["i2"])).sum(0)
    torch.cuda.synchronize()
    return t


def _dx_f32(t):
    m1, i1, g1, p1 = t["bn"]
    s, q = p1.view(SLOTS, 2, C).sum(0)
    return g1 * i1 * (t["dp"].float() - s / t["M"] - (t["x"].float() - m1) * i1 * q / t["M"])


KINDS = ["tail", "min"]


@pytest.mark.parametrize("kind", KINDS)
def test_dx_dgrad_s2_dp2_and_partials(kind):
    """dp2, sum(dp2) and sum(dp2 * xhat2): relative error below 1e-2 against fp32 torch (the bound
    test_gemm_bn_bwd_stats uses for the same quantities) and against the two-kernel path; dp2 exactly zero where
    the mask bit is clear.  At 64 row blocks most workgroups have none: the totals only match if those add
    nothing."""
    t = _case(kind)
    assert _rel(t["dx"], _dx_f32(t)) < 1e-2  # the reference's own dx formula against the unfused pass
    for f in (t["f32"], t["bf16"]):
        dp2 = f["dp2"]
        s, q = f["part"].view(SLOTS, 2, CI).sum(0)
        s2, q2 = t["part_two"].view(SLOTS, 2, CI).sum(0)
        errs = dict(dp2=_rel(dp2, t["dp2_ref"]), s=_rel(s, t["s_ref"]), q=_rel(q, t["q_ref"]),
                    dp2_two=_rel(dp2, t["dp2_two"]), s_two=_rel(s, s2), q_two=_rel(q, q2))
        print(kind, t["M"], errs)
        assert torch.isfinite(f["part"]).all().item()
        assert max(errs.values()) < 1e-2, errs
        assert (dp2[~t["keep"]] == 0).all().item()
        assert dp2.shape == (t["M"], CI) and dp2.dtype == torch.bfloat16


@pytest.mark.parametrize("kind", KINDS)
def test_dx_dgrad_s2_weight_gradient(kind):
    """dW stays within test_bn_dx_wgrad_fused's bounds: 1e-4 for fp32 and 5e-3 for bf16 gradients against fp32 torch
    on the bf16 dx of the unfused pass."""
    t = _case(kind)
    for f, tol in ((t["f32"], 1e-4), (t["bf16"], 5e-3)):
        e = _rel(f["wg"], f["w0"].float() + t["dx"].float().t() @ t["act"].float())
        print(kind, "dW", e, "against the sliced pass", _rel(f["wg"], t["wg_two"]))
        assert e < tol


@pytest.mark.parametrize("kind", KINDS)
def test_dx_dgrad_s2_partial_slots_return_zeroed(kind):
    """The pool contract: the finalize that consumes the partials leaves every slot zero."""
    t = _case(kind)
    L = lib()
    f = t["f32"]
    part = f["part"].clone()
    assert part.abs().sum().item() > 0
    L.bn_bwd_part(f["dp2"], t["y2"], part, t["g2"], t["m2"], t["i2"], False, None, None)
    assert (part == 0).all().item()


def test_dx_dgrad_s2_predicate_and_refusal():
    L = lib()
    assert L.bn_dx_dgrad_full_ok(2048, 512, 128) and L.bn_dx_dgrad_full_ok(32 * 1000, 512, 128)
    assert not L.bn_dx_dgrad_full_ok(2048 + 8, 512, 128) and not L.bn_dx_dgrad_full_ok(2048 + 16, 512, 128)
    assert not L.bn_dx_dgrad_full_ok(1024, 512, 128)
    assert not L.bn_dx_dgrad_full_ok(2048, 256, 64) and not L.bn_dx_dgrad_full_ok(2048, 512, 64)
    assert L.bn_dx_wgrad_slabs(512, 128, 0, dg=True) % 8 == 0
    dev = torch.device("cuda")
    bf = lambda *s: torch.zeros(*s, device=dev, dtype=torch.bfloat16)  # noqa: E731
    fz = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731

    def call(M, c, ci, **kw):
        return L.bn_bwd_part(bf(M, c), bf(M, c), fz(SLOTS * 2 * c), fz(c) + 1, fz(c), fz(c) + 1, False, fz(c), fz(c),
                             dgw=bf(c, ci), dgy=bf(M, ci), dgmean=fz(ci), dginv=fz(ci) + 1,
                             dgbits=torch.zeros(M, ci // 8, device=dev, dtype=torch.uint8),
                             dgpart=fz(SLOTS * 2 * ci), dgfull=True, **kw)

    with pytest.raises(RuntimeError):  # a refused shape: stage 1's belongs to the sliced forms
        call(2048, 256, 64, wact=bf(2048, 64), wgrad=fz(256, 64))
    with pytest.raises(RuntimeError):  # too few rows
        call(1024, C, CI, wact=bf(1024, CI), wgrad=fz(C, CI))
    with pytest.raises(RuntimeError):  # the dgrad rides on the fused weight gradient
        call(2048, C, CI)
    with pytest.raises(RuntimeError):  # no dual form at this width
        M = 2048
        L.bn_bwd2_part(bf(M, C), bf(M, C), fz(SLOTS * 2 * C), fz(C) + 1, fz(C), fz(C) + 1, fz(C), fz(C), bf(M, C),
                       fz(SLOTS * 2 * C), fz(C) + 1, fz(C), fz(C) + 1, fz(C), fz(C), wact=bf(M, CI), wgrad=fz(C, CI),
                       dgw=bf(C, CI), dgy=bf(M, CI), dgmean=fz(CI), dginv=fz(CI) + 1,
                       dgbits=torch.zeros(M, CI // 8, device=dev, dtype=torch.uint8), dgpart=fz(SLOTS * 2 * CI),
                       dgfull=True)


def test_dx_dgrad_s2_model_path(monkeypatch):
    """Stage-2 bottlenecks (projection 256 -> 512 at width 128 and stride 2, then two identity blocks; 2 x 64 x 64
    in, 2048 rows after the stride) with _DXD_S2 on and off: the input gradient and every parameter gradient agree
    within the tolerance of test_dx_dgrad_model_path.  A block takes the fused path only for a gradient that the
    NEXT block's last dgrad wrote (the BN3 link), so a third block follows; the path counter shows that the one
    covered identity block ran the plain form (the projection block has no fused form at this width)."""
    from dtg.models.resnet import Bottleneck
    from dtg.models import resnet_fused
    from dtg.parallel import FlatParams
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1)
    x0 = torch.randn(2, 256, 64, 64, generator=g).to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    gy = None
    outs, grads, calls = [], [], []
    for on in (False, True):
        monkeypatch.setattr(resnet_fused, "_DXD_S2", on)
        monkeypatch.setattr(resnet_fused, "_dxd_calls", 0)
        torch.manual_seed(0)
        bl = torch.nn.Sequential(Bottleneck(256, 128, 2), Bottleneck(512, 128, 1), Bottleneck(512, 128, 1))
        bl = bl.to(dev).to(memory_format=torch.channels_last)
        for b in bl:
            for bn in (b.c1.bn, b.c2.bn, b.c3.bn):
                bn.weight.data.uniform_(0.5, 1.5)
        bl.train()
        FlatParams(bl)
        x = x0.clone().requires_grad_()
        y = bl(x)
        if gy is None:
            gy = torch.randn(y.shape, generator=g).to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last)
        y.backward(gy)
        outs.append(y.float())
        grads.append([x.grad.float()] + [p.grad.float().clone() for p in bl.parameters()])
        calls.append(resnet_fused._dxd_calls)
    assert calls == [0, 1], calls
    assert torch.equal(outs[0], outs[1])  # the switch changes the backward only
    errs = [_rel(ga, gb) for ga, gb in zip(grads[1], grads[0])]
    print("model path", max(errs))
    assert max(errs) < 3e-2, errs
