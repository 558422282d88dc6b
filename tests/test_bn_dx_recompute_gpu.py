"""BN3's fused dx pass without its read of x (csrc/kernels/bn_dx_wgrad.hip, the RX forms; stage 1: 256 x 64): with
dgx=True the caller vouches that x = bf16(wact dgw^T), the forward's conv3 output, and the pass forms each block's x
again by MFMA from the act block and the weight it holds anyway.

The reference is the same binding without dgx on the same operands, which this keyword leaves untouched.  x comes from
the library's own forward, gemm_bn(act, w3, 1); both products are two 32-deep MFMA steps over the same k order, so the
recomputed x equals the stored one and every result except the atomically summed BN2 partials is bit-equal.  The dgx
calls are handed an x full of NaN: they cannot have read it.  Then the model path."""
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
C, CI = 256, 64


def _chan(n, dev, g):
    mean = (torch.randn(n, generator=g) * 0.3).to(dev)
    inv = (torch.rand(n, generator=g) + 0.5).to(dev)
    gamma = (torch.rand(n, generator=g) + 0.5).to(dev)
    return mean, inv, gamma


def _unpack_bits(bits, n):
    k = torch.arange(8, device=bits.device, dtype=torch.int32)
    return ((bits.to(torch.int32).unsqueeze(-1) >> k) & 1).reshape(bits.shape[0], n).bool()


def _rows(kind, dual):
    """tail: 2 G + 8 row blocks over G workgroups -- 8 workgroups run 3 blocks, the rest 2 (the pipeline, both LDS
    slots, the last block's wait path); min: 64 row blocks, so most workgroups have none."""
    if kind == "min":
        return 2048
    return 32 * (2 * lib().bn_dx_wgrad_slabs(C, CI, int(dual), dg=True) + 8)


@functools.lru_cache(maxsize=None)
def _case(kind, dual):
    """Inputs and, per gradient dtype, the reference call (no dgx) and the recomputing call, once per shape and form."""
    L = lib()
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(23)
    M = _rows(kind, dual)
    assert L.bn_dx_recompute_ok(M, C, CI, dual)
    t = {"M": M}
    t["dp"], t["x2"] = (torch.randn(M, C, generator=g).to(dev, torch.bfloat16) for _ in range(2))
    t["act"], t["act2"] = (torch.rand(M, CI, generator=g).to(dev, torch.bfloat16) for _ in range(2))
    t["w3"] = torch.randn(C, CI, generator=g).mul_(CI ** -0.5).to(dev, torch.bfloat16)
    t["x"] = L.gemm_bn(t["act"], t["w3"], 1)[0]  # the forward's conv3, its partials in a buffer of its own
    assert t["x"].shape == (M, C) and t["x"].dtype == torch.bfloat16

    def chan():
        mean, inv, gamma = _chan(C, dev, g)
        part = torch.zeros(SLOTS, 2, C, device=dev)
        part[0] = torch.randn(2, C, generator=g).to(dev) * 10  # non-trivial coefficients
        return mean, inv, gamma, part.view(-1)

    m1, i1, g1, p1 = t["bn"] = chan()
    md, idd, gd, pd = chan()
    t["y2"] = torch.randn(M, CI, generator=g).to(dev, torch.bfloat16)
    t["m2"], t["i2"], t["g2"] = _chan(CI, dev, g)
    t["bits"] = torch.randint(0, 256, (M, CI // 8), generator=g, dtype=torch.int32).to(dev, torch.uint8)
    t["keep"] = _unpack_bits(t["bits"], CI)
    z = lambda: torch.zeros(C, device=dev)  # noqa: E731
    dg = dict(dgw=t["w3"], dgy=t["y2"], dgmean=t["m2"], dginv=t["i2"], dgbits=t["bits"])
    nan = torch.full_like(t["x"], float("nan"))

    def call(gdtype, dgx):
        w0 = (torch.randn(C, CI, generator=torch.Generator(device="cpu").manual_seed(5)) * 0.1).to(dev, gdtype)
        wg, wg2 = w0.clone(), w0.clone()
        part = torch.zeros(SLOTS * 2 * CI, device=dev)
        kw = dict(dgpart=part, **dg, **({"dgx": True} if dgx else {}))
        x = nan if dgx else t["x"]
        if dual:
            r = L.bn_bwd2_part(t["dp"], x, p1.clone(), g1, m1, i1, z(), z(), t["x2"], pd.clone(), gd, md, idd, z(), z(),
                               wact=t["act"], wgrad=wg, wact2=t["act2"], wgrad2=wg2, **kw)
            assert r[0] is None and len(r) == 4
            return dict(w0=w0, wg=wg, wg2=wg2, dx2=r[1], dp2=r[2], part=r[3])
        r = L.bn_bwd_part(t["dp"], x, p1.clone(), g1, m1, i1, False, z(), z(), wact=t["act"], wgrad=wg, **kw)
        assert r[0] is None and len(r) == 6
        return dict(w0=w0, wg=wg, dp2=r[4], part=r[5])

    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        t["ref_" + name], t["new_" + name] = call(dt, False), call(dt, True)
    torch.cuda.synchronize()
    return t


KINDS = [("tail", False), ("min", False), ("tail", True), ("min", True)]
IDS = ["plain-tail", "plain-min", "dual-tail", "dual-min"]


@pytest.mark.parametrize("kind,dual", KINDS, ids=IDS)
def test_recompute_equals_the_pass_that_reads_x(kind, dual):
    """dp2, dW (fp32 and bf16) and the dual form's dW2 and dx2 are torch.equal to the reference's; dp2 is exactly zero
    where the mask bit is clear."""
    t = _case(kind, dual)
    for name in ("f32", "bf16"):
        ref, new = t["ref_" + name], t["new_" + name]
        keys = ["dp2", "wg"] + (["wg2", "dx2"] if dual else [])
        diff = {k: int((new[k].float() != ref[k].float()).sum().item()) for k in keys}
        print(kind, dual, name, t["M"], "differing elements", diff)
        assert torch.isfinite(new["dp2"].float()).all().item() and torch.isfinite(new["wg"].float()).all().item()
        for k in keys:
            assert torch.equal(new[k], ref[k]), (k, diff)
        assert (new["dp2"][~t["keep"]] == 0).all().item()
        assert new["dp2"].shape == (t["M"], CI) and new["dp2"].dtype == torch.bfloat16
        assert ref["dp2"].abs().sum().item() > 0 and not torch.equal(ref["wg"], ref["w0"])


@pytest.mark.parametrize("kind,dual", KINDS, ids=IDS)
def test_recompute_bn2_partials_within_the_reference_spread(kind, dual):
    """BN2's backward partials are atomic sums in arrival order.  The two reference calls (they differ in the weight
    gradient's dtype only, which these sums do not see) show the spread of that; the recomputing pass forms the same
    sums in another order and may differ from a reference by twice that spread (relative L2 over all slots)."""
    t = _case(kind, dual)
    spread = _rel(t["ref_f32"]["part"], t["ref_bf16"]["part"])
    for name in ("f32", "bf16"):
        d = _rel(t["new_" + name]["part"], t["ref_" + name]["part"])
        tot = _rel(t["new_" + name]["part"].view(SLOTS, 2, CI).sum(0), t["ref_" + name]["part"].view(SLOTS, 2, CI).sum(0))
        print(kind, dual, name, "partials: reference spread %.3e, recompute against reference %.3e, totals %.3e"
              % (spread, d, tot))
        assert torch.isfinite(t["new_" + name]["part"]).all().item()
        assert d <= 2 * spread


@pytest.mark.parametrize("kind,dual", KINDS[:3], ids=IDS[:3])
def test_recompute_partial_slots_return_zeroed(kind, dual):
    """The pool contract: the finalize that consumes the partials leaves every slot zero."""
    t = _case(kind, dual)
    f = t["new_f32"]
    part = f["part"].clone()
    assert part.abs().sum().item() > 0
    lib().bn_bwd_part(f["dp2"], t["y2"], part, t["g2"], t["m2"], t["i2"], False, None, None)
    assert (part == 0).all().item()


def test_recompute_predicate_and_refusals():
    L = lib()
    for dual in (False, True):
        assert L.bn_dx_recompute_ok(2048, 256, 64, dual) and L.bn_dx_recompute_ok(32 * 1000, 256, 64, dual)
        assert not L.bn_dx_recompute_ok(2048, 512, 128, dual)  # the full-width form's is not built
        assert not L.bn_dx_recompute_ok(1024, 256, 64, dual) and not L.bn_dx_recompute_ok(2048 + 8, 256, 64, dual)
        assert not L.bn_dx_recompute_ok(2048, 256, 128, dual)
    dev = torch.device("cuda")
    bf = lambda *s: torch.zeros(*s, device=dev, dtype=torch.bfloat16)  # noqa: E731
    fz = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    u8 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.uint8)  # noqa: E731

    def plain(M, c, ci, wact=True, dgw=True, **kw):
        fused = dict(wact=bf(M, ci), wgrad=fz(c, ci)) if wact else {}
        if dgw:
            fused.update(dgw=bf(c, ci), dgy=bf(M, ci), dgmean=fz(ci), dginv=fz(ci) + 1, dgbits=u8(M, ci // 8),
                         dgpart=fz(SLOTS * 2 * ci))
        return L.bn_bwd_part(bf(M, c), bf(M, c), fz(SLOTS * 2 * c), fz(c) + 1, fz(c), fz(c) + 1, False, fz(c), fz(c),
                             **fused, **kw)

    def dual(M, c, ci, wact=True, dgw=True, **kw):
        fused = dict(wact=bf(M, ci), wgrad=fz(c, ci), wact2=bf(M, ci), wgrad2=fz(c, ci)) if wact else {}
        if dgw:
            fused.update(dgw=bf(c, ci), dgy=bf(M, ci), dgmean=fz(ci), dginv=fz(ci) + 1, dgbits=u8(M, ci // 8),
                         dgpart=fz(SLOTS * 2 * ci))
        return L.bn_bwd2_part(bf(M, c), bf(M, c), fz(SLOTS * 2 * c), fz(c) + 1, fz(c), fz(c) + 1, fz(c), fz(c), bf(M, c),
                              fz(SLOTS * 2 * c), fz(c) + 1, fz(c), fz(c) + 1, fz(c), fz(c), **fused, **kw)

    assert len(plain(2048, C, CI, dgx=True)) == 6 and len(dual(2048, C, CI, dgx=True)) == 4
    assert len(plain(2048, C, CI, dgx=False)) == 6  # the keyword's default
    for call in (plain, dual):
        for bad in (lambda: call(2048, C, CI, dgw=False, dgx=True),               # no fused dgrad to ride on
                    lambda: call(2048, C, CI, wact=False, dgw=False, dgx=True),
                    lambda: call(2048, C, CI, wact=False, dgx=True),              # no conv input to recompute from
                    lambda: call(2048, 512, 128, dgx=True)):                      # 512 x 128: not built
            with pytest.raises(RuntimeError, match="dgx"):
                bad()
    with pytest.raises(RuntimeError, match="dgx"):
        plain(2048, 512, 128, dgfull=True, dgx=True)


def _chain(dev):
    """Stage 1 as the model has it: three bottlenecks (the first with a projection) and the block that follows them,
    stage 2's first.  A block's dx pass is the fused one only for a gradient that the NEXT block's last dgrad wrote (the
    BN3 link), so the three-block chain alone would leave its last block on the unlinked path."""
    from dtg.models.resnet import Bottleneck, chain_blocks
    from dtg.parallel import FlatParams
    torch.manual_seed(0)
    chain = torch.nn.Module()
    chain.blocks = torch.nn.Sequential(Bottleneck(64, 64, 1), Bottleneck(256, 64, 1), Bottleneck(256, 64, 1),
                                       Bottleneck(256, 128, 2))
    chain_blocks(chain.blocks)
    chain = chain.to(dev).to(memory_format=torch.channels_last)
    _seed_bn(chain)
    FlatParams(chain)
    chain.train()
    return chain


@functools.lru_cache(maxsize=None)
def _chain_io():
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(2)
    x0 = torch.randn(2, 64, 56, 56, generator=g).to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(2, 512, 28, 28, generator=g).to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return x0, gy


def _run_chain(touch_w3=False):
    """One forward and backward of the chain (2 x 64 x 56 x 56 in: 6272 rows in stage 1) and its errors against
    F.conv2d / F.batch_norm in fp32 with the bf16 storage points emulated."""
    dev = torch.device("cuda")
    x0, gy = _chain_io()
    chain = _chain(dev)
    x = x0.clone().requires_grad_()
    out = chain.blocks(x)
    if touch_w3:  # the same values, but no longer the tensor version the forward multiplied by
        with torch.no_grad():
            for blk in chain.blocks[:3]:
                blk.c3.conv.weight.add_(0)
    out.backward(gy)
    torch.cuda.synchronize()
    P = _ref_params(chain, True)
    xr = x0.float().requires_grad_()
    h = xr
    for i, blk in enumerate(chain.blocks):
        h = _ref_block(P, h, "blocks.%d" % i, blk, bf16=True)
    h.backward(gy.float())
    e = {n: _rel(p.grad.float(), P[n].grad) for n, p in chain.named_parameters()}
    return _rel(out.float(), h.detach()), _rel(x.grad.float(), xr.grad), e


def _check_chain_bounds(tag, e_out, e_dx, e):
    worst = sorted(e.items(), key=lambda kv: -kv[1])[:4]
    print("%s: out %.4f dx %.4f | param grads median %.4f max %.4f %s"
          % (tag, e_out, e_dx, _med(e.values()), worst[0][1], worst[0][0]))
    assert e_out < 1e-2 and e_dx < 6e-2  # test_bottleneck_chain_matches_fp32_reference's bounds
    assert _med(e.values()) <= 6e-2 and max(e.values()) <= 0.15, worst


def test_recompute_model_chain(monkeypatch):
    """With the size threshold at 0 the three stage-1 blocks recompute y3 (the projection block in the dual form, the
    identity blocks in the plain form); input and parameter gradients stay within the chain bounds of the fp32
    reference with _DXR on and off."""
    from dtg.models import resnet_fused
    monkeypatch.setattr(resnet_fused, "_DXR_MIN_BYTES", 0)
    for on in (False, True):
        monkeypatch.setattr(resnet_fused, "_DXR", on)
        monkeypatch.setattr(resnet_fused, "_dxr_calls", 0)
        monkeypatch.setattr(resnet_fused, "_dxd_calls", 0)
        r = _run_chain()
        print("_DXR", on, "fused dgrad passes", resnet_fused._dxd_calls, "recomputing", resnet_fused._dxr_calls)
        assert resnet_fused._dxd_calls == 3
        assert resnet_fused._dxr_calls == (3 if on else 0)
        _check_chain_bounds("_DXR %s" % on, *r)


def test_recompute_model_stale_weight_takes_the_old_path(monkeypatch):
    """A w3 modified in place between forward and backward is not the weight y3 was computed with: the pass reads y3."""
    from dtg.models import resnet_fused
    monkeypatch.setattr(resnet_fused, "_DXR_MIN_BYTES", 0)
    monkeypatch.setattr(resnet_fused, "_dxr_calls", 0)
    r = _run_chain(touch_w3=True)
    assert resnet_fused._dxr_calls == 0
    _check_chain_bounds("stale w3", *r)


def test_recompute_model_default_threshold(monkeypatch):
    """6272 x 256 bf16 is 3 MB, far below the Infinity Cache's size: nothing is recomputed (and no predicate asked --
    tests/test_resnet_plan_gpu.py holds the recorded launch plans to that)."""
    from dtg.models import resnet_fused
    assert resnet_fused._DXR and resnet_fused._DXR_MIN_BYTES == 256 << 20
    monkeypatch.setattr(resnet_fused, "_dxr_calls", 0)
    monkeypatch.setattr(resnet_fused, "_dxd_calls", 0)
    r = _run_chain()
    assert resnet_fused._dxd_calls == 3 and resnet_fused._dxr_calls == 0
    _check_chain_bounds("default threshold", *r)
