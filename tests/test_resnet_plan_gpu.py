"""The launch plan of the fused bottleneck node (models/resnet_fused.py): which native op runs, on which shapes, in
which form and in which order, for one forward and backward of a three-block chain under FlatParams.

resnet_fused.lib and resnet_fused.gemm are swapped for forwarding recorders.  One log line per call:

    <op> [mode=<m>] [<shapes of the tensor arguments, positional first, then keyword ones by name>] <sorted names of
    the keyword arguments that were not None> [@side when the call was issued on another stream than the default one]

Everything is passed through untouched.  The expected logs at the end of this file were recorded with this very file
on the commit before the node was reshaped into plan + straight-line passes (1236782) and pasted in as printed: the
node has to issue exactly that work whatever its Python looks like.  To record again, run with -s and copy what each
case prints.
"""
import pytest
import torch

import dtg  # noqa: F401

pytestmark = pytest.mark.gpu

# (cin, width, stride) of the three blocks, input shape
CHAINS = {
    "a": (((64, 64, 1), (256, 64, 1), (256, 64, 1)), (2, 64, 56, 56)),     # stage 1, 6272 rows: every stage-1 form
    "b": (((256, 128, 2), (512, 128, 1), (512, 128, 1)), (2, 256, 64, 64)),  # stage 2, 2048 rows after the stride
    "c": (((64, 64, 1), (256, 64, 1), (256, 128, 2)), (4, 64, 16, 16)),    # 1024 rows: below every *_ok threshold
}
# chain, the switch that is off (None: the defaults; "broken_link": the gradient reaching block 2 is a clone).
# Only the switches that change the chain's log are listed: all nine were recorded on (a) and (b), and _FWD1_S2 on (a),
# _DXW2 and _DXD2 on (b) gave the log of the defaults.  (_DXD_S2 on (a) and _DXD on (b) change only which predicates
# are asked.)
CASES = [
    ("a", None), ("a", "_DXW"), ("a", "_DXW2"), ("a", "_DXD"), ("a", "_DXD2"), ("a", "_DXD_S2"), ("a", "_FWD1"),
    ("a", "_BITS"), ("a", "_LINK"), ("a", "broken_link"),
    ("b", None), ("b", "_DXW"), ("b", "_DXD"), ("b", "_DXD_S2"), ("b", "_FWD1"), ("b", "_FWD1_S2"), ("b", "_BITS"),
    ("b", "_LINK"),
    ("c", None), ("c", "_SUB2"), ("c", "_FUSE"),
]


def _entry(op, args, kw):
    tensors = list(args) + [kw[k] for k in sorted(kw)]
    s = op
    if op == "gemm_bn":
        s += " mode=%d" % (args[2] if len(args) > 2 else kw["mode"])
    s += " [" + " ".join("x".join(map(str, t.shape)) for t in tensors if isinstance(t, torch.Tensor)) + "]"
    names = sorted(k for k, v in kw.items() if v is not None)
    if names:
        s += " " + ",".join(names)
    if torch.cuda.current_stream() != torch.cuda.default_stream():
        s += " @side"
    return s


class _Recorder:
    """Forwards every attribute of the native module; calls are logged first."""

    def __init__(self, target, log):
        self._target, self._log = target, log

    def __getattr__(self, op):
        fn = getattr(self._target, op)
        if not callable(fn):
            return fn

        def call(*args, **kw):
            self._log.append(_entry(op, args, kw))
            return fn(*args, **kw)
        return call


def _ring_is_zero(like, real):
    """Every buffer of the pooled partial ring (csrc/bindings/ops.cc bn_part) at its full size."""
    return all((real.bn_part_alloc(like, 2048, pooled=True) == 0).all().item() for _ in range(16))


@pytest.mark.parametrize("chain_id,off", CASES, ids=["%s-%s" % (c, o or "default") for c, o in CASES])
def test_launch_plan_is_the_recorded_one(chain_id, off, monkeypatch):
    from dtg.models import resnet_fused
    from dtg.models.resnet import Bottleneck, chain_blocks
    from dtg.parallel import FlatParams, overlap
    dev = torch.device("cuda")
    blocks_cfg, xshape = CHAINS[chain_id]
    if off not in (None, "broken_link"):
        assert getattr(resnet_fused, off) is True
        monkeypatch.setattr(resnet_fused, off, False)
    monkeypatch.setattr(overlap, "_ON", True)            # weight gradients on the side stream, whatever the environment
    monkeypatch.setattr(resnet_fused, "_wsplit_cache", {})  # gemm_pick_split is asked once per shape: start cold
    monkeypatch.setattr(resnet_fused, "_dxd_calls", 0)
    monkeypatch.setattr(resnet_fused, "_fwd1_calls", 0)
    torch.manual_seed(0)
    chain = torch.nn.Module()
    chain.blocks = torch.nn.Sequential(*(Bottleneck(*cfg) for cfg in blocks_cfg))
    chain_blocks(chain.blocks)
    chain = chain.to(dev).to(memory_format=torch.channels_last)
    FlatParams(chain)
    chain.train()
    x = torch.randn(*xshape, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    x.requires_grad_()

    log = []
    real, real_gemm = resnet_fused.lib(), resnet_fused.gemm
    rec = _Recorder(real, log)

    def gemm(*args, **kw):
        log.append(_entry("gemm", args, kw))
        return real_gemm(*args, **kw)
    monkeypatch.setattr(resnet_fused, "lib", lambda: rec)
    monkeypatch.setattr(resnet_fused, "gemm", gemm)

    b1, b2, b3 = chain.blocks
    y1 = b1(x)
    y2 = b2(y1)
    if off == "broken_link":  # block 2 gets a copy of the gradient block 3 wrote: not the linked buffer
        y2.register_hook(lambda g: g.clone())
    y3 = b3(y2)
    log.append("-- backward")
    y3.backward(torch.ones_like(y3))
    torch.cuda.synchronize()
    counters = (resnet_fused._dxd_calls, resnet_fused._fwd1_calls)
    name = "%s-%s" % (chain_id, off or "default")
    print('    "%s": (%d, %d, """\n%s\n"""),' % (name, counters[0], counters[1], "\n".join(log)))
    assert torch.isfinite(x.grad.float()).all().item()
    del y1, y2, y3
    assert _ring_is_zero(x, real)  # every pooled slot went back zeroed, the dropped link's too

    assert name in EXPECTED, "no recorded plan for this case"
    dxd, fwd1, text = EXPECTED[name]
    want = text.strip("\n").split("\n")
    # The *_ok predicates run on the host and launch nothing.  The recorded node asked them where it happened to need
    # the answer; a node that decides first and executes afterwards asks them ahead of the work.  So: everything else
    # in the recorded order, and the same predicates asked the same number of times.
    work = lambda lines: [s for s in lines if not s.split(" ")[0].endswith("_ok")]  # noqa: E731
    asked = lambda lines: sorted(s for s in lines if s.split(" ")[0].endswith("_ok"))  # noqa: E731
    assert work(log) == work(want)
    assert asked(log) == asked(want)
    assert counters == (dxd, fwd1)


# (_dxd_calls, _fwd1_calls, log) per case
EXPECTED = {
    "a-default": (2, 2, """
gemm_bn mode=1 [6272x64 64x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd2_part [6272x256 16384 256 256 256 256 6272x256 16384 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32] bits
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [6272x256 6272x256 6272x256 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm_pick_split [] @side
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 6272x32 6272x256] mask,out,pooled
gemm_pick_split [] @side
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_part_alloc [6272x64] pooled
bn_bwd_part [6272x256 6272x256 16384 256 256 256 256 256 6272x8 64 64 4096 256x64 6272x64 6272x64 256x64] dgbits,dgfull,dginv,dgmean,dgpart,dgw,dgy,wact,wgrad
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
bn_part_alloc [6272x64] pooled
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 256 6272x32 256 6272x256 16384 6272x256] invstd2,mask,mean2,out,part2,pooled,x2
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_part_alloc [6272x64] pooled
bn_bwd2_part [6272x256 6272x256 16384 256 256 256 256 256 6272x256 16384 256 256 256 256 256 6272x8 64 64 4096 256x64 6272x64 6272x64 6272x64 256x64 256x64] dgbits,dgfull,dginv,dgmean,dgpart,dgw,dgy,wact,wact2,wgrad,wgrad2
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm [6272x256 256x64]
gemm [6272x64 64x64 6272x64] beta,out
gemm_pick_split [] @side
gemm [6272x64 6272x64 64x64] beta,out,split_k @side
"""),
    "a-_DXW": (0, 2, """
gemm_bn mode=1 [6272x64 64x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd2_part [6272x256 16384 256 256 256 256 6272x256 16384 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32] bits
-- backward
bn_bwd [6272x256 6272x256 6272x256 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm_pick_split [] @side
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 6272x32 6272x256] mask,out,pooled
gemm_pick_split [] @side
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_bwd_part [6272x256 6272x256 16384 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
bn_part_alloc [6272x64] pooled
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 256 6272x32 256 6272x256 16384 6272x256] invstd2,mask,mean2,out,part2,pooled,x2
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_bwd2_part [6272x256 6272x256 16384 256 256 256 256 256 6272x256 16384 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm [6272x256 256x64]
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
gemm [6272x64 64x64 6272x64] beta,out
gemm_pick_split [] @side
gemm [6272x64 6272x64 64x64] beta,out,split_k @side
"""),
    "a-_DXW2": (1, 2, """
gemm_bn mode=1 [6272x64 64x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd2_part [6272x256 16384 256 256 256 256 6272x256 16384 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32] bits
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [6272x256 6272x256 6272x256 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm_pick_split [] @side
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 6272x32 6272x256] mask,out,pooled
gemm_pick_split [] @side
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_part_alloc [6272x64] pooled
bn_bwd_part [6272x256 6272x256 16384 256 256 256 256 256 6272x8 64 64 4096 256x64 6272x64 6272x64 256x64] dgbits,dgfull,dginv,dgmean,dgpart,dgw,dgy,wact,wgrad
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
bn_part_alloc [6272x64] pooled
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 256 6272x32 256 6272x256 16384 6272x256] invstd2,mask,mean2,out,part2,pooled,x2
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd2_part [6272x256 6272x256 16384 256 256 256 256 256 6272x256 16384 256 256 256 256 256 6272x64 256x64] wact,wgrad
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm [6272x256 256x64]
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
gemm [6272x64 64x64 6272x64] beta,out
gemm_pick_split [] @side
gemm [6272x64 6272x64 64x64] beta,out,split_k @side
"""),
    "a-_DXD": (0, 2, """
gemm_bn mode=1 [6272x64 64x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd2_part [6272x256 16384 256 256 256 256 6272x256 16384 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32] bits
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [6272x256 6272x256 6272x256 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm_pick_split [] @side
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 6272x32 6272x256] mask,out,pooled
gemm_pick_split [] @side
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd_part [6272x256 6272x256 16384 256 256 256 256 256 6272x64 256x64] wact,wgrad
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
bn_part_alloc [6272x64] pooled
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 256 6272x32 256 6272x256 16384 6272x256] invstd2,mask,mean2,out,part2,pooled,x2
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd2_part [6272x256 6272x256 16384 256 256 256 256 256 6272x256 16384 256 256 256 256 256 6272x64 6272x64 256x64 256x64] wact,wact2,wgrad,wgrad2
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm [6272x256 256x64]
gemm [6272x64 64x64 6272x64] beta,out
gemm_pick_split [] @side
gemm [6272x64 6272x64 64x64] beta,out,split_k @side
"""),
    "a-_DXD2": (1, 2, """
gemm_bn mode=1 [6272x64 64x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd2_part [6272x256 16384 256 256 256 256 6272x256 16384 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32] bits
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [6272x256 6272x256 6272x256 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm_pick_split [] @side
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 6272x32 6272x256] mask,out,pooled
gemm_pick_split [] @side
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_part_alloc [6272x64] pooled
bn_bwd_part [6272x256 6272x256 16384 256 256 256 256 256 6272x8 64 64 4096 256x64 6272x64 6272x64 256x64] dgbits,dgfull,dginv,dgmean,dgpart,dgw,dgy,wact,wgrad
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
bn_part_alloc [6272x64] pooled
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 256 6272x32 256 6272x256 16384 6272x256] invstd2,mask,mean2,out,part2,pooled,x2
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd2_part [6272x256 6272x256 16384 256 256 256 256 256 6272x256 16384 256 256 256 256 256 6272x64 6272x64 256x64 256x64] wact,wact2,wgrad,wgrad2
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm [6272x256 256x64]
gemm [6272x64 64x64 6272x64] beta,out
gemm_pick_split [] @side
gemm [6272x64 6272x64 64x64] beta,out,split_k @side
"""),
    "a-_DXD_S2": (2, 2, """
gemm_bn mode=1 [6272x64 64x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd2_part [6272x256 16384 256 256 256 256 6272x256 16384 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32] bits
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_bwd [6272x256 6272x256 6272x256 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm_pick_split [] @side
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 6272x32 6272x256] mask,out,pooled
gemm_pick_split [] @side
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_part_alloc [6272x64] pooled
bn_bwd_part [6272x256 6272x256 16384 256 256 256 256 256 6272x8 64 64 4096 256x64 6272x64 6272x64 256x64] dgbits,dgfull,dginv,dgmean,dgpart,dgw,dgy,wact,wgrad
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
bn_part_alloc [6272x64] pooled
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 256 6272x32 256 6272x256 16384 6272x256] invstd2,mask,mean2,out,part2,pooled,x2
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_part_alloc [6272x64] pooled
bn_bwd2_part [6272x256 6272x256 16384 256 256 256 256 256 6272x256 16384 256 256 256 256 256 6272x8 64 64 4096 256x64 6272x64 6272x64 6272x64 256x64 256x64] dgbits,dgfull,dginv,dgmean,dgpart,dgw,dgy,wact,wact2,wgrad,wgrad2
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm [6272x256 256x64]
gemm [6272x64 64x64 6272x64] beta,out
gemm_pick_split [] @side
gemm [6272x64 6272x64 64x64] beta,out,split_k @side
"""),
    "a-_FWD1": (2, 0, """
gemm_bn mode=1 [6272x64 64x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
gemm_bn mode=1 [6272x64 256x64] pooled
bn_fwd2_part [6272x256 16384 256 256 256 256 6272x256 16384 256 256 256 256 6272x32] bits
gemm_bn mode=1 [6272x256 64x256] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32] bits
gemm_bn mode=1 [6272x256 64x256] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32] bits
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [6272x256 6272x256 6272x256 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm_pick_split [] @side
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 6272x32 6272x256] mask,out,pooled
gemm_pick_split [] @side
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_part_alloc [6272x64] pooled
bn_bwd_part [6272x256 6272x256 16384 256 256 256 256 256 6272x8 64 64 4096 256x64 6272x64 6272x64 256x64] dgbits,dgfull,dginv,dgmean,dgpart,dgw,dgy,wact,wgrad
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
bn_part_alloc [6272x64] pooled
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 256 6272x32 256 6272x256 16384 6272x256] invstd2,mask,mean2,out,part2,pooled,x2
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_part_alloc [6272x64] pooled
bn_bwd2_part [6272x256 6272x256 16384 256 256 256 256 256 6272x256 16384 256 256 256 256 256 6272x8 64 64 4096 256x64 6272x64 6272x64 6272x64 256x64 256x64] dgbits,dgfull,dginv,dgmean,dgpart,dgw,dgy,wact,wact2,wgrad,wgrad2
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm [6272x256 256x64]
gemm [6272x64 64x64 6272x64] beta,out
gemm_pick_split [] @side
gemm [6272x64 6272x64 64x64] beta,out,split_k @side
"""),
    "a-_BITS": (0, 2, """
gemm_bn mode=1 [6272x64 64x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64]
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64]
gemm_bn mode=1 [6272x64 256x64] pooled
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd2_part [6272x256 16384 256 256 256 256 6272x256 16384 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64]
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64]
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64]
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64]
gemm_bn mode=1 [6272x64 256x64] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32] bits
-- backward
bn_dx_wgrad_ok []
bn_bwd [6272x256 6272x256 6272x256 256 256 256 256 256]
gemm_bn mode=2 [6272x256 256x64 6272x64 64 64 64 64] pooled
gemm_pick_split [] @side
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64] pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 6272x32 6272x256] mask,out,pooled
gemm_pick_split [] @side
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_bwd_part [6272x256 6272x256 16384 256 256 256 256 256 6272x64 256x64] wact,wgrad
gemm_bn mode=2 [6272x256 256x64 6272x64 64 64 64 64] pooled
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64] pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
bn_part_alloc [6272x64] pooled
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 256 6272x32 256 6272x256 16384 6272x256] invstd2,mask,mean2,out,part2,pooled,x2
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_bwd2_part [6272x256 6272x256 16384 256 256 256 256 256 6272x256 16384 256 256 256 256 256 6272x64 6272x64 256x64 256x64] wact,wact2,wgrad,wgrad2
gemm_bn mode=2 [6272x256 256x64 6272x64 64 64 64 64] pooled
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64] pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm [6272x256 256x64]
gemm [6272x64 64x64 6272x64] beta,out
gemm_pick_split [] @side
gemm [6272x64 6272x64 64x64] beta,out,split_k @side
"""),
    "a-_LINK": (0, 2, """
gemm_bn mode=1 [6272x64 64x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd2_part [6272x256 16384 256 256 256 256 6272x256 16384 256 256 256 256 4096 64x256] next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 4096 64x256] next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256]
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [6272x256 6272x256 6272x256 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm_pick_split [] @side
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm [6272x64 64x256 6272x256] beta,out
gemm_pick_split [] @side
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [6272x256 6272x256 6272x256 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm [6272x64 64x256 6272x256] beta,out
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [6272x256 6272x256 6272x256 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
bn_bwd [6272x256 6272x256 256 256 256 256 256]
gemm [6272x256 256x64]
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
gemm [6272x64 64x64 6272x64] beta,out
gemm_pick_split [] @side
gemm [6272x64 6272x64 64x64] beta,out,split_k @side
"""),
    "a-broken_link": (1, 2, """
gemm_bn mode=1 [6272x64 64x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd2_part [6272x256 16384 256 256 256 256 6272x256 16384 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_apply_gemm_ok []
bn_part_alloc [6272x256] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32 4096 64x256] bits,next_part,next_w
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
conv_fwd_bn [2x56x56x64 64x3x3x64] pooled
bn_fwd_part [6272x64 4096 64 64 64 64 6272x8] bits
gemm_bn mode=1 [6272x64 256x64] pooled
bn_fwd_part [6272x256 16384 6272x256 256 256 256 256 6272x32] bits
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [6272x256 6272x256 6272x256 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm_pick_split [] @side
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 6272x32 6272x256] mask,out,pooled
gemm_pick_split [] @side
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [6272x256 6272x256 6272x256 256 256 256 256 256]
gemm_bn mode=3 [6272x256 256x64 6272x64 64 64 64 64 6272x8] mask,pooled
gemm [6272x256 6272x64 256x64] beta,out,split_k @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
bn_part_alloc [6272x64] pooled
gemm_bn mode=3 [6272x64 64x256 6272x256 256 256 256 256 256 6272x32 256 6272x256 16384 6272x256] invstd2,mask,mean2,out,part2,pooled,x2
gemm [6272x64 6272x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_part_alloc [6272x64] pooled
bn_bwd2_part [6272x256 6272x256 16384 256 256 256 256 256 6272x256 16384 256 256 256 256 256 6272x8 64 64 4096 256x64 6272x64 6272x64 6272x64 256x64 256x64] dgbits,dgfull,dginv,dgmean,dgpart,dgw,dgy,wact,wact2,wgrad,wgrad2
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
conv_dgrad_bn [2x56x56x64 64x3x3x64 6272x64 64 64 64 64 6272x8] bits,pooled
conv_wgrad [2x56x56x64 2x56x56x64 64x3x3x64] target_wgs @side
bn_bwd_part [6272x64 6272x64 4096 64 64 64 64 64]
gemm [6272x256 256x64]
gemm [6272x64 64x64 6272x64] beta,out
gemm_pick_split [] @side
gemm [6272x64 6272x64 64x64] beta,out,split_k @side
"""),
    "b-default": (1, 2, """
gemm_bn mode=1 [8192x256 128x256] pooled
bn_fwd_part [8192x128 8192 128 128 128 128 8192x16] bits
conv_fwd_bn [2x64x64x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
conv_fwd_bn [2x64x64x256 512x1x1x256] pooled
bn_apply_gemm_ok []
bn_part_alloc [2048x512] pooled
bn_fwd2_part [2048x512 32768 512 512 512 512 2048x512 32768 512 512 512 512 2048x64 8192 128x512] bits,next_part,next_w
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_apply_gemm_ok []
bn_part_alloc [2048x512] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64 8192 128x512] bits,next_part,next_w
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64] bits
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [2048x512 2048x512 2048x512 512 512 512 512 512]
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
gemm_pick_split [] @side
gemm [2048x512 2048x128 512x128] beta,out,split_k @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 2048x64 2048x512] mask,out,pooled
gemm_pick_split [] @side
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_part_alloc [2048x128] pooled
bn_bwd_part [2048x512 2048x512 32768 512 512 512 512 512 2048x16 128 128 8192 512x128 2048x128 2048x128 512x128] dgbits,dgfull,dginv,dgmean,dgpart,dgw,dgy,wact,wgrad
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
bn_part_alloc [2048x128] pooled
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 512 2048x64 512 2048x512 32768 2048x512] invstd2,mask,mean2,out,part2,pooled,x2
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd2_part [2048x512 2048x512 32768 512 512 512 512 512 2048x512 32768 512 512 512 512 512 2048x128 512x128] wact,wgrad
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 8192x128 128 128 128 128 8192x16] bits,pooled
conv_wgrad [2x32x32x128 2x64x64x128 128x3x3x128] target_wgs @side
bn_bwd_part [8192x128 8192x128 8192 128 128 128 128 128]
gemm [8192x128 128x256]
conv_dgrad [2x32x32x512 512x1x1x256 2x64x64x256] beta,out
conv_wgrad [2x32x32x512 2x64x64x256 512x1x1x256] target_wgs @side
gemm_pick_split [] @side
gemm [8192x128 8192x256 128x256] beta,out,split_k @side
"""),
    "b-_DXW": (0, 2, """
gemm_bn mode=1 [8192x256 128x256] pooled
bn_fwd_part [8192x128 8192 128 128 128 128 8192x16] bits
conv_fwd_bn [2x64x64x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
conv_fwd_bn [2x64x64x256 512x1x1x256] pooled
bn_apply_gemm_ok []
bn_part_alloc [2048x512] pooled
bn_fwd2_part [2048x512 32768 512 512 512 512 2048x512 32768 512 512 512 512 2048x64 8192 128x512] bits,next_part,next_w
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_apply_gemm_ok []
bn_part_alloc [2048x512] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64 8192 128x512] bits,next_part,next_w
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64] bits
-- backward
bn_bwd [2048x512 2048x512 2048x512 512 512 512 512 512]
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
gemm_pick_split [] @side
gemm [2048x512 2048x128 512x128] beta,out,split_k @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 2048x64 2048x512] mask,out,pooled
gemm_pick_split [] @side
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_bwd_part [2048x512 2048x512 32768 512 512 512 512 512]
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
gemm [2048x512 2048x128 512x128] beta,out,split_k @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
bn_part_alloc [2048x128] pooled
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 512 2048x64 512 2048x512 32768 2048x512] invstd2,mask,mean2,out,part2,pooled,x2
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_bwd2_part [2048x512 2048x512 32768 512 512 512 512 512 2048x512 32768 512 512 512 512 512]
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
gemm [2048x512 2048x128 512x128] beta,out,split_k @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 8192x128 128 128 128 128 8192x16] bits,pooled
conv_wgrad [2x32x32x128 2x64x64x128 128x3x3x128] target_wgs @side
bn_bwd_part [8192x128 8192x128 8192 128 128 128 128 128]
gemm [8192x128 128x256]
conv_dgrad [2x32x32x512 512x1x1x256 2x64x64x256] beta,out
conv_wgrad [2x32x32x512 2x64x64x256 512x1x1x256] target_wgs @side
gemm_pick_split [] @side
gemm [8192x128 8192x256 128x256] beta,out,split_k @side
"""),
    "b-_DXD": (1, 2, """
gemm_bn mode=1 [8192x256 128x256] pooled
bn_fwd_part [8192x128 8192 128 128 128 128 8192x16] bits
conv_fwd_bn [2x64x64x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
conv_fwd_bn [2x64x64x256 512x1x1x256] pooled
bn_apply_gemm_ok []
bn_part_alloc [2048x512] pooled
bn_fwd2_part [2048x512 32768 512 512 512 512 2048x512 32768 512 512 512 512 2048x64 8192 128x512] bits,next_part,next_w
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_apply_gemm_ok []
bn_part_alloc [2048x512] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64 8192 128x512] bits,next_part,next_w
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64] bits
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [2048x512 2048x512 2048x512 512 512 512 512 512]
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
gemm_pick_split [] @side
gemm [2048x512 2048x128 512x128] beta,out,split_k @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 2048x64 2048x512] mask,out,pooled
gemm_pick_split [] @side
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_full_ok []
bn_part_alloc [2048x128] pooled
bn_bwd_part [2048x512 2048x512 32768 512 512 512 512 512 2048x16 128 128 8192 512x128 2048x128 2048x128 512x128] dgbits,dgfull,dginv,dgmean,dgpart,dgw,dgy,wact,wgrad
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
bn_part_alloc [2048x128] pooled
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 512 2048x64 512 2048x512 32768 2048x512] invstd2,mask,mean2,out,part2,pooled,x2
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd2_part [2048x512 2048x512 32768 512 512 512 512 512 2048x512 32768 512 512 512 512 512 2048x128 512x128] wact,wgrad
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 8192x128 128 128 128 128 8192x16] bits,pooled
conv_wgrad [2x32x32x128 2x64x64x128 128x3x3x128] target_wgs @side
bn_bwd_part [8192x128 8192x128 8192 128 128 128 128 128]
gemm [8192x128 128x256]
conv_dgrad [2x32x32x512 512x1x1x256 2x64x64x256] beta,out
conv_wgrad [2x32x32x512 2x64x64x256 512x1x1x256] target_wgs @side
gemm_pick_split [] @side
gemm [8192x128 8192x256 128x256] beta,out,split_k @side
"""),
    "b-_DXD_S2": (0, 2, """
gemm_bn mode=1 [8192x256 128x256] pooled
bn_fwd_part [8192x128 8192 128 128 128 128 8192x16] bits
conv_fwd_bn [2x64x64x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
conv_fwd_bn [2x64x64x256 512x1x1x256] pooled
bn_apply_gemm_ok []
bn_part_alloc [2048x512] pooled
bn_fwd2_part [2048x512 32768 512 512 512 512 2048x512 32768 512 512 512 512 2048x64 8192 128x512] bits,next_part,next_w
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_apply_gemm_ok []
bn_part_alloc [2048x512] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64 8192 128x512] bits,next_part,next_w
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64] bits
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_bwd [2048x512 2048x512 2048x512 512 512 512 512 512]
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
gemm_pick_split [] @side
gemm [2048x512 2048x128 512x128] beta,out,split_k @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 2048x64 2048x512] mask,out,pooled
gemm_pick_split [] @side
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_bwd_part [2048x512 2048x512 32768 512 512 512 512 512 2048x128 512x128] wact,wgrad
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
bn_part_alloc [2048x128] pooled
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 512 2048x64 512 2048x512 32768 2048x512] invstd2,mask,mean2,out,part2,pooled,x2
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_bwd2_part [2048x512 2048x512 32768 512 512 512 512 512 2048x512 32768 512 512 512 512 512 2048x128 512x128] wact,wgrad
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 8192x128 128 128 128 128 8192x16] bits,pooled
conv_wgrad [2x32x32x128 2x64x64x128 128x3x3x128] target_wgs @side
bn_bwd_part [8192x128 8192x128 8192 128 128 128 128 128]
gemm [8192x128 128x256]
conv_dgrad [2x32x32x512 512x1x1x256 2x64x64x256] beta,out
conv_wgrad [2x32x32x512 2x64x64x256 512x1x1x256] target_wgs @side
gemm_pick_split [] @side
gemm [8192x128 8192x256 128x256] beta,out,split_k @side
"""),
    "b-_FWD1": (1, 0, """
gemm_bn mode=1 [8192x256 128x256] pooled
bn_fwd_part [8192x128 8192 128 128 128 128 8192x16] bits
conv_fwd_bn [2x64x64x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
conv_fwd_bn [2x64x64x256 512x1x1x256] pooled
bn_fwd2_part [2048x512 32768 512 512 512 512 2048x512 32768 512 512 512 512 2048x64] bits
gemm_bn mode=1 [2048x512 128x512] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64] bits
gemm_bn mode=1 [2048x512 128x512] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64] bits
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [2048x512 2048x512 2048x512 512 512 512 512 512]
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
gemm_pick_split [] @side
gemm [2048x512 2048x128 512x128] beta,out,split_k @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 2048x64 2048x512] mask,out,pooled
gemm_pick_split [] @side
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_part_alloc [2048x128] pooled
bn_bwd_part [2048x512 2048x512 32768 512 512 512 512 512 2048x16 128 128 8192 512x128 2048x128 2048x128 512x128] dgbits,dgfull,dginv,dgmean,dgpart,dgw,dgy,wact,wgrad
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
bn_part_alloc [2048x128] pooled
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 512 2048x64 512 2048x512 32768 2048x512] invstd2,mask,mean2,out,part2,pooled,x2
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd2_part [2048x512 2048x512 32768 512 512 512 512 512 2048x512 32768 512 512 512 512 512 2048x128 512x128] wact,wgrad
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 8192x128 128 128 128 128 8192x16] bits,pooled
conv_wgrad [2x32x32x128 2x64x64x128 128x3x3x128] target_wgs @side
bn_bwd_part [8192x128 8192x128 8192 128 128 128 128 128]
gemm [8192x128 128x256]
conv_dgrad [2x32x32x512 512x1x1x256 2x64x64x256] beta,out
conv_wgrad [2x32x32x512 2x64x64x256 512x1x1x256] target_wgs @side
gemm_pick_split [] @side
gemm [8192x128 8192x256 128x256] beta,out,split_k @side
"""),
    "b-_FWD1_S2": (1, 0, """
gemm_bn mode=1 [8192x256 128x256] pooled
bn_fwd_part [8192x128 8192 128 128 128 128 8192x16] bits
conv_fwd_bn [2x64x64x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
conv_fwd_bn [2x64x64x256 512x1x1x256] pooled
bn_apply_gemm_ok []
bn_fwd2_part [2048x512 32768 512 512 512 512 2048x512 32768 512 512 512 512 2048x64] bits
gemm_bn mode=1 [2048x512 128x512] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_apply_gemm_ok []
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64] bits
gemm_bn mode=1 [2048x512 128x512] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64] bits
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [2048x512 2048x512 2048x512 512 512 512 512 512]
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
gemm_pick_split [] @side
gemm [2048x512 2048x128 512x128] beta,out,split_k @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 2048x64 2048x512] mask,out,pooled
gemm_pick_split [] @side
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_part_alloc [2048x128] pooled
bn_bwd_part [2048x512 2048x512 32768 512 512 512 512 512 2048x16 128 128 8192 512x128 2048x128 2048x128 512x128] dgbits,dgfull,dginv,dgmean,dgpart,dgw,dgy,wact,wgrad
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
bn_part_alloc [2048x128] pooled
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 512 2048x64 512 2048x512 32768 2048x512] invstd2,mask,mean2,out,part2,pooled,x2
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd2_part [2048x512 2048x512 32768 512 512 512 512 512 2048x512 32768 512 512 512 512 512 2048x128 512x128] wact,wgrad
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 8192x128 128 128 128 128 8192x16] bits,pooled
conv_wgrad [2x32x32x128 2x64x64x128 128x3x3x128] target_wgs @side
bn_bwd_part [8192x128 8192x128 8192 128 128 128 128 128]
gemm [8192x128 128x256]
conv_dgrad [2x32x32x512 512x1x1x256 2x64x64x256] beta,out
conv_wgrad [2x32x32x512 2x64x64x256 512x1x1x256] target_wgs @side
gemm_pick_split [] @side
gemm [8192x128 8192x256 128x256] beta,out,split_k @side
"""),
    "b-_BITS": (0, 2, """
gemm_bn mode=1 [8192x256 128x256] pooled
bn_fwd_part [8192x128 8192 128 128 128 128]
conv_fwd_bn [2x64x64x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128]
gemm_bn mode=1 [2048x128 512x128] pooled
conv_fwd_bn [2x64x64x256 512x1x1x256] pooled
bn_apply_gemm_ok []
bn_part_alloc [2048x512] pooled
bn_fwd2_part [2048x512 32768 512 512 512 512 2048x512 32768 512 512 512 512 2048x64 8192 128x512] bits,next_part,next_w
bn_fwd_part [2048x128 8192 128 128 128 128]
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128]
gemm_bn mode=1 [2048x128 512x128] pooled
bn_apply_gemm_ok []
bn_part_alloc [2048x512] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64 8192 128x512] bits,next_part,next_w
bn_fwd_part [2048x128 8192 128 128 128 128]
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128]
gemm_bn mode=1 [2048x128 512x128] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 2048x64] bits
-- backward
bn_dx_wgrad_ok []
bn_bwd [2048x512 2048x512 2048x512 512 512 512 512 512]
gemm_bn mode=2 [2048x512 512x128 2048x128 128 128 128 128] pooled
gemm_pick_split [] @side
gemm [2048x512 2048x128 512x128] beta,out,split_k @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128] pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 2048x64 2048x512] mask,out,pooled
gemm_pick_split [] @side
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_bwd_part [2048x512 2048x512 32768 512 512 512 512 512 2048x128 512x128] wact,wgrad
gemm_bn mode=2 [2048x512 512x128 2048x128 128 128 128 128] pooled
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128] pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
bn_part_alloc [2048x128] pooled
gemm_bn mode=3 [2048x128 128x512 2048x512 512 512 512 512 512 2048x64 512 2048x512 32768 2048x512] invstd2,mask,mean2,out,part2,pooled,x2
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_bwd2_part [2048x512 2048x512 32768 512 512 512 512 512 2048x512 32768 512 512 512 512 512 2048x128 512x128] wact,wgrad
gemm_bn mode=2 [2048x512 512x128 2048x128 128 128 128 128] pooled
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 8192x128 128 128 128 128] pooled
conv_wgrad [2x32x32x128 2x64x64x128 128x3x3x128] target_wgs @side
bn_bwd_part [8192x128 8192x128 8192 128 128 128 128 128]
gemm [8192x128 128x256]
conv_dgrad [2x32x32x512 512x1x1x256 2x64x64x256] beta,out
conv_wgrad [2x32x32x512 2x64x64x256 512x1x1x256] target_wgs @side
gemm_pick_split [] @side
gemm [8192x128 8192x256 128x256] beta,out,split_k @side
"""),
    "b-_LINK": (0, 2, """
gemm_bn mode=1 [8192x256 128x256] pooled
bn_fwd_part [8192x128 8192 128 128 128 128 8192x16] bits
conv_fwd_bn [2x64x64x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
conv_fwd_bn [2x64x64x256 512x1x1x256] pooled
bn_apply_gemm_ok []
bn_part_alloc [2048x512] pooled
bn_fwd2_part [2048x512 32768 512 512 512 512 2048x512 32768 512 512 512 512 8192 128x512] next_part,next_w
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_apply_gemm_ok []
bn_part_alloc [2048x512] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512 8192 128x512] next_part,next_w
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
conv_fwd_bn [2x32x32x128 128x3x3x128] pooled
bn_fwd_part [2048x128 8192 128 128 128 128 2048x16] bits
gemm_bn mode=1 [2048x128 512x128] pooled
bn_fwd_part [2048x512 32768 2048x512 512 512 512 512]
-- backward
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [2048x512 2048x512 2048x512 512 512 512 512 512]
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
gemm_pick_split [] @side
gemm [2048x512 2048x128 512x128] beta,out,split_k @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
gemm [2048x128 128x512 2048x512] beta,out
gemm_pick_split [] @side
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [2048x512 2048x512 2048x512 512 512 512 512 512]
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
gemm [2048x512 2048x128 512x128] beta,out,split_k @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 2048x128 128 128 128 128 2048x16] bits,pooled
conv_wgrad [2x32x32x128 2x32x32x128 128x3x3x128] target_wgs @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
gemm [2048x128 128x512 2048x512] beta,out
gemm [2048x128 2048x512 128x512] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_dx_dgrad_ok []
bn_dx_dgrad_full_ok []
bn_bwd [2048x512 2048x512 2048x512 512 512 512 512 512]
gemm_bn mode=3 [2048x512 512x128 2048x128 128 128 128 128 2048x16] mask,pooled
gemm [2048x512 2048x128 512x128] beta,out,split_k @side
bn_bwd_part [2048x128 2048x128 8192 128 128 128 128 128]
conv_dgrad_bn [2x32x32x128 128x3x3x128 8192x128 128 128 128 128 8192x16] bits,pooled
conv_wgrad [2x32x32x128 2x64x64x128 128x3x3x128] target_wgs @side
bn_bwd_part [8192x128 8192x128 8192 128 128 128 128 128]
bn_bwd [2048x512 2048x512 512 512 512 512 512]
gemm [8192x128 128x256]
conv_dgrad [2x32x32x512 512x1x1x256 2x64x64x256] beta,out
conv_wgrad [2x32x32x512 2x64x64x256 512x1x1x256] target_wgs @side
gemm_pick_split [] @side
gemm [8192x128 8192x256 128x256] beta,out,split_k @side
"""),
    "c-default": (0, 0, """
gemm_bn mode=1 [1024x64 64x64] pooled
bn_fwd_part [1024x64 4096 64 64 64 64 1024x8] bits
conv_fwd_bn [4x16x16x64 64x3x3x64] pooled
bn_fwd_part [1024x64 4096 64 64 64 64 1024x8] bits
gemm_bn mode=1 [1024x64 256x64] pooled
gemm_bn mode=1 [1024x64 256x64] pooled
bn_apply_gemm_ok []
bn_fwd2_part [1024x256 16384 256 256 256 256 1024x256 16384 256 256 256 256 1024x32] bits
gemm_bn mode=1 [1024x256 64x256] pooled
bn_fwd_part [1024x64 4096 64 64 64 64 1024x8] bits
conv_fwd_bn [4x16x16x64 64x3x3x64] pooled
bn_fwd_part [1024x64 4096 64 64 64 64 1024x8] bits
gemm_bn mode=1 [1024x64 256x64] pooled
bn_apply_gemm_ok []
bn_fwd_part [1024x256 16384 1024x256 256 256 256 256 1024x32] bits
gemm_bn mode=1 [1024x256 128x256] pooled
bn_fwd_part [1024x128 8192 128 128 128 128 1024x16] bits
conv_fwd_bn [4x16x16x128 128x3x3x128] pooled
bn_fwd_part [256x128 8192 128 128 128 128 256x16] bits
gemm_bn mode=1 [256x128 512x128] pooled
conv_fwd_bn [4x16x16x256 512x1x1x256] pooled
bn_fwd2_part [256x512 32768 512 512 512 512 256x512 32768 512 512 512 512 256x64] bits
-- backward
bn_dx_wgrad_ok []
bn_bwd [256x512 256x512 256x512 512 512 512 512 512]
gemm_bn mode=3 [256x512 512x128 256x128 128 128 128 128 256x16] mask,pooled
gemm_pick_split [] @side
gemm [256x512 256x128 512x128] beta,out,split_k @side
bn_bwd_part [256x128 256x128 8192 128 128 128 128 128]
conv_dgrad_bn [4x8x8x128 128x3x3x128 1024x128 128 128 128 128 1024x16] bits,pooled
conv_wgrad [4x8x8x128 4x16x16x128 128x3x3x128] target_wgs @side
bn_bwd_part [1024x128 1024x128 8192 128 128 128 128 128]
bn_bwd [256x512 256x512 512 512 512 512 512]
conv_dgrad [4x8x8x512 512x1x1x256] zero_rest
conv_wgrad [4x8x8x512 4x16x16x256 512x1x1x256] target_wgs @side
gemm_bn mode=3 [1024x128 128x256 1024x256 256 256 256 256 1024x32 1024x256] mask,out,pooled,sub2_hw
gemm_pick_split [] @side
gemm [1024x128 1024x256 128x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_bwd_part [1024x256 1024x256 16384 256 256 256 256 256]
gemm_bn mode=3 [1024x256 256x64 1024x64 64 64 64 64 1024x8] mask,pooled
gemm_pick_split [] @side
gemm [1024x256 1024x64 256x64] beta,out,split_k @side
bn_bwd_part [1024x64 1024x64 4096 64 64 64 64 64]
conv_dgrad_bn [4x16x16x64 64x3x3x64 1024x64 64 64 64 64 1024x8] bits,pooled
conv_wgrad [4x16x16x64 4x16x16x64 64x3x3x64] target_wgs @side
bn_bwd_part [1024x64 1024x64 4096 64 64 64 64 64]
bn_part_alloc [1024x64] pooled
gemm_bn mode=3 [1024x64 64x256 1024x256 256 256 256 256 256 1024x32 256 1024x256 16384 1024x256] invstd2,mask,mean2,out,part2,pooled,x2
gemm_pick_split [] @side
gemm [1024x64 1024x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_bwd2_part [1024x256 1024x256 16384 256 256 256 256 256 1024x256 16384 256 256 256 256 256]
gemm_bn mode=3 [1024x256 256x64 1024x64 64 64 64 64 1024x8] mask,pooled
gemm [1024x256 1024x64 256x64] beta,out,split_k @side
bn_bwd_part [1024x64 1024x64 4096 64 64 64 64 64]
conv_dgrad_bn [4x16x16x64 64x3x3x64 1024x64 64 64 64 64 1024x8] bits,pooled
conv_wgrad [4x16x16x64 4x16x16x64 64x3x3x64] target_wgs @side
bn_bwd_part [1024x64 1024x64 4096 64 64 64 64 64]
gemm [1024x256 256x64]
gemm [1024x256 1024x64 256x64] beta,out,split_k @side
gemm [1024x64 64x64 1024x64] beta,out
gemm_pick_split [] @side
gemm [1024x64 1024x64 64x64] beta,out,split_k @side
"""),
    "c-_SUB2": (0, 0, """
gemm_bn mode=1 [1024x64 64x64] pooled
bn_fwd_part [1024x64 4096 64 64 64 64 1024x8] bits
conv_fwd_bn [4x16x16x64 64x3x3x64] pooled
bn_fwd_part [1024x64 4096 64 64 64 64 1024x8] bits
gemm_bn mode=1 [1024x64 256x64] pooled
gemm_bn mode=1 [1024x64 256x64] pooled
bn_apply_gemm_ok []
bn_fwd2_part [1024x256 16384 256 256 256 256 1024x256 16384 256 256 256 256 1024x32] bits
gemm_bn mode=1 [1024x256 64x256] pooled
bn_fwd_part [1024x64 4096 64 64 64 64 1024x8] bits
conv_fwd_bn [4x16x16x64 64x3x3x64] pooled
bn_fwd_part [1024x64 4096 64 64 64 64 1024x8] bits
gemm_bn mode=1 [1024x64 256x64] pooled
bn_apply_gemm_ok []
bn_fwd_part [1024x256 16384 1024x256 256 256 256 256 1024x32] bits
gemm_bn mode=1 [1024x256 128x256] pooled
bn_fwd_part [1024x128 8192 128 128 128 128 1024x16] bits
conv_fwd_bn [4x16x16x128 128x3x3x128] pooled
bn_fwd_part [256x128 8192 128 128 128 128 256x16] bits
gemm_bn mode=1 [256x128 512x128] pooled
conv_fwd_bn [4x16x16x256 512x1x1x256] pooled
bn_fwd2_part [256x512 32768 512 512 512 512 256x512 32768 512 512 512 512 256x64] bits
-- backward
bn_dx_wgrad_ok []
bn_bwd [256x512 256x512 256x512 512 512 512 512 512]
gemm_bn mode=3 [256x512 512x128 256x128 128 128 128 128 256x16] mask,pooled
gemm_pick_split [] @side
gemm [256x512 256x128 512x128] beta,out,split_k @side
bn_bwd_part [256x128 256x128 8192 128 128 128 128 128]
conv_dgrad_bn [4x8x8x128 128x3x3x128 1024x128 128 128 128 128 1024x16] bits,pooled
conv_wgrad [4x8x8x128 4x16x16x128 128x3x3x128] target_wgs @side
bn_bwd_part [1024x128 1024x128 8192 128 128 128 128 128]
bn_bwd [256x512 256x512 512 512 512 512 512]
conv_dgrad [4x8x8x512 512x1x1x256] zero_rest
conv_wgrad [4x8x8x512 4x16x16x256 512x1x1x256] target_wgs @side
gemm_bn mode=3 [1024x128 128x256 1024x256 256 256 256 256 1024x32 1024x256] mask,out,pooled
gemm_pick_split [] @side
gemm [1024x128 1024x256 128x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_bwd_part [1024x256 1024x256 16384 256 256 256 256 256]
gemm_bn mode=3 [1024x256 256x64 1024x64 64 64 64 64 1024x8] mask,pooled
gemm_pick_split [] @side
gemm [1024x256 1024x64 256x64] beta,out,split_k @side
bn_bwd_part [1024x64 1024x64 4096 64 64 64 64 64]
conv_dgrad_bn [4x16x16x64 64x3x3x64 1024x64 64 64 64 64 1024x8] bits,pooled
conv_wgrad [4x16x16x64 4x16x16x64 64x3x3x64] target_wgs @side
bn_bwd_part [1024x64 1024x64 4096 64 64 64 64 64]
bn_part_alloc [1024x64] pooled
gemm_bn mode=3 [1024x64 64x256 1024x256 256 256 256 256 256 1024x32 256 1024x256 16384 1024x256] invstd2,mask,mean2,out,part2,pooled,x2
gemm_pick_split [] @side
gemm [1024x64 1024x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_bwd2_part [1024x256 1024x256 16384 256 256 256 256 256 1024x256 16384 256 256 256 256 256]
gemm_bn mode=3 [1024x256 256x64 1024x64 64 64 64 64 1024x8] mask,pooled
gemm [1024x256 1024x64 256x64] beta,out,split_k @side
bn_bwd_part [1024x64 1024x64 4096 64 64 64 64 64]
conv_dgrad_bn [4x16x16x64 64x3x3x64 1024x64 64 64 64 64 1024x8] bits,pooled
conv_wgrad [4x16x16x64 4x16x16x64 64x3x3x64] target_wgs @side
bn_bwd_part [1024x64 1024x64 4096 64 64 64 64 64]
gemm [1024x256 256x64]
gemm [1024x256 1024x64 256x64] beta,out,split_k @side
gemm [1024x64 64x64 1024x64] beta,out
gemm_pick_split [] @side
gemm [1024x64 1024x64 64x64] beta,out,split_k @side
"""),
    "c-_FUSE": (0, 0, """
gemm [1024x64 64x64]
bn_fwd_train [1024x64 64 64 64 64]
conv_fwd [4x16x16x64 64x3x3x64]
bn_fwd_train [1024x64 64 64 64 64]
gemm [1024x64 256x64]
gemm [1024x64 256x64]
bn_fwd_train [1024x256 256 256 256 256]
bn_fwd_train [1024x256 1024x256 256 256 256 256]
gemm [1024x256 64x256]
bn_fwd_train [1024x64 64 64 64 64]
conv_fwd [4x16x16x64 64x3x3x64]
bn_fwd_train [1024x64 64 64 64 64]
gemm [1024x64 256x64]
bn_fwd_train [1024x256 1024x256 256 256 256 256]
gemm [1024x256 128x256]
bn_fwd_train [1024x128 128 128 128 128]
conv_fwd [4x16x16x128 128x3x3x128]
bn_fwd_train [256x128 128 128 128 128]
gemm [256x128 512x128]
conv_fwd [4x16x16x256 512x1x1x256]
bn_fwd_train [256x512 512 512 512 512]
bn_fwd_train [256x512 256x512 512 512 512 512]
-- backward
bn_dx_wgrad_ok []
bn_bwd [256x512 256x512 256x512 512 512 512 512 512]
gemm [256x512 512x128]
gemm_pick_split [] @side
gemm [256x512 256x128 512x128] beta,out,split_k @side
bn_bwd [256x128 256x128 256x128 128 128 128 128 128]
conv_dgrad [4x8x8x128 128x3x3x128]
conv_wgrad [4x8x8x128 4x16x16x128 128x3x3x128] target_wgs @side
bn_bwd [1024x128 1024x128 1024x128 128 128 128 128 128]
bn_bwd [256x512 256x512 512 512 512 512 512]
gemm [1024x128 128x256]
conv_dgrad [4x8x8x512 512x1x1x256 4x16x16x256] beta,out
conv_wgrad [4x8x8x512 4x16x16x256 512x1x1x256] target_wgs @side
gemm_pick_split [] @side
gemm [1024x128 1024x256 128x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_bwd [1024x256 1024x256 1024x256 256 256 256 256 256]
gemm [1024x256 256x64]
gemm_pick_split [] @side
gemm [1024x256 1024x64 256x64] beta,out,split_k @side
bn_bwd [1024x64 1024x64 1024x64 64 64 64 64 64]
conv_dgrad [4x16x16x64 64x3x3x64]
conv_wgrad [4x16x16x64 4x16x16x64 64x3x3x64] target_wgs @side
bn_bwd [1024x64 1024x64 1024x64 64 64 64 64 64]
gemm [1024x64 64x256 1024x256] beta,out
gemm_pick_split [] @side
gemm [1024x64 1024x256 64x256] beta,out,split_k @side
bn_dx_wgrad_ok []
bn_bwd [1024x256 1024x256 1024x256 256 256 256 256 256]
gemm [1024x256 256x64]
gemm [1024x256 1024x64 256x64] beta,out,split_k @side
bn_bwd [1024x64 1024x64 1024x64 64 64 64 64 64]
conv_dgrad [4x16x16x64 64x3x3x64]
conv_wgrad [4x16x16x64 4x16x16x64 64x3x3x64] target_wgs @side
bn_bwd [1024x64 1024x64 1024x64 64 64 64 64 64]
bn_bwd [1024x256 1024x256 256 256 256 256 256]
gemm [1024x256 256x64]
gemm [1024x256 1024x64 256x64] beta,out,split_k @side
gemm [1024x64 64x64 1024x64] beta,out
gemm_pick_split [] @side
gemm [1024x64 1024x64 64x64] beta,out,split_k @side
"""),
}
