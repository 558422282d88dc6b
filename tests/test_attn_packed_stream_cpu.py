"""The streaming packed attention entry points of ops/seqpack.py on CPU tensors: they reach the mirror
(attn_packed_ref) and autograd through it, like the other packed pairs.  Set A of test_attn_packed_stream_gpu.py
(S = 640), nh = 1, fp32."""
import torch

import dtg  # noqa: F401
from dtg.ops import seqpack

S, NH, LENS = 640, 1, [640, 1, 513, 65, 0, 577, 127, 600]
B, H = len(LENS), NH * 64


def test_cpu_tensors_reach_the_mirror():
    cu = seqpack.seq_offsets(torch.tensor(LENS, dtype=torch.int32), S)
    T = int(cu[B])
    Ta = -(-T // 64) * 64
    assert (T, Ta) == (2523, 2560)
    g = torch.Generator().manual_seed(3)
    qkv, dout = torch.randn(Ta, 3 * H, generator=g), torch.randn(Ta, H, generator=g)
    for p in (0.0, 0.1):
        ctx, lse = seqpack.attn_packed_stream_fwd(qkv, cu, B, S, NH, p, 9)
        x = qkv.clone().requires_grad_()
        want = seqpack.attn_packed_ref(x, cu, B, S, NH, p, 9)
        assert lse is None and torch.equal(ctx, want.detach()) and not ctx[T:].any()
        (gx,) = torch.autograd.grad(want, x, dout)
        db = torch.full((3 * H,), 0.5)
        dqkv = seqpack.attn_packed_stream_bwd(qkv, ctx, dout, None, cu, B, S, NH, p, 9, dbias=db)
        assert torch.equal(dqkv, gx) and not dqkv[T:].any() and gx.abs().sum() > 0
        assert torch.allclose(db, gx.sum(0) + 0.5, rtol=0, atol=1e-5 * gx.abs().sum(0).max().item())
