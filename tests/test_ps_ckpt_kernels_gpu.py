"""state_pack / state_unpack (csrc/kernels/snapshot.hip) against ``_view_like(buf, off, p).contiguous()``.
The kernels only copy, so every comparison is bit-exact.  A few hundred thousand elements in total."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu


def _cl(*shape):
    return torch.empty(*shape).to(memory_format=torch.channels_last)


def _params():
    return [torch.empty(5),              # shorter than a 16-byte vector
            torch.empty(64),
            torch.empty(7, 13),
            _cl(5, 3, 3, 3),             # odd I and RS
            _cl(4, 8, 1, 1),             # 1x1: _view_like does not permute it -> an identity row
            _cl(16, 16, 3, 3),           # 2304 elements: a chunk boundary in the middle of an o
            _cl(64, 3, 7, 7),            # RS = 49
            _cl(256, 128, 3, 3)]         # many chunks


def _layout(params):
    from dtg.parallel.flat import _align
    offs, off = [], 0
    for p in params:
        offs.append(off)
        off += _align(p.numel())
    return offs, off


def _padding_mask(offs, params, n, dev):
    pad = torch.ones(n, dtype=torch.bool, device=dev)
    for o, p in zip(offs, params):
        pad[o:o + p.numel()] = False
    return pad


@pytest.fixture(scope="module")
def case():
    import dtg  # noqa: F401
    from dtg.ops import snapshot as S
    dev = torch.device("cuda", 0)
    params = _params()
    offs, n = _layout(params)
    plan = S.SnapshotPlan(offs, params, n, dev)
    g = torch.Generator().manual_seed(0)
    srcs = [torch.randn(n, generator=g).to(dev) for _ in range(3)]
    return S, dev, params, offs, n, plan, srcs


def test_plan_rows_follow_view_like(case):
    S, dev, params, offs, n, plan, srcs = case
    rows = plan.rows.tolist()
    assert rows[4] == [offs[4], 32, 1, 1]          # the 1x1 conv is an identity row
    assert rows[3] == [offs[3], 135, 3, 9] and rows[6] == [offs[6], 64 * 3 * 49, 3, 49]
    assert [r[3] for r in rows[:3]] == [1, 1, 1]
    assert plan.chunks_dev.shape == (sum((p.numel() + 2047) // 2048 for p in params), 2)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_pack_unpack_against_view_like(case, k):
    from dtg.parallel.flat import _view_like
    S, dev, params, offs, n, plan, srcs = case
    srcs = srcs[:k]
    keep = [s.clone() for s in srcs]
    image = plan.new_image(k)
    S.state_pack(plan, srcs, image)
    pad = _padding_mask(offs, params, n, dev)
    for j in range(k):
        assert torch.equal(srcs[j], keep[j])                       # the sources are unchanged
        assert (image[j][pad] == 0).all()                          # image padding is still zero
        for o, p in zip(offs, params):
            want = _view_like(srcs[j], o, p).contiguous()
            assert torch.equal(image[j, o:o + p.numel()].view(p.shape), want), (j, tuple(p.shape))
    # unpack(pack(x)) == x on parameter elements; a sentinel in the destination's padding survives
    dsts = [torch.full((n,), -7.0, device=dev) for _ in range(k)]
    S.state_unpack(plan, dsts, image)
    for j in range(k):
        assert torch.equal(dsts[j][~pad], srcs[j][~pad])
        assert (dsts[j][pad] == -7.0).all()
    # the CPU mirror computes the same image
    cplan = S.SnapshotPlan(offs, params, n, "cpu")
    cimg = cplan.new_image(k)
    S.state_pack(cplan, [s.cpu() for s in srcs], cimg)
    assert torch.equal(cimg, image.cpu())
    cd = [torch.full((n,), -7.0) for _ in range(k)]
    S.state_unpack(cplan, cd, cimg)
    assert all(torch.equal(a, b.cpu()) for a, b in zip(cd, dsts))


def _convbn_linear():
    from dtg.models.layers import ConvBN, Linear

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c = ConvBN(3, 5, 3, padding=1)
            self.f = Linear(5, 4)

    torch.manual_seed(0)
    return M()


@pytest.mark.parametrize("which", ["convbn_linear", "resnet18_like_tiny"])
def test_pack_unpack_real_model(which):
    import dtg  # noqa: F401
    from dtg.models import resnet
    from dtg.ops import snapshot as S
    from dtg.parallel import FlatParams
    from dtg.parallel.flat import _view_like
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = _convbn_linear() if which == "convbn_linear" else resnet.resnet18_like_tiny(10)
    model = model.to(dev).to(memory_format=torch.channels_last)
    flat = FlatParams(model)
    permuted = 0
    for g in flat:
        plan = S.SnapshotPlan.of_group(g)
        permuted += int((plan.rows[:, 3] > 1).sum())
        slot = torch.randn(g.numel, device=dev)
        image = plan.new_image(2)
        S.state_pack(plan, [g.master, slot], image)
        for i, (n, p, o, numel) in enumerate(g.param_slices()):
            assert torch.equal(image[0, o:o + numel].view(p.shape), g.master_view(i).contiguous()), n
            assert torch.equal(image[1, o:o + numel].view(p.shape), _view_like(slot, o, p).contiguous()), n
        back = [torch.full_like(g.master, 3.0), torch.full_like(g.master, 3.0)]
        S.state_unpack(plan, back, image)
        pad = _padding_mask(g.offsets, g.params, g.numel, dev)
        assert torch.equal(back[0][~pad], g.master[~pad]) and torch.equal(back[1][~pad], slot[~pad])
        assert (back[0][pad] == 3.0).all() and (back[1][pad] == 3.0).all()
    assert permuted >= 1  # the models do hold channels_last k x k conv weights


def test_bindings_refuse_before_launch(case):
    from dtg.ops import lib
    S, dev, params, offs, n, plan, srcs = case
    C = lib()

    def pack(bufs, image, rows=None, plan_=plan):
        C.state_pack(bufs, image, plan_.rows if rows is None else rows, plan_.rows_dev, plan_.chunks_dev)

    with pytest.raises(RuntimeError, match="1..4 state buffers"):
        pack([srcs[0]] * 5, torch.zeros(5 * n, device=dev))
    with pytest.raises(RuntimeError, match="must be fp32"):
        pack([srcs[0], srcs[1].to(torch.bfloat16)], plan.new_image(2))
    with pytest.raises(RuntimeError, match="size mismatch"):
        pack([srcs[0], srcs[1][:n - 64]], plan.new_image(2))
    past = plan.rows.clone()
    past[-1, 1] += 64  # the last row now ends past the buffer
    with pytest.raises(RuntimeError, match="outside the buffer"):
        pack([srcs[0]], plan.new_image(1), rows=past)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        big = torch.zeros(n + 4, device=dev)
        pack([big[1:n + 1]], plan.new_image(1))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        rows = torch.tensor([[2, 5, 1, 1]])
        p2 = S.SnapshotPlan([0], [torch.empty(5)], 64, dev)
        C.state_unpack([torch.zeros(64, device=dev)], torch.zeros(64, device=dev), rows, p2.rows_dev, p2.chunks_dev)
    with pytest.raises(RuntimeError, match="chunk table"):
        C.state_pack([srcs[0]], plan.new_image(1), plan.rows, plan.rows_dev, plan.chunks_dev[:-1].contiguous())
    torch.cuda.synchronize()
