"""Evaluation on the GPU: the metric kernels (csrc/kernels/eval_metrics.hip) against their PyTorch mirrors and fp64,
the eval-mode forward (``bn_fwd_infer`` and the layer-wise ResNet path that ends in it), and the Evaluator on the card.

Comparison rules, as in tests/test_bert_rows_gpu.py: exact (``torch.equal``) where the arithmetic is exact -- ranks and
counts are integers -- and bounds derived from the number formats and the kernels' reduction layout otherwise, never
from the kernels' output.  Every check prints its figure before it asserts.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import dtg  # noqa: F401
from dtg import ops
from dtg.data import DeviceLoader, synthetic_image_set, write_image_shards
from dtg.models import resnet
from dtg.ops.metrics import metric_accumulate, metric_accumulate_ref, xent_topk, xent_topk_ref
from dtg.parallel import FlatParams
from dtg.train import Evaluator

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")

BF16_ROW = 2.0 ** -7  # the per-row rule of test_bert_rows_gpu.py; these outputs are rounded to bf16 once (2^-8)
F32_EPS = 2.0 ** -24  # fp32 unit roundoff
WAVE_ROW_MAX_V = 2048  # eval_metrics.hip::kWaveRowMaxV: up to here a wave takes a row, beyond it a workgroup does


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ------------------------------------------------------------------------------------------------ xent_rank
# (path, V, B).  The launcher's threshold between the two forms is V <= 2048, between the issue's 1008 and 4104, so
# its sizes stand: V = 1000 is the vector path in the wave-per-row form (125 chunks: a full 64-lane iteration and a
# partly filled second one), 1001 and the 2-byte-offset 1008 its scalar paths (16 iterations, the last partial), fp32
# 257 (5 iterations, the last holds one column), 4104 the workgroup-per-row form (513 chunks: two full 256-lane
# iterations and one chunk in the third), 30528 the MLM decoder width (3816 chunks: 15 iterations, the last partial).
# B = 9 in the wave form: the third workgroup holds one row and three waves that leave.
PATHS = [("fp32", 257, 9), ("bf16", 1000, 9), ("bf16", 1001, 9), ("bf16-unaligned", 1008, 9), ("bf16", 4104, 9),
         ("bf16", 30528, 5)]


def place(path, x32):
    """x32 in the path's dtype and placement; 'bf16-unaligned' is the contiguous view that starts 2 bytes into its
    storage (test_bert_rows_gpu.py::xent_logits): vector-eligible by shape, scalar by address"""
    B, V = x32.shape
    if path == "fp32":
        return x32.clone()
    if path == "bf16":
        return x32.bfloat16()
    store = torch.empty(B * V + 8, device=dev, dtype=torch.bfloat16)
    view = store[1:1 + B * V].view(B, V)
    view.copy_(x32)
    assert view.is_contiguous() and view.data_ptr() % 16 == 2
    return view


def is_vec(path, V):
    return path == "bf16" and V % 8 == 0


def loss_tol(path, V):
    """Bound on |loss - fp64| for finite logits with |x| <= 16, from the kernel's layout, doubled at the end:

    * lse = M + log S with M exact.  S sums the V terms exp(x - M).  A term reaches S through a product of fast-exp
      factors (its own, the rescales of its lane's running sum, of the 6 butterfly levels and of the block combine)
      whose arguments are all <= 0 and add up to x - M, so the argument roundings (x * log2(e) in fp32) add up to
      what one exp of x - M would have: 3.5e-6 down to -40, with its ulps 4e-6 (XENT_LSE_TOL's figure).  Every factor
      after the first adds its own ulps and the product's rounding, 3 * 2^-24: at most one per lane iteration, 6 in
      the butterfly, 1 in the block combine.
    * the additions: a lane adds 8 terms (vector path) or 1 per iteration, then 6 butterfly levels, then 4 wave
      partials in the workgroup form; each addition rounds S by at most 2^-24 of itself.
    * log S keeps S's relative error as an absolute one; the fast log and the addition to M at |lse| <= 16 add
      1.5e-6 (XENT_LSE_TOL's figure); the subtraction of the label's logit rounds once more at |loss| < 32."""
    vec, block = is_vec(path, V), V > WAVE_ROW_MAX_V
    iters = math.ceil((V // 8 if vec else V) / (256 if block else 64))
    chain = iters * (8 if vec else 1) + 6 + (4 if block else 0)
    factors = iters + 6 + (1 if block else 0)
    return 2 * (4e-6 + (3 * factors + chain) * F32_EPS + 1.5e-6 + 32 * F32_EPS)


def check_against_mirror(name, path, x, labels):
    """rank: exactly the mirror's.  loss: exactly 0 on ignored / out-of-range rows, NaN or +inf where the mirror's
    is, and within loss_tol of fp64 elsewhere."""
    B, V = x.shape
    loss, rank = xent_topk(x, labels)
    ref_loss, ref_rank = xent_topk_ref(x, labels)
    assert loss.dtype == torch.float32 and rank.dtype == torch.int32 and loss.shape == rank.shape == (B,)
    print(f"[rank] {name}: kernel {rank.tolist()} mirror {ref_rank.tolist()}")
    assert torch.equal(rank, ref_rank), name
    off = (labels < 0) | (labels >= V)
    assert (loss[off] == 0).all(), name
    nan = torch.isnan(ref_loss)
    assert torch.equal(torch.isnan(loss), nan), name
    inf = torch.isinf(ref_loss)
    assert torch.equal(loss[inf], ref_loss[inf]), name
    ok = ~off & ~nan & ~inf
    if ok.any():
        x64 = x[ok].double()
        ref64 = torch.logsumexp(x64, -1) - x64.gather(1, labels[ok][:, None])[:, 0]
        assert x64[torch.isfinite(x64)].abs().max().item() <= 16 and ref64.abs().max().item() < 32  # loss_tol's premises
        err = (loss[ok].double() - ref64).abs().max().item()
        tol = loss_tol(path, V)
        print(f"[loss] {name}: max |loss - fp64| = {err:.3e} bound {tol:.3e}")
        assert err <= tol, (name, err, tol)
    return loss, rank, ref_rank


@pytest.mark.parametrize("path,V,B", PATHS)
def test_rank_integer_logits_every_row_ties(path, V, B):
    g = gen(100 + V)
    x32 = torch.randint(-4, 5, (B, V), device=dev, generator=g).float()
    labels = torch.randint(0, V, (B,), device=dev, generator=g)
    labels[0], labels[1] = 0, V - 1
    x = place(path, x32)
    xl = x.float().gather(1, labels[:, None])
    ties = (x.float() == xl).sum(1) - 1
    lower = ((x.float() == xl) & (torch.arange(V, device=dev)[None, :] < labels[:, None])).sum(1)
    print(f"[rank] {path} V={V} ints: ties per row {ties.tolist()}, of them in lower columns {lower.tolist()}")
    assert (ties >= 1).all()  # every row has a tie with its label's logit
    assert (lower[2:] > 0).any() and (lower < ties).any()  # ties on both sides of the label: the rule decides
    check_against_mirror(f"{path} V={V} ints", path, x, labels)


@pytest.mark.parametrize("path,V,B", PATHS)
def test_rank_at_the_topk_boundaries(path, V, B):
    """labels placed by the reference's own sort at positions 0, 1, 4, 5, 6 and V - 1: k - 1 and k for k = 1 and 5"""
    g = gen(200 + V)
    x = place(path, torch.randn(B, V, device=dev, generator=g) * 3)
    order = torch.sort(x.float(), dim=1, descending=True, stable=True).indices
    pos = torch.tensor([0, 1, 4, 5, 6, V - 1], device=dev)[torch.arange(B, device=dev) % 6]
    labels = order.gather(1, pos[:, None])[:, 0]
    _, _, ref_rank = check_against_mirror(f"{path} V={V} randn", path, x, labels)
    assert torch.equal(ref_rank.long(), pos)  # a stable descending sort breaks ties toward the lower column too
    assert {0, 1, 4, 5} <= set(ref_rank.tolist())


@pytest.mark.parametrize("path,V,B", PATHS)
def test_rank_special_rows(path, V, B):
    g = gen(300 + V)
    x32 = torch.randn(B, V, device=dev, generator=g) * 3
    labels = torch.randint(0, V, (B,), device=dev, generator=g)
    labels[0], labels[1] = -1, V  # ignored; out of range (the row is never indexed with it)
    x32[2, labels[2]] = float("nan")  # the label's logit is NaN
    x32[3, (labels[3] + V // 2) % V] = float("nan")  # a NaN elsewhere in the row
    cols = torch.arange(V, device=dev)
    m = (cols % 3 == 1)[None, :] & (cols[None, :] != labels[:, None])
    m[:4] = False
    x32 = x32.masked_fill(m, float("-inf"))  # rows 4..: a third of the non-label columns masked out
    if B >= 9:  # +inf (an overflowed logit) is not NaN: the logsumexp is +inf, and the rank still counts
        x32[7, (labels[7] + V // 2) % V] = float("inf")  # elsewhere in the row: loss +inf, one more column above
        x32[8, labels[8]] = float("inf")  # at the label and at one other column: loss inf - inf, the tie rule ranks
        x32[8, (labels[8] + V // 2) % V] = float("inf")
    x = place(path, x32)
    loss, rank, _ = check_against_mirror(f"{path} V={V} special", path, x, labels)
    assert rank[:4].tolist() == [-1, -2, V, V] and (rank[4:] >= 0).all() and (rank[4:] < V).all()
    assert torch.isfinite(loss[4:7]).all() and torch.isnan(loss[2:4]).all()
    if B >= 9:
        assert loss[7] == float("inf") and torch.isnan(loss[8]) and rank[8] in (0, 1)


@pytest.mark.parametrize("path,V,B", PATHS)
def test_no_access_outside_the_rows(path, V, B):
    """the same [B, V] logits inside a larger NaN-filled buffer score bit for bit as their standalone copy (a read
    outside the view would turn a loss NaN or move a rank), and outputs embedded in sentinel-filled buffers leave
    their surroundings untouched"""
    g = gen(400 + V)
    dt = torch.float32 if path == "fp32" else torch.bfloat16
    lead = V + (1 if path == "bf16-unaligned" else 0)  # V % 8 == 0 keeps the vector path's 16-byte alignment
    big = torch.full((lead + (B + 1) * V + 8,), float("nan"), device=dev, dtype=dt)
    view = big[lead:lead + B * V].view(B, V)
    view.copy_(torch.randn(B, V, device=dev, generator=g) * 3)
    if path == "bf16-unaligned":
        assert view.data_ptr() % 16 == 2
    elif is_vec(path, V):
        assert view.data_ptr() % 16 == 0
    labels = torch.randint(0, V, (B,), device=dev, generator=g)
    labels[0], labels[B - 1] = 0, V - 1  # the first and the last element of the view
    lbuf = torch.full((B + 16,), -7.5, device=dev)
    rbuf = torch.full((B + 16,), -77, device=dev, dtype=torch.int32)
    loss, rank = xent_topk(view, labels, out=(lbuf[8:8 + B], rbuf[8:8 + B]))
    alone = place(path, view.float()) if path == "bf16-unaligned" else view.clone()
    loss1, rank1 = xent_topk(alone, labels)
    print(f"[view] {path} V={V}: ranks {rank.tolist()} standalone {rank1.tolist()}")
    assert torch.isfinite(loss).all() and torch.equal(loss, loss1) and torch.equal(rank, rank1)
    assert loss.data_ptr() == lbuf[8:].data_ptr() and rank.data_ptr() == rbuf[8:].data_ptr()
    assert (lbuf[:8] == -7.5).all() and (lbuf[8 + B:] == -7.5).all()
    assert (rbuf[:8] == -77).all() and (rbuf[8 + B:] == -77).all()


def test_xent_topk_no_rows_and_bad_arguments():
    loss, rank = xent_topk(torch.empty(0, 1000, device=dev, dtype=torch.bfloat16),
                           torch.empty(0, device=dev, dtype=torch.int64))
    assert loss.shape == rank.shape == (0,)
    acc = torch.full((8,), 3.0, device=dev, dtype=torch.float64)
    metric_accumulate(acc, loss, rank, (1,), 1000)  # B == 0 launches nothing
    assert (acc == 3.0).all()
    x, y = torch.zeros(4, 16, device=dev), torch.zeros(4, device=dev, dtype=torch.int64)
    with pytest.raises(ValueError):
        xent_topk(x.half(), y)
    with pytest.raises(ValueError):
        xent_topk(x, y.cpu())
    loss, rank = xent_topk(x, y)
    for bad in (lambda: ops.lib().metric_accumulate(acc, loss, rank, [], 16),
                lambda: ops.lib().metric_accumulate(acc, loss, rank, [1, 2, 3, 4, 5], 16),
                lambda: ops.lib().metric_accumulate(acc.float(), loss, rank, [1], 16),
                lambda: ops.lib().metric_accumulate(acc[:7], loss, rank, [1], 16),
                lambda: ops.lib().metric_accumulate(acc.cpu(), loss, rank, [1], 16),
                lambda: ops.lib().metric_accumulate(acc, loss[:3], rank, [1], 16),
                lambda: ops.lib().xent_rank(x[:, ::2], y)):
        with pytest.raises(RuntimeError):
            bad()


# ---------------------------------------------------------------------------------------- metric_accumulate
def _scored_batch(B, seed, with_bad=True):
    """(loss, rank) of the kernel on B fp32 rows of V = 257; with_bad: rows with label V and a NaN logit too"""
    g = gen(seed)
    V = 257
    x = torch.randn(B, V, device=dev, generator=g) * 3
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    pos = torch.randint(0, 8, (B,), device=dev, generator=g)  # ranks 0..7: both sides of k = 1 and 5
    labels = order.gather(1, pos[:, None])[:, 0]
    if B > 4:
        labels[1] = -1
        if with_bad:
            labels[2] = V
            x[3, labels[3]] = float("nan")
    loss, rank = xent_topk(x, labels)
    return loss, rank, V


@pytest.mark.parametrize("B", [1, 300])
def test_metric_accumulate_counts_and_sum(B):
    """B = 300 is past one sweep of the 256 lanes.  Counts equal the mirror's exactly; slot 1 is the fp64 sum of
    the kernel's own fp32 losses, within (B + 8) * 2^-53 relative: fp64 additions in another order."""
    ks = (1, 5, 3, 257)
    loss, rank, V = _scored_batch(B, 500 + B)
    acc = torch.zeros(8, device=dev, dtype=torch.float64)
    ref = torch.zeros(8, device=dev, dtype=torch.float64)
    assert metric_accumulate(acc, loss, rank, ks, V) is acc
    metric_accumulate_ref(ref, loss, rank, ks, V)
    counts = [0, 2, 3, 4, 5, 6, 7]
    print(f"[acc] B={B} with label V and NaN rows: kernel {acc.tolist()} mirror {ref.tolist()}")
    assert torch.equal(acc[counts], ref[counts])
    if B > 4:
        assert acc[2] == 1 and acc[3] == 1 and acc[0] == B - 2 and math.isnan(acc[1].item())
        assert 0 < acc[4] < acc[6] < acc[5] < acc[7] == B - 3  # k = 1 < 3 < 5 < 257; rank V is a miss at k = V too
    # the loss sum, on a batch without NaN rows
    loss, rank, V = _scored_batch(B, 600 + B, with_bad=False)
    acc = torch.zeros(8, device=dev, dtype=torch.float64)
    metric_accumulate(acc, loss, rank, ks, V)
    want = loss.double()[rank >= 0].sum().item()
    err = abs(acc[1].item() - want) / abs(want)
    print(f"[acc] B={B}: loss sum {acc[1].item():.15e} fp64 sum of the fp32 losses {want:.15e} "
          f"rel err {err:.3e} bound {(B + 8) * 2.0 ** -53:.3e}")
    assert err <= (B + 8) * 2.0 ** -53
    again = torch.zeros(8, device=dev, dtype=torch.float64)
    metric_accumulate(again, loss, rank, ks, V)
    assert torch.equal(acc, again)  # one workgroup, a fixed order: the same bits


def test_metric_accumulate_two_batches_into_one_accumulator():
    ks = (1, 5)
    buf = torch.full((24,), -3.0, device=dev, dtype=torch.float64)
    acc = buf[8:16]
    acc.zero_()
    ref = torch.zeros(8, device=dev, dtype=torch.float64)
    parts = [_scored_batch(300, 701, with_bad=False), _scored_batch(37, 702, with_bad=False)]
    for loss, rank, V in parts:
        metric_accumulate(acc, loss, rank, ks, V)
        metric_accumulate_ref(ref, loss, rank, ks, V)
    print(f"[acc] 300 + 37 rows: kernel {acc.tolist()} mirror {ref.tolist()}")
    assert torch.equal(acc[[0, 2, 3, 4, 5, 6, 7]], ref[[0, 2, 3, 4, 5, 6, 7]]) and acc[0] == 335 and acc[6] == 0
    want = sum(l.double()[r >= 0].sum().item() for l, r, _ in parts)
    assert abs(acc[1].item() - want) / abs(want) <= (337 + 8) * 2.0 ** -53
    assert (buf[:8] == -3.0).all() and (buf[16:] == -3.0).all()  # the accumulator's surroundings
    acc2 = torch.zeros(8, device=dev, dtype=torch.float64)
    for loss, rank, V in parts:
        metric_accumulate(acc2, loss, rank, ks, V)
    assert torch.equal(acc2, acc)


# ----------------------------------------------------------------------------------------- eval-mode BatchNorm
def row_err(out, ref64):
    d = (out.double() - ref64).abs().amax(-1)
    s = ref64.abs().amax(-1).clamp_min(torch.finfo(torch.float64).tiny)
    return (d / s).max().item()


@pytest.mark.parametrize("C", [8, 64, 2048])
@pytest.mark.parametrize("M", [1, 37, 150])
@pytest.mark.parametrize("res,relu", [(False, False), (False, True), (True, False), (True, True)])
def test_batch_norm_act_inference_against_fp64(C, M, res, relu):
    """bn_fwd_infer through ops.batch_norm_act(training=False).  A workgroup of bn_apply_kernel takes 2 x RPP rows
    (RPP = 32 for C <= 64, 4 for C = 2048) and a thread two of them: M = 1 is a lone row, M = 37 a second row for
    some threads only (C <= 64) or several workgroups with a partial last one, M = 150 is past a single workgroup's
    rows at every C (2 x 64 + 22).  One rounding of the output: the BF16_ROW rule."""
    g = gen(800 + C + M)
    x = (torch.randn(M, C, device=dev, generator=g) * 2 + 0.5).bfloat16()
    r = torch.randn(M, C, device=dev, generator=g).bfloat16() if res else None
    gamma = torch.rand(C, device=dev, generator=g) + 0.5
    beta = torch.randn(C, device=dev, generator=g)
    rmean = torch.randn(C, device=dev, generator=g) * 0.7 + 0.3
    rvar = torch.rand(C, device=dev, generator=g) * 3 + 0.25
    rm0, rv0 = rmean.clone(), rvar.clone()
    as4 = lambda t: t.view(M, 1, 1, C).permute(0, 3, 1, 2)  # noqa: E731  [M, C, 1, 1] channels_last over [M, C]
    y = ops.batch_norm_act(as4(x), gamma, beta, rmean, rvar, training=False, eps=1e-5,
                           residual=as4(r) if res else None, relu=relu)
    y = y.permute(0, 2, 3, 1).reshape(M, C)
    ref = (x.double() - rmean.double()) * torch.rsqrt(rvar.double() + 1e-5) * gamma.double() + beta.double()
    if res:
        ref = ref + r.double()
    if relu:
        ref = ref.clamp_min(0)
    e = row_err(y, ref)
    print(f"[bn infer] C={C} M={M} res={res} relu={relu}: err={e:.3e} bound={BF16_ROW:.3e} "
          f"(fp64->bf16 floor {row_err(ref.bfloat16(), ref):.3e})")
    assert y.dtype == torch.bfloat16 and torch.isfinite(y.float()).all()
    assert e <= BF16_ROW
    if relu:
        assert (y >= 0).all() and ((y == 0).any() or M * C < 256)
    assert torch.equal(rmean, rm0) and torch.equal(rvar, rv0)  # inference leaves the running statistics alone


# -------------------------------------------------------------------------------------- eval-mode ResNet-50
def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _ref_cbn(P, Bf, x, pre, stride=1, pad=0, relu=True, res=None, training=False):
    """conv -> BN (inference: the running statistics; training: the batch's) (-> + res) (-> relu) in fp32 torch, rounded
    to bf16 where the layer-wise path stores bf16: the conv output and the BN pass's output"""
    y = _bf(F.conv2d(x, P[pre + ".conv.weight"], None, stride, pad))
    if training:
        y = F.batch_norm(y, None, None, P[pre + ".bn.weight"], P[pre + ".bn.bias"], True, 0.0, 1e-5)
    else:
        y = F.batch_norm(y, Bf[pre + ".bn.running_mean"], Bf[pre + ".bn.running_var"], P[pre + ".bn.weight"],
                         P[pre + ".bn.bias"], False, 0.0, 1e-5)
    if res is not None:
        y = y + res
    if relu:
        y = F.relu(y)
    return _bf(y)


def _ref_logits(model, P, Bf, x32, training=False):
    """the layer-wise forward of models/resnet.py in fp32 on the CPU, bf16 storage points emulated"""
    kw = dict(training=training)
    h = _ref_cbn(P, Bf, x32, "stem", 2, 3, **kw)
    h = F.max_pool2d(h, 3, 2, 1)
    for i, blk in enumerate(model.blocks):
        pre, st = "blocks.%d" % i, blk.c2.conv.stride
        idn = _ref_cbn(P, Bf, h, pre + ".down", st, 0, relu=False, **kw) if blk.down is not None else h
        t = _ref_cbn(P, Bf, h, pre + ".c1", **kw)
        t = _ref_cbn(P, Bf, t, pre + ".c2", st, 1, **kw)
        h = _ref_cbn(P, Bf, t, pre + ".c3", res=idn, **kw)
    h = _bf(h.mean(dim=(2, 3)))
    return _bf(F.linear(h, P["fc.weight"], P["fc.bias"]))


def _ref_params(model, noise=0.0, seed=11):
    """the model's parameters as fp32 CPU tensors, conv / FC weights rounded as the bf16 compute mirror holds them"""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for n, p in model.named_parameters():
        t = p.detach().float().cpu().contiguous().clone()
        if noise:
            t = t * (1 + noise * torch.randn(t.shape, generator=g))
        P[n] = _bf(t) if p.dim() > 1 else t
    return P


def _seed_bn(model):
    """BN parameters as tests/test_resnet_gpu.py::_seed_bn draws them (zero-init c3 gammas would hide every residual
    branch), and running statistics away from (0, 1)"""
    from dtg.models.layers import BatchNorm2d
    for name, m in model.named_modules():
        if isinstance(m, BatchNorm2d):
            m.weight.data.uniform_(*((0.1, 0.3) if name.endswith("c3.bn") else (0.8, 1.2)))
            m.bias.data.uniform_(-0.2, 0.2)
            m.running_mean.normal_(0.0, 0.3)
            m.running_var.uniform_(0.5, 2.0)


_rel = lambda a, b: ((a - b).norm() / (b.norm() + 1e-12)).item()  # noqa: E731


def test_resnet50_eval_forward_matches_fp32_reference():
    """ResNet-50(100) in eval(): fused_ok / stem_ok are false, so every layer runs conv + bn_fwd_infer.  The logits
    are held to the project's noise-floor rule: within 1.6 x the fp32 reference's own movement under 2^-9 relative
    weight noise, plus 0.02.  Negative control: the same reference with training-mode BN lies at least twice as far."""
    torch.manual_seed(0)
    model = resnet.resnet50(100).to(dev).to(memory_format=torch.channels_last)
    _seed_bn(model)
    FlatParams(model)
    model.eval()
    x, _ = resnet.synthetic_batch(4, dev, torch.bfloat16, 64, 100, seed=3)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        logits = model(x)
    torch.cuda.synchronize()
    assert logits.shape == (4, 100) and torch.isfinite(logits.float()).all()
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    got = logits.float().cpu()
    Bf = {n: b.detach().float().cpu() for n, b in model.named_buffers()}
    x32 = x.float().cpu()
    with torch.no_grad():
        ref = _ref_logits(model, _ref_params(model), Bf, x32)
        noisy = _ref_logits(model, _ref_params(model, noise=2 ** -9), Bf, x32)
        train_bn = _ref_logits(model, _ref_params(model), Bf, x32, training=True)
    e, e_noise, e_bad = _rel(got, ref), _rel(noisy, ref), _rel(got, train_bn)
    print("[resnet50 eval] logits rel err %.4f; fp32 reference under 2^-9 weight noise %.4f (bound %.4f); against "
          "training-mode BN %.4f; |ref| %.3f" % (e, e_noise, 1.6 * e_noise + 0.02, e_bad, ref.norm().item()))
    assert e <= 1.6 * e_noise + 0.02
    assert e_bad >= 2.0 * e


# ------------------------------------------------------------------------------------- the Evaluator on the card
def test_evaluator_on_the_gpu(tmp_path):
    """tiny ResNet, bf16, 50 generated records at batch 8 (7 steps, the last with 2 records and 6 padding rows): the
    counts equal those of the same batches' logits through the mirrors, and a second run() gives the same bits"""
    images, labels = synthetic_image_set(50, size=36, classes=10, seed=6)
    write_image_shards(str(tmp_path), images, labels, per_shard=20)
    torch.manual_seed(1)
    model = resnet.resnet18_like_tiny(10).to(dev).to(memory_format=torch.channels_last)
    _seed_bn(model)
    FlatParams(model)
    model.train()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    ks = (1, 5)
    with DeviceLoader(str(tmp_path), 8, 32, torch.device("cuda", 0), train=False, drop_last=False) as loader:
        ev = Evaluator(model, loader, ks=ks)
        first = ev.run()
        second = ev.run()
        assert model.training
        # the same batches once more, by hand, through the mirrors
        ref = torch.zeros(8, device=dev, dtype=torch.float64)
        model.eval()
        loader.seek(0)
        seen = []
        with torch.no_grad():
            for _ in range(loader.steps_per_epoch):
                x, y, idx = loader.next()
                logits = model(x)
                assert logits.dtype == torch.bfloat16 and logits.shape == (8, 10)
                l, r = xent_topk_ref(logits, y)
                metric_accumulate_ref(ref, l, r, ks, 10)
                seen.extend(idx[y.cpu() >= 0].tolist())
        model.train()
    ref = ref.tolist()
    print("[evaluator] first %s\n[evaluator] mirror sums %s" % (first, ref))
    assert seen == list(range(50))
    assert first["n"] == 50 == int(ref[0]) and first["bad_labels"] == 0 and first["nonfinite"] == 0
    assert first["top1_count"] == int(ref[4]) and first["top5_count"] == int(ref[5])
    assert 0 < first["top5_count"] < 50
    # the kernel's fp32 losses against the mirror's on bf16 logits of 10 classes: loss_tol's bound per row
    assert abs(first["loss"] - ref[1] / 50) <= loss_tol("bf16", 10)
    for k in ("n", "loss", "loss_sum", "top1", "top5", "top1_count", "top5_count", "bad_labels", "nonfinite"):
        assert first[k] == second[k], k  # bit-equal: the same kernels in the same order
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
