"""BERT on data, on the GPU: the masking kernel (csrc/kernels/mlm_mask.hip) bit for bit against its PyTorch mirror,
its memory accesses inside sentinel-filled buffers, the token loader's ring against the CPU loader, the eval-mode
logits of the fused path under the project's noise-floor rule, BertEvaluator on the card, and one training step fed by
the loader.

The masking rule is integer only, so every comparison of it is ``torch.equal``.
"""
import os
import sys

import pytest
import torch

import dtg  # noqa: F401
from dtg.data import TokenLoader, masking_args, synthetic_token_set, write_token_meta, write_token_shards
from dtg.models import bert
from dtg.ops.metrics import metric_accumulate_ref, xent_topk_ref
from dtg.ops.mlm import mlm_mask, mlm_mask_ref
from dtg.parallel import FlatParams
from dtg.train import BertEvaluator

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bert_cases import HI, IDS, LO, make_rows  # noqa: E402

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
dev0 = torch.device("cuda", 0)  # the loaders open a stream on it
NAMES = ("ids", "token_types", "attention_mask", "positions", "labels")


def _to_dev(rows):
    return tuple(t.to(dev) for t in rows)


# ------------------------------------------------------------------------------------------------ kernel == mirror
# S: below a wave, one full chunk of 64, chunk plus tail, the production shapes 128 and 512, past 8 chunks, the limit.
@pytest.mark.parametrize("S", [8, 64, 72, 128, 512, 520, 2048])
def test_kernel_equals_mirror(S):
    """B in {1, 3, 5, 256} (row counts that do not fill a workgroup of 4 rows), P in {1, 20, 80}, key_bits in {4, 32},
    valid_rows in {0, B - 2, B}; lengths 0, 1, 4, S and random ones"""
    n = 0
    for B in (1, 3, 5, 256):
        rows = _to_dev(make_rows(B, S, seed=S * 7 + B))
        for P in (1, 20, 80):
            for key_bits in (4, 32):
                for valid_rows in sorted({0, max(B - 2, 0), B}):
                    kw = dict(IDS, seed=S + 13, epoch=P, P=P, key_bits=key_bits, valid_rows=valid_rows)
                    got = mlm_mask(*rows, **kw)
                    want = mlm_mask_ref(*rows, **kw)
                    for name, g, w in zip(NAMES, got, want):
                        assert g.dtype == torch.int64 and g.shape == w.shape
                        assert torch.equal(g, w), (name, B, P, key_bits, valid_rows)
                    n += 1
    torch.cuda.synchronize()
    print("[mlm_mask] S=%d: %d cases bit-equal" % (S, n))


def test_kernel_masks_a_real_share():
    """not vacuous: at the production shape every full row predicts P tokens, and ties at 4 key bits change the choice"""
    rows = _to_dev(make_rows(64, 128, seed=1, lengths=[128] * 64))
    kw = dict(IDS, seed=3, epoch=0, P=20)
    a, b = mlm_mask(*rows, **kw), mlm_mask(*rows, key_bits=4, **kw)
    assert int((a[4] >= 0).sum()) == 64 * 19 and not torch.equal(a[3], b[3])  # 125 candidates: n_pred = 19
    assert (a[3][:, :19].diff(dim=1) > 0).all() and (a[0] != rows[0]).any()


# ------------------------------------------------------------------------------------------------ no stray accesses
SENT = -0x5A5A5A5A5A5A5A5B


@pytest.mark.parametrize("S,B,P", [(7, 5, 3), (65, 6, 20), (128, 9, 20), (129, 3, 80), (2048, 5, 20)])
@pytest.mark.parametrize("wild", [False, True])
def test_no_stray_accesses(S, B, P, wild):
    """the input rows sit inside a larger buffer of ordinary-looking tokens, the outputs inside sentinel-filled buffers
    at an odd element offset (8 bytes off any 16-byte boundary), odd S included: the result is that of the standalone
    run and every sentinel is intact.  wild: length / a_len far outside [0, S] are clamped, never used as extents."""
    ids, a_len, length, index = make_rows(B, S, seed=S + B)
    if wild:
        length = torch.tensor(([-5, S + 100, 2 ** 31 - 1, -2 ** 31, 3] * B)[:B], dtype=torch.int32)
        a_len = torch.tensor(([7, -1, 2 ** 31 - 1, 5, S + 9] * B)[:B], dtype=torch.int32)
    pad = 3 * S + 5
    g = torch.Generator().manual_seed(1)
    big = torch.randint(LO, HI, (pad + B * S + pad,), generator=g, dtype=torch.int32).to(dev)
    big[pad:pad + B * S] = ids.reshape(-1).to(dev)
    d_ids = big[pad:pad + B * S].view(B, S)
    scal = torch.randint(1, S + 1, (3, 64 + B + 64), generator=g, dtype=torch.int32).to(dev)
    scal[0, 64:64 + B], scal[1, 64:64 + B] = a_len.to(dev), length.to(dev)
    d_alen, d_len = scal[0, 64:64 + B], scal[1, 64:64 + B]
    idx_buf = torch.randint(0, 2 ** 40, (64 + B + 64,), generator=g).to(dev)
    idx_buf[64:64 + B] = index.to(dev)
    d_index = idx_buf[64:64 + B]
    assert d_ids.is_contiguous() and d_len.is_contiguous()
    bufs, outs = [], []
    for cols in (S, S, S, P, P):
        buf = torch.full((1 + 2 * cols + B * cols + 2 * cols + 1,), SENT, dtype=torch.int64, device=dev)
        view = buf[1 + 2 * cols:1 + 2 * cols + B * cols].view(B, cols)
        assert view.data_ptr() % 16 == 8  # an unaligned view for 16-byte stores
        bufs.append(buf)
        outs.append(view)
    kw = dict(IDS, seed=5, epoch=2, P=P, valid_rows=B - 1)
    res = mlm_mask(d_ids, d_alen, d_len, d_index, out=tuple(outs), **kw)
    torch.cuda.synchronize()
    alone = mlm_mask(ids.to(dev), a_len.to(dev), length.to(dev), index.to(dev), **kw)
    want = mlm_mask_ref(ids.to(dev), a_len.to(dev), length.to(dev), index.to(dev), **kw)
    for name, r, a, w, buf, cols in zip(NAMES, res, alone, want, bufs, (S, S, S, P, P)):
        assert torch.equal(r, a) and torch.equal(r, w), name
        lo = 1 + 2 * cols
        assert (buf[:lo] == SENT).all() and (buf[lo + B * cols:] == SENT).all(), name
    if wild:  # rows 0 and 3 clamp to length 0: nothing real, nothing predicted
        assert (res[2][0] == 0).all() and (res[4][0] == -1).all()
        if B > 2:
            assert (res[2][2] == 1).all()  # length 2^31 - 1 clamps to S


def test_binding_refuses_what_it_cannot_run():
    ids, a_len, length, index = _to_dev(make_rows(2, 16, seed=0))
    kw = dict(IDS, seed=0, epoch=0, P=4)
    with pytest.raises(ValueError):
        mlm_mask(torch.zeros(1, 2049, dtype=torch.int32, device=dev), a_len[:1], length[:1], index[:1], **kw)
    from dtg.ops import lib
    out = [torch.empty(2, 16, dtype=torch.int64, device=dev) for _ in range(3)] + \
          [torch.empty(2, 4, dtype=torch.int64, device=dev) for _ in range(2)]
    args = (0, 0, 150, 3, 4, 1000, [0, 1, 2, 3], 2, 32)
    lib().mlm_mask(ids, a_len, length, index, *out, *args)
    with pytest.raises(RuntimeError):  # S beyond the LDS row
        big = [torch.empty(2, 2049, dtype=torch.int64, device=dev) for _ in range(3)] + out[3:]
        lib().mlm_mask(torch.zeros(2, 2049, dtype=torch.int32, device=dev), a_len, length, index, *big, *args)
    with pytest.raises(RuntimeError):  # a strided destination
        lib().mlm_mask(ids, a_len, length, index, torch.empty(2, 32, dtype=torch.int64, device=dev)[:, ::2],
                       *out[1:], *args)
    with pytest.raises(RuntimeError):  # labels of another P
        lib().mlm_mask(ids, a_len, length, index, *out[:4], torch.empty(2, 5, dtype=torch.int64, device=dev), *args)
    with pytest.raises(RuntimeError):
        lib().mlm_mask(ids, a_len, length, index, *out, 0, 0, 150, 3, 4, 1000, [0, 1, 2, 3], 3, 32)  # valid_rows > B
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the loader's ring
SEQ, VOCAB, PRED = 64, 1000, 10
META = dict(pad_id=0, cls_id=1, sep_id=2, mask_id=3, vocab_lo=4, vocab_hi=VOCAB)


@pytest.fixture(scope="module")
def token_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("tokens_gpu")
    write_token_shards(str(d), synthetic_token_set(70, seq=SEQ, vocab_hi=VOCAB, seed=4), 32)
    write_token_meta(str(d), **META)
    return str(d)


def _loader(d, batch, device, **kw):
    return TokenLoader(d, batch, device, P=PRED, **masking_args(META), **kw)


@pytest.mark.parametrize("depth", [1, 3])
def test_loader_ring_equals_cpu_loader(token_dir, depth):
    """12 steps (into the second epoch) at depth 1 and 3, with the stream kept busy in front of every masking launch,
    so the producer is ready to refill a slot long before its kernel has run: the batches are those of the CPU loader
    bit for bit, which they are only if a slot is reused after its kernel"""
    busy = torch.randn(2048, 2048, device=dev)
    with _loader(token_dir, 8, "cpu", seed=6) as cpu, _loader(token_dir, 8, dev0, seed=6, depth=depth) as gpu:
        got, want = [], []
        for _ in range(12):
            for _ in range(4):
                busy = (busy @ busy).clamp_(-1, 1)
            got.append(gpu.next())
            want.append(cpu.next())
        torch.cuda.synchronize()
        for step, (g, w) in enumerate(zip(got, want)):
            assert g[1] == w[1] == int((g[0][4] >= 0).sum()) and torch.equal(g[2], w[2])
            for name, a, b in zip(NAMES + ("nsp",), g[0], w[0]):
                assert a.is_cuda and torch.equal(a.cpu(), b), (step, name)
        c = gpu.counters()
        print("[token loader] depth %d: %s" % (depth, c))
        assert c["batches"] == 12
        gpu.seek(7)
        again = gpu.next()
        assert all(torch.equal(a, b) for a, b in zip(again[0], got[7][0]))


def test_loader_ring_seek_with_a_busy_stream(token_dir):
    """3 batches through 2 slots, seek(1) while their masking launches are still queued behind the matmuls, 4 more: a
    ring that forgot a slot's consumed event at the seek would refill it before its kernel ran"""
    busy = torch.randn(2048, 2048, device=dev)
    with _loader(token_dir, 8, "cpu", seed=6) as cpu, _loader(token_dir, 8, dev0, seed=6, depth=2) as gpu:
        want = [cpu.next() for _ in range(5)]
        got = []
        for n in (3, 4):
            for _ in range(n):
                for _ in range(4):
                    busy = (busy @ busy).clamp_(-1, 1)
                got.append(gpu.next())
            if n == 3:
                gpu.seek(1)  # no synchronise before or after
        torch.cuda.synchronize()
        assert gpu.step == 5 and gpu.counters()["batches"] == 7
        for step, g in zip((0, 1, 2, 1, 2, 3, 4), got):
            w = want[step]
            assert g[1] == w[1] and torch.equal(g[2], w[2])
            for name, a, b in zip(NAMES + ("nsp",), g[0], w[0]):
                assert a.is_cuda and torch.equal(a.cpu(), b), (step, name)


# ------------------------------------------------------------------------------------------------ the model
CFG = dict(vocab_size=1024, hidden=128, layers=2, heads=2, intermediate=512, max_position=128)
_rel = lambda a, b: ((a - b).norm() / (b.norm() + 1e-12)).item()  # noqa: E731


def _model(seed=0):
    torch.manual_seed(seed)
    model = bert.BertForPreTraining(bert.BertConfig(**CFG)).to(dev)
    with torch.no_grad():  # biases and LayerNorm parameters away from (0, 1): an omitted one would show
        for n, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    flat = FlatParams(model)
    return model, flat


def _ref_model(model, noise=0.0, seed=11):
    """the reference path in fp32 on the CPU with the weights as the bf16 mirror holds them; noise: relative weight
    noise, the matrices rounded to bf16 again"""
    g = torch.Generator().manual_seed(seed)
    ref = bert.BertForPreTraining(bert.BertConfig(**CFG))
    state = {}
    for n, p in model.named_parameters():
        t = p.detach().float().cpu().clone()
        if noise:
            t = t * (1 + noise * torch.randn(t.shape, generator=g))
            t = t.bfloat16().float() if p.dim() > 1 else t
        state[n] = t
    ref.load_state_dict(state)
    return ref.eval()


def _batch(B, seed, valid_rows=None):
    rows = make_rows(B, SEQ, seed=seed, lengths=None)
    rows = (rows[0], rows[1].clamp(min=1), rows[2].clamp(min=8), rows[3])  # every row attends to something
    return mlm_mask_ref(*rows, seed=1, epoch=0, P=PRED, valid_rows=valid_rows, **IDS)


def test_pretraining_logits_match_fp32_reference():
    """the fused encoder and head GEMMs in bf16 against the fp32 reference path, under the noise-floor rule of
    test_eval_gpu.py::test_resnet50_eval_forward_matches_fp32_reference: within 1.6 x the reference's own movement
    under 2^-9 relative weight noise, plus 0.02.  No dropout is drawn in train() either and ``_step`` stays."""
    model, _ = _model()
    ids, tt, am, pos, _ = _batch(8, seed=2)
    d = [t.to(dev) for t in (ids, tt, am, pos)]
    assert model.fused_ok(d[0])
    model.train()
    step = model._step
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        mlm_t, nsp_t = model.pretraining_logits(*d)
        model.eval()
        mlm_e, nsp_e = model.pretraining_logits(*d)
    torch.cuda.synchronize()
    assert mlm_e.shape == (8 * PRED, 1024) and nsp_e.shape == (8, 2) and model._step == step
    assert torch.equal(mlm_t, mlm_e) and torch.equal(nsp_t, nsp_e)  # no dropout whatever the flag says
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    with torch.no_grad():
        ref = _ref_model(model).pretraining_logits(ids, tt, am, pos)
        noisy = _ref_model(model, noise=2 ** -9).pretraining_logits(ids, tt, am, pos)
    for name, got, r, nz in (("mlm", mlm_e, ref[0], noisy[0]), ("nsp", nsp_e, ref[1], noisy[1])):
        e, e_noise = _rel(got.float().cpu(), r), _rel(nz, r)
        print("[bert eval logits] %s: rel err %.4f; fp32 reference under 2^-9 weight noise %.4f (bound %.4f); |ref| "
              "%.3f" % (name, e, e_noise, 1.6 * e_noise + 0.02, r.norm().item()))
        assert torch.isfinite(got.float()).all() and e <= 1.6 * e_noise + 0.02


def test_bert_evaluator_on_the_gpu(token_dir):
    """tiny model, bf16, 70 records at batch 8 (9 steps, the last with 6 records and 2 padding rows): the counts equal
    those of the same batches' logits through the metric mirrors, and a second run() gives the same bits"""
    model, _ = _model(seed=1)
    model.train()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    ks = (1, 5)
    with _loader(token_dir, 8, dev0, train=False, drop_last=False, eval_seed=3) as loader:
        ev = BertEvaluator(model, loader, ks=ks)
        first, second = ev.run(), ev.run()
        assert model.training
        ref = torch.zeros(2, 8, device=dev, dtype=torch.float64)
        model.eval()
        loader.seek(0)
        seen = []
        with torch.no_grad():
            for _ in range(loader.steps_per_epoch):
                (ids, tt, am, pos, lab, nsp), _, idx = loader.next()
                ml, nl = model.pretraining_logits(ids, tt, am, pos)
                assert ml.dtype == torch.bfloat16 and ml.shape == (8 * PRED, 1024) and nl.shape == (8, 2)
                l, r = xent_topk_ref(ml, lab.reshape(-1))
                metric_accumulate_ref(ref[0], l, r, ks, 1024)
                l, r = xent_topk_ref(nl, nsp)
                metric_accumulate_ref(ref[1], l, r, (1,), 2)
                seen.extend(idx[nsp.cpu() >= 0].tolist())
        model.train()
    m, s = ref.tolist()
    print("[bert eval gpu] n=%d mlm_n=%d top1=%d top5=%d nsp=%d mlm_loss=%.6f (mirror %.6f) nsp_loss=%.6f (mirror "
          "%.6f)" % (first["n"], first["mlm_n"], first["mlm_top1_count"], first["mlm_top5_count"],
                     first["nsp_correct"], first["mlm_loss"], m[1] / m[0], first["nsp_loss"], s[1] / s[0]))
    assert seen == list(range(70)) and first["n"] == 70 == int(s[0]) and first["mlm_n"] == int(m[0]) > 70
    assert first["mlm_top1_count"] == int(m[4]) and first["mlm_top5_count"] == int(m[5])
    assert first["nsp_correct"] == int(s[4]) and first["bad_labels"] == 0 and first["nonfinite"] == 0
    # the kernel's fp32 losses against the mirror's, per row within test_eval_gpu.py::loss_tol's bound for the path
    from test_eval_gpu import loss_tol
    assert abs(first["mlm_loss"] - m[1] / m[0]) <= loss_tol("bf16", 1024)
    assert abs(first["nsp_loss"] - s[1] / s[0]) <= loss_tol("fp32", 2)
    drop = ("seconds", "sequences_per_sec")
    assert {k: v for k, v in first.items() if k not in drop} == {k: v for k, v in second.items() if k not in drop}
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_training_step_fed_by_the_loader(token_dir):
    """one forward + backward of the fused model on a loader batch with its own num_valid: finite, and the loss of
    the same step fed with the mirror's tensors bit for bit (the inputs are the same bits; the forward has no
    atomics), the gradients up to the order of the atomic sums (one bf16 rounding, 2^-8, of each element)"""
    model, flat = _model(seed=2)
    model.train()
    with _loader(token_dir, 8, dev0, seed=9) as gpu, _loader(token_dir, 8, "cpu", seed=9) as cpu:
        gpu.seek(2)
        cpu.seek(2)
        batch, nv, idx = gpu.next()
        mirror, nv_c, idx_c = cpu.next()
    assert nv == nv_c and nv != 8 * PRED and torch.equal(idx, idx_c)
    losses, grads = [], []
    for b in (batch, tuple(t.to(dev) for t in mirror)):
        assert model.fused_ok(b[0])
        model._step = 5  # the same dropout seeds for both
        flat.zero_grad()
        loss = model(*b, num_valid=nv)
        loss.backward()
        torch.cuda.synchronize()
        losses.append(loss.detach().float().clone())
        grads.append(torch.cat([g.grad.float().reshape(-1) for g in flat]).clone())
    e = _rel(grads[0], grads[1])
    print("[bert loader step] num_valid %d of %d slots, loss %.6f / %.6f, grad rel diff %.3e, |grad| %.4f" % (
        nv, 8 * PRED, losses[0].item(), losses[1].item(), e, grads[1].norm().item()))
    assert torch.isfinite(losses[0]).all() and torch.isfinite(grads[0]).all() and grads[0].norm() > 0
    assert torch.equal(losses[0], losses[1])
    assert e <= 2.0 ** -8
    # the denominator is the loader's count: all slots as the denominator gives another loss
    with torch.no_grad():
        model._step = 5
        other = model(*batch)
    assert not torch.equal(other.float(), losses[0])
