"""BERT on data, off the GPU: the masking rule's PyTorch mirror against a per-row pure-Python implementation, its
invariants, the token loader on the CPU, BertEvaluator against a per-record reference (1 rank and 2 gloo ranks), and
``bert_train.py --tiny --data_dir --eval_dir`` / ``bert_eval.py`` end to end, with a stop/resume."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import dtg  # noqa: F401
from dtg.data import (TokenLoader, masking_args, read_token_meta, synthetic_token_set, write_token_meta,
                      write_token_shards)
from dtg.models import bert
from dtg.ops.metrics import xent_topk_ref
from dtg.ops.mlm import count_valid, mlm_mask, mlm_mask_ref
from dtg.train import BertEvaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _bert_cases import HI, IDS, LO, MASK, SPECIAL, make_rows, mask_python, mask_row_python, n_pred_rule  # noqa: E402


# ---- the rule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,P,key_bits", [(8, 1, 32), (40, 5, 32), (72, 20, 4), (130, 80, 32), (33, 3, 4)])
def test_mirror_equals_per_row_python(S, P, key_bits):
    ids, a_len, length, index = make_rows(9, S, seed=S + P)
    for valid_rows in (9, 7, 0):
        kw = dict(IDS, seed=11, epoch=3, P=P, key_bits=key_bits)
        got = mlm_mask_ref(ids, a_len, length, index, valid_rows=valid_rows, **kw)
        want = mask_python(ids, a_len, length, index, valid_rows=valid_rows, **kw)
        for name, g, w in zip(("ids", "token_types", "attention_mask", "positions", "labels"), got, want):
            assert g.dtype == torch.int64 and torch.equal(g, w), (name, valid_rows)
        assert mlm_mask(ids, a_len, length, index, valid_rows=valid_rows, **kw)[3].equal(want[3])  # the CPU path


def test_invariants():
    B, S, P = 64, 48, 6
    lengths = [0, 1, 2, 3, 4, 5, 6, S] + [None] * (B - 8)  # n_cand = 0, 0, 1, 2, 1, 2, 3, S - 3, ...
    g = torch.Generator().manual_seed(5)
    lengths = [n if n is not None else int(torch.randint(5, S + 1, (1,), generator=g)) for n in lengths]
    ids, a_len, length, index = make_rows(B, S, seed=1, lengths=lengths)
    out, tt, am, pos, lab = mlm_mask_ref(ids, a_len, length, index, seed=2, epoch=0, P=P, **IDS)
    seen = set()
    for b in range(B):
        row, n = ids[b].tolist(), lengths[b]
        n_cand = sum(1 for j in range(n) if row[j] not in SPECIAL)
        n_pred = n_pred_rule(n_cand, P, 150)
        seen.add((n_cand == 0, n_cand == 1, n_cand < P, n_pred == P))
        p, l = pos[b].tolist(), lab[b].tolist()
        assert sum(x >= 0 for x in l) == n_pred
        assert all(p[i] < p[i + 1] for i in range(n_pred - 1))  # strictly ascending, so unique
        assert all(0 <= j < n and row[j] not in SPECIAL for j in p[:n_pred])
        assert l[:n_pred] == [row[j] for j in p[:n_pred]]
        assert p[n_pred:] == [0] * (P - n_pred) and l[n_pred:] == [-1] * (P - n_pred)
        untouched = [j for j in range(S) if j not in p[:n_pred]]
        assert [out[b, j].item() for j in untouched] == [row[j] for j in untouched]
        assert tt[b].tolist() == [int(int(a_len[b]) <= j < n) for j in range(S)]
        assert am[b].tolist() == [int(j < n) for j in range(S)]
    # every branch of the count rule occurred: no candidate, one, fewer than P, and the cap P itself
    assert {(True, False, True, False), (False, True, True, False), (False, False, False, True)} <= seen
    assert n_pred_rule(0, 20, 150) == 0 and n_pred_rule(1, 20, 150) == 1 and n_pred_rule(3, 20, 150) == 1
    assert n_pred_rule(10, 20, 150) == 2 and n_pred_rule(126, 20, 150) == 19 and n_pred_rule(510, 20, 150) == 20


def test_purity():
    """a row's result depends on (seed, epoch, index) alone: not on its place in the batch, the batch's size or who
    computes it; another epoch masks anew"""
    ids, a_len, length, index = make_rows(12, 64, seed=7)
    kw = dict(IDS, seed=4, P=10)
    full = mlm_mask_ref(ids, a_len, length, index, epoch=1, **kw)
    perm = torch.randperm(12, generator=torch.Generator().manual_seed(0))
    shuffled = mlm_mask_ref(ids[perm], a_len[perm], length[perm], index[perm], epoch=1, **kw)
    for f, s in zip(full, shuffled):
        assert torch.equal(f[perm], s)
    for lo, hi in ((0, 5), (5, 12), (11, 12)):  # the parts two ranks (or a batch of one) would hold
        part = mlm_mask_ref(ids[lo:hi], a_len[lo:hi], length[lo:hi], index[lo:hi], epoch=1, **kw)
        for f, p in zip(full, part):
            assert torch.equal(f[lo:hi], p)
    other = mlm_mask_ref(ids, a_len, length, index, epoch=2, **kw)
    # rows of >= 32 tokens choose >= 4 of >= 29 candidates: two epochs agree with probability < 1 / 23 000
    differs = [(not torch.equal(full[3][b], other[3][b])) for b in range(12) if int(length[b]) >= 32]
    assert all(differs) and len(differs) >= 3


def test_ties_break_toward_the_lower_position():
    B, S, P = 32, 64, 9  # 61 candidates per row: n_pred = 9, every slot used
    ids, a_len, length, index = make_rows(B, S, seed=3, lengths=[S] * B)
    kw = dict(IDS, seed=9, epoch=0, P=P, key_bits=4)
    pos = mlm_mask_ref(ids, a_len, length, index, **kw)[3]
    from _bert_cases import hash32
    tied_rows = 0
    for b in range(B):
        row = ids[b].tolist()
        key = {j: hash32(9, 0, int(index[b]), j, 0) >> 28 for j in range(S) if row[j] not in SPECIAL}
        chosen = pos[b].tolist()
        assert len(set(chosen)) == P
        worst = max(key[j] for j in chosen)
        rest = [j for j in key if j not in chosen]
        assert all(key[j] >= worst for j in rest)
        boundary = [j for j in rest if key[j] == worst]  # tied with a chosen position, yet left out
        if boundary:
            tied_rows += 1
            assert min(boundary) > max(j for j in chosen if key[j] == worst)
    print("[mlm ties] %d of %d rows tie at the boundary with 4-bit keys" % (tied_rows, B))
    assert tied_rows > B // 2


def test_action_shares():
    """over >= 30 000 chosen positions the shares lie within 5 sigma of 0.8 / 0.1 / 0.1, sigma = sqrt(p (1 - p) / N)"""
    B, S, P = 1800, 128, 20
    ids, a_len, length, index = make_rows(B, S, seed=21, lengths=[S] * B)
    out, _, _, pos, lab = mlm_mask_ref(ids, a_len, length, index, seed=1, epoch=0, P=P, **IDS)
    used = lab >= 0
    new = out.gather(1, pos)[used]
    old = lab[used]
    N = int(used.sum())
    # actions from the hashes themselves (a random token may equal the old one, so the ids alone do not tell)
    from dtg.ops.mlm import hash32_t
    act = ((hash32_t(1, 0, index.view(B, 1), pos, 1) * 10) >> 32)[used]
    masked, kept, rand = act < 8, act == 8, act == 9
    assert (new[masked] == MASK).all() and (new[kept] == old[kept]).all()
    assert ((new[rand] >= LO) & (new[rand] < HI)).all()
    assert len(torch.unique(new[rand])) > 0.5 * min(HI - LO, int(rand.sum()))  # spread over the range
    for name, share, p in (("mask", masked, 0.8), ("keep", kept, 0.1), ("random", rand, 0.1)):
        f, sigma = share.float().mean().item(), math.sqrt(p * (1 - p) / N)
        print("[mlm actions] %s: %.5f of %d (%.2f sigma)" % (name, f, N, (f - p) / sigma))
        assert abs(f - p) <= 5 * sigma
    assert N >= 30000


# ---- the loader on the CPU --------------------------------------------------------------------------------------------
N, S, P, VOCAB = 50, 32, 5, 132
META = dict(pad_id=0, cls_id=1, sep_id=2, mask_id=3, vocab_lo=4, vocab_hi=VOCAB)


def _write_set(d, n, seed, seq=S, strides=(1, 2, 3, 5), per_shard=20):
    fields = synthetic_token_set(n, seq=seq, vocab_hi=VOCAB, seed=seed, strides=strides)
    write_token_shards(str(d), fields, per_shard)
    write_token_meta(str(d), **META)
    return fields


@pytest.fixture(scope="module")
def token_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("tokens")
    return str(d), _write_set(d, N, seed=8)


def test_generated_set(token_set):
    d, f = token_set
    ids, a, n = f["input_ids"], f["a_len"], f["length"]
    assert ids.dtype == np.int32 and ids.shape == (N, S) and read_token_meta(d) == META
    assert ((1 <= a) & (a <= n) & (n <= S)).all() and n.min() < S // 2 and n.max() == S
    assert set(f["next_sentence_label"].tolist()) == {0, 1}
    for i in range(N):
        row = ids[i].tolist()
        assert row[0] == 1 and row[a[i] - 1] == 2 and row[n[i] - 1] == 2 and all(t == 0 for t in row[n[i]:])
        words = [t for t in row[:n[i]] if t > 3]
        assert len(words) == n[i] - 3 and all(4 <= t < VOCAB for t in words)
        seg_a = row[1:a[i] - 1]
        d1 = {(y - x) % (VOCAB - 4) for x, y in zip(seg_a, seg_a[1:])}
        assert len(d1) <= 1 and d1 <= {1, 2, 3, 5}  # one stride per progression
        if f["next_sentence_label"][i] == 0 and len(seg_a) > 1:  # B continues A across [SEP]
            assert (row[a[i]] - seg_a[-1]) % (VOCAB - 4) in d1
    again = synthetic_token_set(N, seq=S, vocab_hi=VOCAB, seed=8)
    assert all(np.array_equal(f[k], again[k]) for k in f)
    with pytest.raises(ValueError):
        write_token_shards(d + "_bad", dict(f, length=f["length"] + S), 20)


def _loader(d, batch, **kw):
    return TokenLoader(d, batch, "cpu", P=P, **masking_args(META), **kw)


def test_world_ranks_read_the_global_batch(token_set):
    d, _ = token_set
    with _loader(d, 12, seed=3) as one, _loader(d, 4, world=3, rank=0, seed=3) as r0, \
            _loader(d, 4, world=3, rank=1, seed=3) as r1, _loader(d, 4, world=3, rank=2, seed=3) as r2:
        assert one.steps_per_epoch == 4
        for step in range(6):  # into the second epoch
            big, nv, idx = one.next()
            parts = [r.next() for r in (r0, r1, r2)]
            assert torch.equal(idx, torch.cat([p[2] for p in parts]))
            for i in range(6):
                assert torch.equal(big[i], torch.cat([p[0][i] for p in parts])), (step, i)
            assert nv == sum(p[1] for p in parts) == int((big[4] >= 0).sum())
            assert all(p[1] == int((p[0][4] >= 0).sum()) for p in parts)  # num_valid is the label count


def test_seek_gives_the_batch_again_and_epochs_mask_anew(token_set):
    d, f = token_set
    with _loader(d, 8, seed=5, depth=2) as loader:
        first = [loader.next() for _ in range(8)]
        assert loader.step == 8 and loader.steps_per_epoch == 6
        for k in (5, 0, 7):
            loader.seek(k)
            again = loader.next()
            assert all(torch.equal(x, y) for x, y in zip(first[k][0], again[0]))
            assert again[1] == first[k][1] and torch.equal(again[2], first[k][2])
        # the batch is the mirror of its records at the step's epoch
        (ids, tt, am, pos, lab, nsp), nv, idx = first[7]
        want = mlm_mask_ref(torch.from_numpy(f["input_ids"][idx]), torch.from_numpy(f["a_len"][idx]),
                            torch.from_numpy(f["length"][idx]), idx, seed=5, epoch=1, P=P, **masking_args(META))
        assert all(torch.equal(x, y) for x, y in zip((ids, tt, am, pos, lab), want))
        assert torch.equal(nsp, torch.from_numpy(f["next_sentence_label"][idx]))
        assert nv == count_valid(f["input_ids"][idx], f["length"][idx], P, 150, masking_args(META)["special_ids"])
        # a record seen in both epochs is masked differently in most cases
        e0 = {int(i): p for b in first[:6] for i, p in zip(b[2], b[0][3])}
        e1 = {int(i): p for b in first[6:] for i, p in zip(b[2], b[0][3])}
        both = [i for i in e1 if i in e0]
        assert len(both) >= 10 and sum(not torch.equal(e0[i], e1[i]) for i in both) > len(both) // 2


def test_seek_inside_a_full_ring_and_close(token_set):
    """depth 2 and three batches taken: both slots have been through the ring when the seek comes, and the batches
    after it are those of a fresh loader's steps 1..3 bit for bit; a closed loader holds no thread"""
    import threading
    d, _ = token_set
    with _loader(d, 8, seed=9, depth=2) as fresh:
        want = [fresh.next() for _ in range(4)]
    loader = _loader(d, 8, seed=9, depth=2)
    for k in range(3):
        assert torch.equal(loader.next()[2], want[k][2])
    loader.seek(1)
    for k in (1, 2, 3):
        tensors, nv, idx = loader.next()
        assert nv == want[k][1] and torch.equal(idx, want[k][2])
        assert all(torch.equal(x, y) for x, y in zip(tensors, want[k][0]))
    assert loader.step == 4 and loader.counters()["batches"] == 6
    loader.close()
    loader.close()
    assert loader._thread is None
    assert not [t for t in threading.enumerate() if t.name == "dtg-token-producer"]
    with pytest.raises(RuntimeError):
        loader.next()


def test_eval_pass_every_record_once_and_padding_rows(token_set):
    d, f = token_set
    with pytest.raises(ValueError):
        _loader(d, 8, train=True, drop_last=False)
    with _loader(d, 8, train=False, drop_last=False, eval_seed=77) as loader:
        assert loader.steps_per_epoch == 7
        seen, masks = [], []
        for step in range(7):
            (ids, tt, am, pos, lab, nsp), nv, idx = loader.next()
            valid = 8 if step < 6 else 2
            seen.extend(idx[:valid].tolist())
            assert (nsp[valid:] == -1).all() and (nsp[:valid] >= 0).all() and (idx[valid:] == 0).all()
            assert (lab[valid:] == -1).all() and (pos[valid:] == 0).all()
            assert torch.equal(ids[valid:], torch.from_numpy(f["input_ids"][idx[valid:]]).long())  # copied unmasked
            assert (lab[:valid, 0] >= 0).all() and nv == max(1, int((lab >= 0).sum()))
            masks.append((ids, pos, lab))
        assert seen == list(range(N))
        with pytest.raises(StopIteration):
            loader.next()
        loader.seek(0)  # every evaluation sees the same masks: epoch 0 and the evaluation seed
        for step in range(7):
            (ids, _, _, pos, lab, _), _, _ = loader.next()
            assert all(torch.equal(x, y) for x, y in zip((ids, pos, lab), masks[step]))
    with _loader(d, 8, train=False, drop_last=False, eval_seed=78) as other:
        assert not torch.equal(other.next()[0][3], masks[0][1])


def test_loader_refuses_bad_lengths(tmp_path):
    f = synthetic_token_set(20, seq=S, vocab_hi=VOCAB, seed=1)
    from dtg.data import write_shard
    bad = dict(f)
    bad["length"] = f["length"].copy()
    bad["length"][13] = S + 5
    write_shard(str(tmp_path / "shard-00000.dtgrec"), **bad)  # around the writer's own check
    with _loader(str(tmp_path), 20, train=False, drop_last=False) as loader:
        with pytest.raises(RuntimeError) as e:
            loader.next()
        assert "record 13" in str(e.value.__cause__)


# ---- BertEvaluator -----------------------------------------------------------------------------------------------------
EVAL_SEED = 12


def _tiny_model(seed=3):
    torch.manual_seed(seed)
    cfg = bert.BertConfig(vocab_size=VOCAB + 4, hidden=32, layers=2, heads=2, intermediate=64, max_position=S)
    return bert.BertForPreTraining(cfg)


@pytest.fixture(scope="module")
def eval_ref(token_set):
    """the per-record reference: one record at a time through the masking mirror, the model and the row definition"""
    d, f = token_set
    model = _tiny_model().eval()
    mlm_loss, nsp_loss, top1, top5, nsp_ok, mlm_n = [], [], 0, 0, 0, 0
    with torch.no_grad():
        for i in range(N):
            ids, tt, am, pos, lab = mlm_mask_ref(
                torch.from_numpy(f["input_ids"][i:i + 1]), torch.from_numpy(f["a_len"][i:i + 1]),
                torch.from_numpy(f["length"][i:i + 1]), torch.tensor([i]), seed=EVAL_SEED, epoch=0, P=P,
                **masking_args(META))
            ml, nl = model.pretraining_logits(ids, tt, am, pos)
            assert ml.shape == (P, VOCAB + 4) and nl.shape == (1, 2)
            l, r = xent_topk_ref(ml, lab.reshape(-1))
            keep = r >= 0
            mlm_n += int(keep.sum())
            mlm_loss.extend(l[keep].double().tolist())
            top1 += int((keep & (r < 1)).sum())
            top5 += int((keep & (r < 5)).sum())
            l, r = xent_topk_ref(nl, torch.from_numpy(f["next_sentence_label"][i:i + 1]))
            nsp_loss.append(l[0].double().item())
            nsp_ok += int(r[0] == 0)
    ref = {"n": N, "mlm_n": mlm_n, "mlm_loss": math.fsum(mlm_loss) / mlm_n, "nsp_loss": math.fsum(nsp_loss) / N,
           "top1": top1, "top5": top5, "nsp_ok": nsp_ok}
    assert 0 <= top1 <= top5 < mlm_n and 0 < nsp_ok < N and mlm_n > N
    return d, ref


# fp32 GEMMs of another batch shape may add in another order: every logit moves by a few units of 2^-24 of the terms
# it sums (at most 64 of them here), and the loss by as much; the sums themselves are fp64.  2^-17 relative is far above
# that and far below what a wrong record, mask or denominator would cost (1 / mlm_n = 0.7 %).
LOSS_RTOL = 2.0 ** -17


def _evaluate(d, batch, world=1, rank=0, model=None):
    with _loader(d, batch, world=world, rank=rank, train=False, drop_last=False, eval_seed=EVAL_SEED) as loader:
        assert loader.steps_per_epoch == math.ceil(N / (batch * world))
        return BertEvaluator(model or _tiny_model(), loader, ks=(1, 5)).run()


def _check_result(res, ref, what):
    e_mlm = abs(res["mlm_loss"] - ref["mlm_loss"]) / ref["mlm_loss"]
    e_nsp = abs(res["nsp_loss"] - ref["nsp_loss"]) / ref["nsp_loss"]
    print("[bert eval] %s: n=%d mlm_n=%d top1=%d top5=%d nsp=%d mlm_loss=%.9f (rel err %.2e) nsp_loss=%.9f (rel err "
          "%.2e) bound %.2e" % (what, res["n"], res["mlm_n"], res["mlm_top1_count"], res["mlm_top5_count"],
                                res["nsp_correct"], res["mlm_loss"], e_mlm, res["nsp_loss"], e_nsp, LOSS_RTOL))
    assert res["n"] == ref["n"] and res["mlm_n"] == ref["mlm_n"] and res["bad_labels"] == 0 and res["nonfinite"] == 0
    assert res["mlm_top1_count"] == ref["top1"] and res["mlm_top5_count"] == ref["top5"]
    assert res["nsp_correct"] == ref["nsp_ok"] and res["nsp_acc"] == ref["nsp_ok"] / N
    assert res["mlm_top1"] == ref["top1"] / ref["mlm_n"] and res["mlm_top5"] == ref["top5"] / ref["mlm_n"]
    assert e_mlm <= LOSS_RTOL and e_nsp <= LOSS_RTOL
    assert res["seconds"] > 0 and res["sequences_per_sec"] > 0


def test_bert_evaluator_equals_per_record_reference(eval_ref):
    d, ref = eval_ref
    model = _tiny_model().train()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    step = model._step
    first = _evaluate(d, 7, model=model)
    _check_result(first, ref, "1 rank x 7")
    second = _evaluate(d, 7, model=model)
    assert model.training and all(m.training for m in model.modules()) and model._step == step
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert not any(p.grad is not None for p in model.parameters())
    drop = ("seconds", "sequences_per_sec")
    assert {k: v for k, v in first.items() if k not in drop} == {k: v for k, v in second.items() if k not in drop}
    model.eval()
    _evaluate(d, 50, model=model)
    assert not model.training


def _gloo_rank(rank, world, port, d, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        import dtg  # noqa: F401
        from dtg.parallel import comm
        comm.init("gloo")
        res = _evaluate(d, 3, world, rank)
        comm.shutdown()
        q.put((rank, res))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, traceback.format_exc()))
        raise


def test_bert_evaluator_two_gloo_ranks(eval_ref):
    d, ref = eval_ref
    from _cluster import free_ports
    port = free_ports(1)[0]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_rank, args=(r, 2, port, d, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    res = dict(q.get(timeout=5) for _ in range(2))
    assert all(isinstance(v, dict) for v in res.values()), res
    for r in (0, 1):
        _check_result(res[r], ref, "2 gloo ranks x 3, rank %d" % r)
    assert res[0]["mlm_loss_sum"] == res[1]["mlm_loss_sum"] and res[0]["nsp_loss_sum"] == res[1]["nsp_loss_sum"]


def _gloo_rank_refusing_broadcasts(rank, world, port, d, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        import dtg  # noqa: F401
        import torch.distributed as dist
        from dtg.parallel import comm
        comm.init("gloo")

        def refuse(*args, **kw):
            raise AssertionError("BertEvaluator launched a broadcast")
        dist.broadcast = refuse
        model = _tiny_model()
        model.register_buffer("running", torch.full((3,), float(rank)))  # what a borrowing pass would broadcast
        res = _evaluate(d, 3, world, rank, model=model)
        assert model.running.tolist() == [float(rank)] * 3
        comm.shutdown()
        q.put((rank, res))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, traceback.format_exc()))
        raise


def test_bert_evaluator_two_gloo_ranks_launch_no_broadcast(eval_ref):
    """the pass shared with Evaluator borrows no buffers for BERT: with a floating-point buffer on the model and
    ``torch.distributed.broadcast`` made to raise, two ranks still evaluate, each with its own buffer"""
    d, ref = eval_ref
    from _cluster import free_ports
    port = free_ports(1)[0]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_rank_refusing_broadcasts, args=(r, 2, port, d, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    res = dict(q.get(timeout=5) for _ in range(2))
    assert all(isinstance(v, dict) for v in res.values()), res
    for r in (0, 1):
        _check_result(res[r], ref, "2 gloo ranks x 3, no broadcast, rank %d" % r)


def test_eval_hook_formatter():
    from dtg.train import EvalHook
    from dtg.train.evaluation import format_bert_result
    res = {"n": 50, "mlm_n": 141, "mlm_loss": 6.25, "mlm_top1": 0.5, "mlm_top5": 0.75, "nsp_loss": 0.69,
           "nsp_acc": 0.36}
    line = format_bert_result(60, res, (1, 5))
    assert line == ("eval step 60: n=50 mlm_n=141 mlm_loss=6.250000 mlm_top1=0.500000 mlm_top5=0.750000 "
                    "nsp_loss=0.690000 nsp_acc=0.360000")

    class Ev:
        ks = (1, 5)

        def run(self):
            return res

        def close(self):
            pass

    class Values:
        results = 2

    lines = []
    hook = EvalHook(Ev(), 2, "gs", log=True, formatter=lambda step, r, ks: lines.append((step, ks)) or "x")
    hook.after_run(None, Values())
    assert lines == [(2, (1, 5))] and hook.results == [(2, res)]


# ---- the examples, end to end -------------------------------------------------------------------------------------
LINE = re.compile(r"eval step (\d+): n=(\d+) mlm_n=(\d+) mlm_loss=(\d+\.\d{6}) mlm_top1=(\d\.\d{6}) "
                  r"mlm_top5=(\d\.\d{6}) nsp_loss=(\d+\.\d{6}) nsp_acc=(\d\.\d{6})")


def _clean_env():
    e = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DTG_FAULT"):
        e.pop(k, None)
    return e


def _launch(nproc, script, *args):
    from _cluster import free_ports
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(free_ports(1)[0]),
           os.path.join(ROOT, "examples", "BERT", script), *args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=_clean_env())


def test_examples_train_from_shards_then_eval_script(tmp_path):
    """2 gloo ranks train the tiny model on the generated set (stride 0: the member of the family it learns within
    a few hundred steps) and evaluate on a held-out shard; bert_eval.py prints the last line again; both losses of
    the trained model lie below those of the untrained one, measured here on the same shard"""
    train_dir, val_dir, ck = str(tmp_path / "train"), str(tmp_path / "val"), str(tmp_path / "ck")
    tools = os.path.join(ROOT, "tools", "make_shards.py")
    for out, n, seed in ((train_dir, "512", "0"), (val_dir, "60", "9")):
        r = subprocess.run([sys.executable, tools, "--synthetic_tokens", n, "--seq", "32", "--vocab", "68", "--strides",
                            "0", "--seed", seed, "--out", out, "--per_shard", "200"], capture_output=True, text=True,
                           env=_clean_env())
        assert r.returncode == 0 and "wrote %s records" % n in r.stdout, r.stdout + r.stderr
    r = _launch(2, "bert_train.py", "--tiny", "--batch", "8", "--steps", "300", "--lr", "3e-3", "--warmup", "20",
                "--save_every", "1000", "--log_every", "100", "--ckpt_dir", ck, "--data_dir", train_dir, "--eval_dir",
                val_dir, "--eval_every", "150", "--eval_batch", "7", "--max_predictions", "5")
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("eval step ")]
    print("\n".join(lines))
    assert [int(LINE.fullmatch(l).group(1)) for l in lines] == [150, 300], r.stdout
    assert "done at global step 300" in r.stdout and "loader: {'batches': 300" in r.stdout

    e = _launch(2, "bert_eval.py", "--tiny", "--batch", "7", "--ckpt_dir", ck, "--data_dir", val_dir,
                "--max_predictions", "5")
    assert e.returncode == 0, e.stdout + e.stderr[-3000:]
    got = [l for l in e.stdout.splitlines() if l.startswith("eval step ")]
    print("\n".join(got))
    assert got == lines[-1:], (got, lines)  # the same counts, the losses to the printed digits

    torch.manual_seed(1234)  # the untrained model of bert_train.py --tiny, scored here
    untrained = bert.BertForPreTraining(bert.BertConfig.tiny())
    with TokenLoader(val_dir, 7, "cpu", train=False, drop_last=False, P=5,
                     **masking_args(read_token_meta(val_dir))) as loader:
        base = BertEvaluator(untrained, loader).run()
    m = LINE.fullmatch(got[0])
    trained_mlm, trained_nsp = float(m.group(4)), float(m.group(7))
    print("[bert e2e] untrained mlm_loss %.6f nsp_loss %.6f; trained %.6f %.6f" % (
        base["mlm_loss"], base["nsp_loss"], trained_mlm, trained_nsp))
    assert int(m.group(2)) == base["n"] == 60 and int(m.group(3)) == base["mlm_n"]
    assert trained_mlm < base["mlm_loss"] and trained_nsp < base["nsp_loss"]

    none = _launch(1, "bert_eval.py", "--tiny", "--ckpt_dir", str(tmp_path / "empty"), "--data_dir", val_dir)
    assert none.returncode == 1 and "no checkpoint" in none.stderr


def test_bert_example_data_dir_resume_bit_equal(tmp_path):
    """a job stopped at step 3 and resumed to 6 ends with the bits of an uninterrupted one: the batches follow the
    restored global step"""
    data = str(tmp_path / "data")
    _write_set(data, 40, seed=1)  # 5 steps per epoch at 2 x 4: the resume crosses an epoch

    def launch(ck, last):
        r = _launch(2, "bert_train.py", "--tiny", "--batch", "4", "--steps", str(last), "--total_steps", "6",
                    "--warmup", "2", "--save_every", "100", "--log_every", "1", "--ckpt_dir", ck, "--data_dir", data,
                    "--data_seed", "4", "--max_predictions", "5")
        assert r.returncode == 0, r.stdout + r.stderr[-3000:]
        assert "done at global step %d" % last in r.stdout, r.stdout
        return r.stdout

    full, parts = str(tmp_path / "ck_full"), str(tmp_path / "ck_parts")
    whole = launch(full, 6)
    launch(parts, 3)
    out = launch(parts, 6)
    assert "resumed from" in out and "(global step 3)" in out, out
    losses = lambda text: [l for l in text.splitlines() if re.match(r"step [456] loss ", l)]  # noqa: E731
    assert len(losses(whole)) == 3 and losses(whole) == losses(out)
    ra = dtg.train.NewCheckpointReader(dtg.train.latest_checkpoint(full))
    rb = dtg.train.NewCheckpointReader(dtg.train.latest_checkpoint(parts))
    keys = sorted(ra.get_variable_to_shape_map())
    assert keys == sorted(rb.get_variable_to_shape_map()) and len(keys) > 10
    assert int(ra.get_tensor("global_step")) == int(rb.get_tensor("global_step")) == 6
    for k in keys:
        assert np.array_equal(np.asarray(ra.get_tensor(k)), np.asarray(rb.get_tensor(k))), k
