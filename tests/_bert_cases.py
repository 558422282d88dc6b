"""Shared by test_bert_data_cpu.py and test_bert_data_gpu.py: token rows laid out as the records are, and the masking
rule of ops/mlm.py written once more per row in pure Python integers (no numpy, no torch in the arithmetic)."""
import torch

PAD, CLS, SEP, MASK, LO, HI = 0, 1, 2, 3, 4, 1000
SPECIAL = (PAD, CLS, SEP, MASK)
IDS = dict(mask_id=MASK, vocab_lo=LO, vocab_hi=HI, special_ids=SPECIAL)
M32 = 0xFFFFFFFF


def make_rows(B, S, seed, lengths=None):
    """-> (input_ids i32 [B,S], a_len i32 [B], length i32 [B], index i64 [B]) on the CPU: ``[CLS] A.. [SEP] B.. [SEP]
    [PAD]..`` with random words.  The first rows take the lengths 0, 1 (only [CLS]), 4 (one candidate) and S where
    they fit, the others random ones; indices are large and not in order.  A length-0 row is all padding."""
    g = torch.Generator().manual_seed(seed)
    if lengths is None:
        fixed = [n for n in (0, 1, 4, S) if n <= S][:B]
        lengths = fixed + torch.randint(5, S + 1, (B - len(fixed),), generator=g).tolist() if S >= 5 else \
            (fixed + [S] * B)[:B]
    ids = torch.randint(LO, HI, (B, S), generator=g, dtype=torch.int32)
    a_len = torch.zeros(B, dtype=torch.int32)
    for b, n in enumerate(lengths):
        ids[b, n:] = PAD
        if n >= 1:
            ids[b, 0] = CLS
            a_len[b] = 1
        if n >= 4:
            a = int(torch.randint(3, n, (1,), generator=g))  # [CLS] A.. [SEP] ends at a
            ids[b, a - 1] = SEP
            ids[b, n - 1] = SEP
            a_len[b] = a
    index = torch.randint(0, 2 ** 40, (B,), generator=g, dtype=torch.int64)
    return ids, a_len, torch.tensor(lengths, dtype=torch.int32), index


def fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def hash32(*words):
    h = 0x9E3779B9
    for w in words:
        h = fmix32(h ^ (((w & M32) * 0x9E3779B1) & M32))
        h = (h * 5 + 0xE6546B64) & M32
    return fmix32(h)


def n_pred_rule(n_cand, P, per_mille):
    return 0 if n_cand == 0 else min(P, n_cand, max(1, (n_cand * per_mille + 500) // 1000))


def mask_row_python(row, a_len, length, index, *, seed, epoch, P, mask_per_mille=150, mask_id, vocab_lo, vocab_hi,
                    special_ids, masked=True, key_bits=32):
    """One row of the rule -> (ids, token_types, attention_mask, positions, labels) as lists; also returns the chosen
    positions' actions as a sixth element."""
    S = len(row)
    length, a_len = min(max(length, 0), S), min(max(a_len, 0), S)
    cand = [j for j in range(length) if row[j] not in special_ids] if masked else []
    n_pred = n_pred_rule(len(cand), P, mask_per_mille)
    keyed = sorted(((hash32(seed, epoch, index, j, 0) >> (32 - key_bits)) << 32) | j for j in cand)
    chosen = sorted(k & M32 for k in keyed[:n_pred])
    ids, actions = list(row), []
    for j in chosen:
        a = (hash32(seed, epoch, index, j, 1) * 10) >> 32
        actions.append(a)
        if a < 8:
            ids[j] = mask_id
        elif a == 9:
            ids[j] = vocab_lo + ((hash32(seed, epoch, index, j, 2) * (vocab_hi - vocab_lo)) >> 32)
    tt = [1 if a_len <= j < length else 0 for j in range(S)]
    am = [1 if j < length else 0 for j in range(S)]
    pos = chosen + [0] * (P - n_pred)
    lab = [row[j] for j in chosen] + [-1] * (P - n_pred)
    return ids, tt, am, pos, lab, actions


def mask_python(ids, a_len, length, index, valid_rows=None, **kw):
    """The whole batch through ``mask_row_python`` -> five int64 tensors."""
    B = ids.shape[0]
    vr = B if valid_rows is None else valid_rows
    rows = [mask_row_python(ids[b].tolist(), int(a_len[b]), int(length[b]), int(index[b]), masked=b < vr, **kw)[:5]
            for b in range(B)]
    return tuple(torch.tensor([r[i] for r in rows], dtype=torch.int64) for i in range(5))
