"""Learnable generated sets, drawn from a seed, so the examples and the tests run on a machine with no data set: an
image set (class prototypes + noise, as models/mnist.py::synthetic_mnist) and a token set for BERT pre-training
(arithmetic progressions: a masked token follows from its neighbours, the pair label from the two segments)."""
import os

import numpy as np

from .records import SUFFIX, write_shard


def synthetic_image_set(n, size=64, classes=10, seed=0, noise=0.25):
    """-> (images uint8 [n, size, size, 3], labels int64 [n]).  Each class has one smooth random prototype (a coarse
    8 x 8 x 3 grid blown up to size x size); a sample is its class prototype plus pixel noise."""
    proto_rng = np.random.default_rng(1234)  # the classes are the same for every seed: seeds give new samples
    coarse = proto_rng.random((classes, 8, 8, 3)).astype(np.float32)
    rep = -(-size // 8)
    protos = np.repeat(np.repeat(coarse, rep, axis=1), rep, axis=2)[:, :size, :size]
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, classes, size=n, dtype=np.int64)
    images = np.empty((n, size, size, 3), dtype=np.uint8)
    for lo in range(0, n, 128):  # bounded temporaries for large sets
        hi = min(n, lo + 128)
        eps = rng.standard_normal((hi - lo, size, size, 3), dtype=np.float32)
        x = protos[labels[lo:hi]] + np.float32(noise) * eps
        images[lo:hi] = np.clip(np.rint(x * 255.0), 0, 255).astype(np.uint8)
    return images, labels


def write_image_shards(out_dir, images, labels, per_shard):
    """images uint8 [n, H, W, 3], labels [n] -> out_dir/shard-00000.dtgrec, ...; returns the paths."""
    images, labels = np.asarray(images), np.asarray(labels).astype(np.int64)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3 or labels.shape != images.shape[:1]:
        raise ValueError("images must be uint8 [n, H, W, 3] and labels [n]")
    if per_shard < 1:
        raise ValueError("per_shard >= 1 required")
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for k, lo in enumerate(range(0, len(images), per_shard)):
        paths.append(write_shard(os.path.join(out_dir, "shard-%05d%s" % (k, SUFFIX)),
                                 image=images[lo:lo + per_shard], label=labels[lo:lo + per_shard]))
    return paths


# ---- token records (BERT pre-training) ------------------------------------------------------------------------------
TOKEN_FIELDS = (("input_ids", "int32"), ("a_len", "int32"), ("length", "int32"), ("next_sentence_label", "int64"))
TOKEN_STRIDES = (1, 2, 3, 5)


def synthetic_token_set(n, seq=128, vocab_lo=4, vocab_hi=512, seed=0, pad_id=0, cls_id=1, sep_id=2, min_len=8,
                        strides=TOKEN_STRIDES):
    """A learnable generated token set -> {"input_ids" int32 [n, seq], "a_len" int32 [n], "length" int32 [n],
    "next_sentence_label" int64 [n]}, rows laid out ``[CLS] A.. [SEP] B.. [SEP] [PAD]..``.

    Segment A is an arithmetic progression over the word range ``[vocab_lo, vocab_hi)`` (hashed start, stride from
    ``strides``; stride 0 repeats one word, the member of the family a 2-layer model learns within a few hundred
    steps); segment B continues it (label 0) or is an unrelated progression (label 1).  Lengths run from ``min_len``
    to ``seq`` (one record in eight is full).  A masked token follows from its neighbours and the pair label from
    the two segments, so a falling loss means something.  Every value is a hash of (seed, record index)."""
    from .sampler import hash32
    R = vocab_hi - vocab_lo
    if not (5 <= min_len <= seq and R >= 8 and n >= 1):
        raise ValueError("5 <= min_len <= seq, vocab_hi - vocab_lo >= 8 and n >= 1 required")
    if len({pad_id, cls_id, sep_id}) != 3 or any(vocab_lo <= s < vocab_hi for s in (pad_id, cls_id, sep_id)):
        raise ValueError("pad, cls and sep ids must differ and lie outside [vocab_lo, vocab_hi)")
    i = np.arange(n, dtype=np.int64)
    st = np.asarray(strides, dtype=np.int64)
    if st.ndim != 1 or st.size < 1 or (st < 0).any():
        raise ValueError("strides: a non-empty list of non-negative integers required")

    def h(k):
        return hash32(seed, i, k).astype(np.int64)

    length = np.where(h(0) % 8 == 0, seq, min_len + h(1) % (seq - min_len + 1))
    words = length - 3                                  # >= 2: both segments hold a word
    la = 1 + h(2) % (words - 1)
    a_len = la + 2                                      # [CLS] A.. [SEP]
    label = h(3) & 1
    start_a, stride_a = h(4) % R, st[h(5) % st.size]
    start_b = np.where(label == 0, start_a + la * stride_a, h(6)) % R
    stride_b = np.where(label == 0, stride_a, st[h(7) % st.size])
    j = np.arange(seq, dtype=np.int64)[None, :]
    la_, al_, n_ = la[:, None], a_len[:, None], length[:, None]
    tok_a = vocab_lo + (start_a[:, None] + (j - 1) * stride_a[:, None]) % R
    tok_b = vocab_lo + (start_b[:, None] + (j - al_) * stride_b[:, None]) % R
    ids = np.where(j <= la_, tok_a, tok_b)
    ids = np.where((j == al_ - 1) | (j == n_ - 1), sep_id, ids)
    ids = np.where(j == 0, cls_id, ids)
    ids = np.where(j >= n_, pad_id, ids)
    return {"input_ids": ids.astype(np.int32), "a_len": a_len.astype(np.int32), "length": length.astype(np.int32),
            "next_sentence_label": label.astype(np.int64)}


def check_token_fields(fields):
    """Validate the four token fields (arrays with a leading record dimension): dtypes, shapes and
    ``1 <= a_len <= length <= S``."""
    ids = np.asarray(fields["input_ids"])
    if ids.ndim != 2 or ids.dtype != np.int32:
        raise ValueError("input_ids must be int32 [n, S]")
    n, S = ids.shape
    for name, dt in TOKEN_FIELDS[1:]:
        a = np.asarray(fields[name])
        if a.shape != (n,) or a.dtype != np.dtype(dt):
            raise ValueError("%s must be %s [n]" % (name, dt))
    a, m = np.asarray(fields["a_len"]), np.asarray(fields["length"])
    if n and not ((1 <= a) & (a <= m) & (m <= S)).all():
        raise ValueError("1 <= a_len <= length <= S required in every record")


def write_token_shards(out_dir, fields, per_shard):
    """The four token fields -> out_dir/shard-00000.dtgrec, ...; returns the paths."""
    check_token_fields(fields)
    if per_shard < 1:
        raise ValueError("per_shard >= 1 required")
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for k, lo in enumerate(range(0, len(fields["input_ids"]), per_shard)):
        paths.append(write_shard(os.path.join(out_dir, "shard-%05d%s" % (k, SUFFIX)),
                                 **{name: np.asarray(fields[name])[lo:lo + per_shard] for name, _ in TOKEN_FIELDS}))
    return paths
