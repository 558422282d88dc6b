"""The token loader: ``ring.py``'s prefetch ring for BERT pre-training records (``input_ids`` int32 [S], ``a_len``
int32, ``length`` int32, ``next_sentence_label`` int64), ending in one masking launch per batch.

What it adds to the ring: a slot of the four fields plus the record indices; a host fill that gathers them,
validates the lengths and counts the step's predictions (``ops/mlm.py::count_valid`` on the pinned ids: no device
read); and ``mlm_mask`` as the launch of ``next()`` (on the CPU its PyTorch mirror).

The masks are a pure function of (seed, epoch, record index).  Training takes the step's epoch from the sampler, so
every epoch masks a record anew; evaluation takes epoch 0 and ``eval_seed``, so every evaluation of a set sees the
same masks.

``pack=True`` adds the batch's ``ops/seqpack.py::SeqPack`` to what ``next()`` returns, for a model that runs without
padding: one ``seq_offsets`` launch on the slot's device lengths, the host lengths copied from the pinned slot (so
``T`` is a Python int with no device read, like ``num_valid``).
"""
import json
import os

import numpy as np
import torch

from ..ops.mlm import MAX_SEQ, count_valid, mlm_mask
from ..ops.seqpack import SeqPack
from .ring import FeedHook, PrefetchRing

META_FILE = "tokens.json"
# the ids of the uncased BERT vocabulary: [PAD] 0, [CLS] 101, [SEP] 102, [MASK] 103, words from 999
BERT_UNCASED = {"pad_id": 0, "cls_id": 101, "sep_id": 102, "mask_id": 103, "vocab_lo": 999, "vocab_hi": 30522}


def write_token_meta(directory, **ids):
    """The token ids a set was written with -> ``directory/tokens.json`` (settings only)."""
    meta = {k: int(ids[k]) for k in ("pad_id", "cls_id", "sep_id", "mask_id", "vocab_lo", "vocab_hi")}
    with open(os.path.join(directory, META_FILE), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    return meta


def read_token_meta(directory):
    """-> the dict of ``write_token_meta``; BERT's uncased ids when the set has no tokens.json."""
    path = os.path.join(directory, META_FILE)
    if not os.path.exists(path):
        return dict(BERT_UNCASED)
    with open(path) as f:
        return {k: int(v) for k, v in json.load(f).items()}


def masking_args(meta):
    """tokens.json -> the TokenLoader keywords it determines."""
    return dict(mask_id=meta["mask_id"], vocab_lo=meta["vocab_lo"], vocab_hi=meta["vocab_hi"],
                special_ids=(meta["pad_id"], meta["cls_id"], meta["sep_id"], meta["mask_id"]))


class TokenLoader(PrefetchRing):
    _thread_name = "dtg-token-producer"

    def __init__(self, shards, batch, device, world=1, rank=0, seed=0, train=True, depth=3, P=20, mask_per_mille=150,
                 mask_id=BERT_UNCASED["mask_id"], vocab_lo=BERT_UNCASED["vocab_lo"], vocab_hi=BERT_UNCASED["vocab_hi"],
                 special_ids=(0, 101, 102, 103), drop_last=True, eval_seed=0, threads=2, pack=False):
        """drop_last=False (evaluation only, ``train=False``): one pass of ``steps_per_epoch`` steps visits every
        record exactly once over the ranks (EvalSampler); the rows that pad the last batches repeat record 0, are
        copied unmasked with every MLM label -1, and carry ``nsp_label`` -1.  pack=True: ``next()`` returns a fourth
        item, the batch's ``SeqPack``."""
        self.P = int(P)
        self.pack = bool(pack)
        self.seed = int(seed) if train else int(eval_seed)
        self.mask = dict(P=self.P, mask_per_mille=int(mask_per_mille), mask_id=int(mask_id), vocab_lo=int(vocab_lo),
                         vocab_hi=int(vocab_hi), special_ids=tuple(int(s) for s in special_ids))
        super().__init__(shards, batch, device, world, rank, seed, train, depth, threads, drop_last)

    def _layout(self):
        fields = self.shards.fields
        dt, shape = fields.get("input_ids", (None, None))
        if dt != "int32" or len(shape) != 1 or not 1 <= shape[0] <= MAX_SEQ:
            raise ValueError("field 'input_ids' must be int32 [S], 1 <= S <= %d, got %s %s" % (MAX_SEQ, dt, shape))
        for name, want in (("a_len", "int32"), ("length", "int32"), ("next_sentence_label", "int64")):
            if fields.get(name) != (want, ()):
                raise ValueError("field %r must be %s []" % (name, want))
        self.S = shape[0]
        b = (self.batch,)  # ids, a_len, length, nsp, index
        return [((self.batch, self.S), torch.int32), (b, torch.int32), (b, torch.int32), (b, torch.int64),
                (b, torch.int64)]

    def _host_fill(self, slot, epoch, idx, valid):
        ids, a_len, length, nsp, index = slot.host
        self._gather_rows(ids, "input_ids", idx, self.threads)
        self._gather_rows(a_len, "a_len", idx)
        self._gather_rows(length, "length", idx)
        self._gather_rows(nsp, "next_sentence_label", idx)
        a, n = a_len.numpy(), length.numpy()
        if not ((1 <= a) & (a <= n) & (n <= self.S)).all():
            bad = int(np.flatnonzero(~((1 <= a) & (a <= n) & (n <= self.S)))[0])
            raise ValueError("record %d: 1 <= a_len <= length <= %d required, got a_len %d, length %d" % (
                idx[bad], self.S, a[bad], n[bad]))
        if valid < len(idx):
            nsp[valid:] = -1  # padding rows: ignored by the loss and the metrics
        index.copy_(torch.from_numpy(idx))
        slot.epoch = epoch if self.train else 0
        slot.valid = valid
        slot.num_valid = max(1, count_valid(ids.numpy(), n, self.P, self.mask["mask_per_mille"],
                                            self.mask["special_ids"], valid))

    def _consume(self, slot, tensors):
        """-> ((ids, token_types, attention_mask [batch, S], mlm_positions, mlm_labels [batch, P], nsp_labels
        [batch]) int64 on the device, num_valid: the Python int ``max(1, number of mlm_labels >= 0)`` computed on the
        host, indices int64 [batch] on the host); with ``pack=True`` also the batch's SeqPack (its lengths are the
        row sums of attention_mask; nothing in it aliases the slot)."""
        ids, a_len, length, nsp, index = tensors
        out = mlm_mask(ids, a_len, length, index, **self.mask, seed=self.seed, epoch=slot.epoch,
                       valid_rows=slot.valid)
        res = (*out, nsp.clone()), slot.num_valid, slot.host[4].clone()
        if self.pack:
            res += (SeqPack.from_lengths(length.clone(), slot.host[2].numpy(), self.S),)
        return res


class TokenFeedHook(FeedHook):
    """``ring.py::FeedHook`` for the six BERT placeholders and a ``TokenLoader``.  ``set_num_valid(n)`` is called
    with the fed batch's prediction count before every run, for the model's loss denominator; ``set_seq_pack(pack)``
    likewise with the batch's SeqPack (a ``TokenLoader(pack=True)``), e.g. ``model.set_seq_pack``."""

    def __init__(self, loader, placeholders, global_step, set_num_valid=None, set_seq_pack=None):
        if len(placeholders) != 6:
            raise ValueError("six placeholders required: ids, token types, attention mask, positions, labels, nsp")
        super().__init__(loader, global_step)
        if set_seq_pack is not None and not getattr(loader, "pack", False):
            raise ValueError("set_seq_pack needs a TokenLoader(pack=True)")
        self._ph, self._set, self._set_pack = list(placeholders), set_num_valid, set_seq_pack

    def _feed(self, batch):
        if self._set is not None:
            self._set(batch[1])
        if self._set_pack is not None:
            self._set_pack(batch[3])
        return dict(zip(self._ph, batch[0]))
