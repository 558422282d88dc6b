#!/usr/bin/env python3
"""Write dtg record shards (dtg/data/records.py) for an image set or a token set.

    python tools/make_shards.py --from_npy images.npy labels.npy --out DIR --per_shard K
    python tools/make_shards.py --synthetic N --size 64 --classes 10 --out DIR [--seed 0] [--per_shard K]
    python tools/make_shards.py --synthetic_tokens N --seq 128 --vocab 30528 --out DIR [--seed 0] [--strides 1 2 3 5]
    python tools/make_shards.py --from_npy input_ids.npy a_len.npy length.npy next_sentence_label.npy --out DIR
                                [--pad_id 0 --cls_id 101 --sep_id 102 --mask_id 103 --vocab_lo 999 --vocab_hi 30522]

--from_npy with two files converts a uint8 [n, H, W, 3] array and its [n] labels (already decoded and resized to one
size: JPEG decoding is not part of this project); with four files the token fields of BERT pre-training records
(int32 [n, S] ids laid out [CLS] A.. [SEP] B.. [SEP] [PAD].., the two lengths, the pair label: tokenisation is not
part of this project).  --synthetic and --synthetic_tokens write learnable generated sets, drawn from a seed, for
machines with no data set.  A token set also gets tokens.json, the ids its loader masks with.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dtg  # noqa: E402,F401
from dtg.data import (ShardSet, synthetic_image_set, synthetic_token_set, write_image_shards,  # noqa: E402
                      write_token_meta, write_token_shards, BERT_UNCASED)
from dtg.data.synthetic import TOKEN_FIELDS  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--from_npy", nargs="+", metavar="NPY", help="IMAGES LABELS, or the four token fields")
    src.add_argument("--synthetic", type=int, metavar="N")
    src.add_argument("--synthetic_tokens", type=int, metavar="N")
    ap.add_argument("--out", required=True)
    ap.add_argument("--per_shard", type=int, default=4096)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seq", type=int, default=128, help="--synthetic_tokens: sequence length S")
    ap.add_argument("--vocab", type=int, default=512, help="--synthetic_tokens: words are drawn from [4, vocab)")
    ap.add_argument("--strides", type=int, nargs="+", default=[1, 2, 3, 5],
                    help="--synthetic_tokens: the progressions' strides (0 alone: the easiest set)")
    for k, v in BERT_UNCASED.items():
        ap.add_argument("--" + k, type=int, default=None, help="token sets: default %d (--from_npy)" % v)
    a = ap.parse_args(argv)
    tokens = None
    if a.synthetic_tokens is not None:
        meta = {"pad_id": 0, "cls_id": 1, "sep_id": 2, "mask_id": 3, "vocab_lo": 4, "vocab_hi": a.vocab}
        tokens = synthetic_token_set(a.synthetic_tokens, a.seq, meta["vocab_lo"], meta["vocab_hi"], a.seed,
                                     meta["pad_id"], meta["cls_id"], meta["sep_id"], strides=tuple(a.strides))
    elif a.from_npy and len(a.from_npy) == 4:
        meta = {k: v if getattr(a, k) is None else getattr(a, k) for k, v in BERT_UNCASED.items()}
        tokens = {name: np.load(path).astype(dt) for (name, dt), path in zip(TOKEN_FIELDS, a.from_npy)}
    elif a.from_npy and len(a.from_npy) != 2:
        ap.error("--from_npy takes IMAGES LABELS or INPUT_IDS A_LEN LENGTH NEXT_SENTENCE_LABEL")
    if tokens is not None:
        paths = write_token_shards(a.out, tokens, a.per_shard)
        write_token_meta(a.out, **meta)
    else:
        if a.from_npy:
            images, labels = np.load(a.from_npy[0], mmap_mode="r"), np.load(a.from_npy[1])
        else:
            images, labels = synthetic_image_set(a.synthetic, a.size, a.classes, a.seed)
        paths = write_image_shards(a.out, images, labels, a.per_shard)
    s = ShardSet(a.out)  # reopen: sizes and specs are checked
    print("wrote %d records in %d shard(s) to %s: %s" % (len(s), len(paths), a.out, s.fields))


if __name__ == "__main__":
    main()
