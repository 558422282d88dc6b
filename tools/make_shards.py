#!/usr/bin/env python3
"""Write dtg record shards (dtg/data/records.py) for an image set.

    python tools/make_shards.py --from_npy images.npy labels.npy --out DIR --per_shard K
    python tools/make_shards.py --synthetic N --size 64 --classes 10 --out DIR [--seed 0] [--per_shard K]

--from_npy converts a uint8 [n, H, W, 3] array and its [n] labels (already decoded and resized to one size: JPEG
decoding is not part of this project).  --synthetic writes a learnable generated set -- class prototypes plus
noise, drawn from a seed -- for machines with no data set.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dtg  # noqa: E402,F401
from dtg.data import ShardSet, synthetic_image_set, write_image_shards  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--from_npy", nargs=2, metavar=("IMAGES", "LABELS"))
    src.add_argument("--synthetic", type=int, metavar="N")
    ap.add_argument("--out", required=True)
    ap.add_argument("--per_shard", type=int, default=4096)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    if a.from_npy:
        images, labels = np.load(a.from_npy[0], mmap_mode="r"), np.load(a.from_npy[1])
    else:
        images, labels = synthetic_image_set(a.synthetic, a.size, a.classes, a.seed)
    paths = write_image_shards(a.out, images, labels, a.per_shard)
    s = ShardSet(a.out)  # reopen: sizes and specs are checked
    print("wrote %d records in %d shard(s) to %s: %s" % (len(s), len(paths), a.out, s.fields))


if __name__ == "__main__":
    main()
