"""A learnable generated image set (class prototypes + noise, as models/mnist.py::synthetic_mnist), drawn from a
seed, so the examples and the tests run on a machine with no data set."""
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
