"""The image loader: ``ring.py``'s prefetch ring for image records, ending in one augmentation launch per batch.

What it adds to the ring: a slot of a raw-image buffer ``[batch, H, W, 3]``, a parameter table and a label buffer;
a host fill that makes and validates the step's augmentation parameters and gathers images and labels; and
``crop_resize_norm`` as the launch of ``next()`` (on the CPU its PyTorch mirror).
"""
import torch

from ..ops.augment import IMAGENET_MEAN, IMAGENET_STD, crop_resize_norm, norm_constants
from .augment_params import eval_params, train_params, validate_params
from .ring import FeedHook, PrefetchRing


class DeviceLoader(PrefetchRing):
    _thread_name = "dtg-data-producer"

    def __init__(self, shards, batch, S, device, world=1, rank=0, seed=0, train=True, depth=3, threads=4,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD, image_field="image", label_field="label",
                 dtype=torch.bfloat16, drop_last=True):
        """dtype: what ``next()`` returns the images as (the kernel writes bf16; another dtype is a cast of that,
        for fp32 CPU models).  drop_last=False (evaluation only, ``train=False``): one pass of ``steps_per_epoch``
        steps visits every record exactly once over the ranks (EvalSampler); the rows that pad the last batches
        repeat record 0 and carry label -1, which the loss and the metric kernels ignore."""
        self.S, self.seed = S, seed
        self._image, self._label, self._dtype = image_field, label_field, dtype
        super().__init__(shards, batch, device, world, rank, seed, train, depth, threads, drop_last)
        self.scale, self.shift = norm_constants(mean, std)
        self._norm = (self.scale.to(self.device), self.shift.to(self.device))

    def _layout(self):
        fields = self.shards.fields
        dt, shape = fields[self._image]
        if dt != "uint8" or len(shape) != 3 or shape[2] != 3:
            raise ValueError("field %r must be uint8 [H, W, 3], got %s %s" % (self._image, dt, shape))
        if fields[self._label] != ("int64", ()):
            raise ValueError("field %r must be int64 []" % self._label)
        self.H, self.W = shape[0], shape[1]
        return [((self.batch, self.H, self.W, 3), torch.uint8), ((self.batch, 5), torch.int32),
                ((self.batch,), torch.int64)]

    def _host_fill(self, slot, epoch, idx, valid):
        raw, params, labels = slot.host
        p = train_params(idx, epoch, self.seed, self.H, self.W) if self.train else \
            eval_params(len(idx), self.H, self.W)
        validate_params(p, self.H, self.W)
        self._gather_rows(raw, self._image, idx, self.threads)
        self._gather_rows(labels, self._label, idx)
        if valid < len(idx):
            labels[valid:] = -1  # padding rows: ignored by the loss and the metrics
        params.copy_(torch.from_numpy(p))
        slot.indices = idx

    def _consume(self, slot, tensors):
        """-> (images bf16 [batch, 3, S, S] channels_last, labels int64 [batch] on the device, indices int64 [batch]
        on the host)."""
        raw, params, labels = tensors
        images = crop_resize_norm(raw, params, self.S, *self._norm)
        if images.dtype != self._dtype:
            images = images.to(self._dtype)
        return images, labels.clone(), torch.from_numpy(slot.indices.copy())


class DataFeedHook(FeedHook):
    """``ring.py::FeedHook`` for ``images_ph`` / ``labels_ph`` and a ``DeviceLoader``."""

    def __init__(self, loader, images_ph, labels_ph, global_step):
        super().__init__(loader, global_step)
        self._x, self._y = images_ph, labels_ph

    def _feed(self, batch):
        return {self._x: batch[0], self._y: batch[1]}
