"""Checkpoint snapshot of a flat parameter group (csrc/kernels/snapshot.hip) with a CPU reference path.

``state_pack`` copies 1..4 fp32 buffers of one flat layout (a group's master and its optimizer slots) into a
checkpoint *image* in one launch; ``state_unpack`` is the inverse.  The image keeps the flat buffer's offsets but
holds every parameter in logical order, so ``image[j, off:off + numel].reshape(p.shape)`` is exactly the array a
checkpoint stores (``train/saver.py::flat_arrays``).  Alignment padding is neither read nor written.
"""
import torch

from ._native import lib

MAX_STATE_SRCS = 4
CHUNK = 2048


def _permuted(p):
    # the predicate of parallel/flat.py::_view_like
    return p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last) and not p.is_contiguous()


class SnapshotPlan:
    """The tables of one flat layout: ``rows`` (host int64 [P, 4] = offset, numel, I, RS; RS == 1 for every
    parameter that ``_view_like`` views without a permute -- a 1x1 conv included) and, on a GPU, their device copy
    and the host-built (row, chunk within row) table the kernel is launched over."""

    def __init__(self, offsets, params, numel, device):
        rows = []
        for off, p in zip(offsets, params):
            if _permuted(p):
                o, i, kh, kw = p.shape
                rows.append((int(off), p.numel(), int(i), int(kh * kw)))
            else:
                rows.append((int(off), p.numel(), 1, 1))
        self.rows = torch.tensor(rows, dtype=torch.int64).reshape(len(rows), 4)
        self.numel = int(numel)
        self.device = torch.device(device)
        self.rows_dev = self.chunks_dev = None
        if self.device.type == "cuda":
            chunks = lib().state_chunk_table(self.rows, self.numel)  # validates the rows against numel
            self.rows_dev = self.rows.to(self.device)
            self.chunks_dev = chunks.to(self.device)

    @classmethod
    def of_group(cls, g):
        return cls(g.offsets, g.params, g.numel, g.master.device)

    def new_image(self, k, pin=False, device=None):
        """A zeroed [k, numel] fp32 image (padding stays zero for ever: pack never writes it)."""
        dev = self.device if device is None else torch.device(device)
        return torch.zeros(k, self.numel, dtype=torch.float32, device=dev, pin_memory=bool(pin and dev.type == "cpu"))


def _cpu_check(bufs, image):
    if not 1 <= len(bufs) <= MAX_STATE_SRCS:
        raise RuntimeError("1..4 state buffers, got %d" % len(bufs))
    n = bufs[0].numel()
    if any(b.dtype != torch.float32 or b.numel() != n for b in bufs) or image.dtype != torch.float32:
        raise RuntimeError("state buffers must be fp32 and of one size")
    if image.numel() != len(bufs) * n:
        raise RuntimeError("image must hold %d x %d elements" % (len(bufs), n))
    return image.view(len(bufs), n)


def _cpu_rows(plan, flat_buf, img):
    """(flat-side view, image-side view) per row, element-aligned -- the copies ``_view_like`` would make."""
    for off, numel, i, rs in plan.rows.tolist():
        f, g = flat_buf[off:off + numel], img[off:off + numel]
        if rs == 1:
            yield f, g
        else:
            yield f.view(-1, rs, i).permute(0, 2, 1), g.view(-1, i, rs)


def state_pack(plan, srcs, image):
    """image[j] = srcs[j] with every parameter in logical order (padding untouched)."""
    srcs = list(srcs)
    if image.is_cuda or (srcs and srcs[0].is_cuda):
        return lib().state_pack(srcs, image, plan.rows, plan.rows_dev, plan.chunks_dev)
    img = _cpu_check(srcs, image)
    for j, s in enumerate(srcs):
        for f, g in _cpu_rows(plan, s, img[j]):
            g.copy_(f)


def state_unpack(plan, dsts, image):
    """The inverse of :func:`state_pack`: dsts[j] = image[j] in the flat (physical) order, padding untouched."""
    dsts = list(dsts)
    if image.is_cuda or (dsts and dsts[0].is_cuda):
        return lib().state_unpack(dsts, image, plan.rows, plan.rows_dev, plan.chunks_dev)
    img = _cpu_check(dsts, image)
    for j, d in enumerate(dsts):
        for f, g in _cpu_rows(plan, d, img[j]):
            f.copy_(g)
