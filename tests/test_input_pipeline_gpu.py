"""The input pipeline on the GPU: the crop/resize/normalize kernel against its exact PyTorch mirror (bf16 bits),
where its loops repeat and where its paths change; the prefetch ring under a consumer that never synchronises;
and ``resnet50_train.py --tiny --data_dir`` run and resumed on cuda:0."""
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import dtg  # noqa: F401
from dtg.data import DeviceLoader, ShardedSampler, synthetic_image_set, train_params, write_image_shards
from dtg.ops.augment import crop_resize_norm, crop_resize_norm_ref, norm_constants

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H5, W5 = 37, 53  # W * 3 = 159: source rows are not even 2-byte aligned
ROWS5 = [(0, 0, 53, 37, 0),    # full image
         (0, 0, 53, 37, 1),    # full image, flipped
         (52, 36, 1, 1, 0),    # the 1x1 crop at (36, 52)
         (0, 0, 8, 8, 0),      # 8x8 at the origin: upscales
         (36, 28, 17, 9, 1)]   # flipped, touches both far edges


def dev():
    return torch.device("cuda", 0)


def raw5():
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, 256, (5, H5, W5, 3), dtype=torch.uint8, generator=g)


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def consts():
    return norm_constants()


@pytest.fixture(scope="module")
def ref5():
    """The mirror's result for the five rows, computed once on the CPU per S and shared."""
    raw, params = raw5(), torch.tensor(ROWS5, dtype=torch.int32)
    scale, shift = consts()
    return {S: crop_resize_norm_ref(raw, params, S, scale, shift) for S in (32, 20)}


@pytest.mark.parametrize("S", [32, 20])  # 32: 16-byte vector stores; 20: the scalar tail path
def test_kernel_equals_mirror_bits(ref5, S):
    scale, shift = consts()
    raw, params = raw5().to(dev()), torch.tensor(ROWS5, dtype=torch.int32, device=dev())
    y = crop_resize_norm(raw, params, S, scale, shift)
    assert y.shape == (5, 3, S, S) and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(bits(y), bits(ref5[S]))
    y2 = crop_resize_norm(raw, params, S, scale, shift)  # determinism: two launches, equal bits
    assert torch.equal(bits(y), bits(y2))
    # a host parameter table is validated by the wrapper and then taken to the device
    y3 = crop_resize_norm(raw, torch.tensor(ROWS5, dtype=torch.int32), S, scale, shift)
    assert torch.equal(bits(y), bits(y3))


def test_grid_stride_repeats():
    """_grid=2 on [9, 16, 16, 3] -> S = 8: 18 row groups over 2 workgroups, so the item loop runs 9 times."""
    g = torch.Generator().manual_seed(9)
    raw = torch.randint(0, 256, (9, 16, 16, 3), dtype=torch.uint8, generator=g)
    params = torch.from_numpy(train_params(np.arange(9), 0, 1, 16, 16))
    params[0] = torch.tensor([0, 0, 16, 16, 1], dtype=torch.int32)
    scale, shift = consts()
    ref = crop_resize_norm_ref(raw, params, 8, scale, shift)
    for grid in (2, None):
        y = crop_resize_norm(raw.to(dev()), params.to(dev()), 8, scale, shift, _grid=grid)
        assert torch.equal(bits(y), bits(ref)), grid


@pytest.mark.parametrize("N,H,W,S,rows", [
    # a 1200-byte source segment: the staging loop of a wave runs twice (64 lanes x 16 bytes a turn); S = 6 is
    # not a multiple of the 4 rows of a workgroup, so the last row group has dead waves
    (2, 5, 403, 6, [(1, 0, 400, 5, 0), (3, 1, 400, 3, 1)]),
    # S = 520 > 512: the 8-pixel output loop of a lane runs twice
    (1, 9, 11, 520, [(2, 1, 7, 8, 1)]),
    # S = 70: the scalar path's loop runs twice; a downscale by more than 2
    (2, 150, 161, 70, [(0, 0, 161, 150, 0), (5, 3, 150, 147, 1)]),
])
def test_inner_loops_repeat(N, H, W, S, rows):
    g = torch.Generator().manual_seed(N * 1000 + W)
    raw = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g)
    params = torch.tensor(rows, dtype=torch.int32)
    scale, shift = consts()
    ref = crop_resize_norm_ref(raw, params, S, scale, shift)
    y = crop_resize_norm(raw.to(dev()), params.to(dev()), S, scale, shift)
    assert torch.equal(bits(y), bits(ref))


def test_unaligned_raw_view_and_first_last_rows():
    """raw is a view one byte into a buffer, so no source segment is 16-byte aligned and the aligned vector around
    the first and the last bytes of the tensor is not wholly inside it (the guarded byte path)."""
    g = torch.Generator().manual_seed(3)
    n = 2 * 6 * 7 * 3
    store = torch.randint(0, 256, (n + 1,), dtype=torch.uint8, generator=g)
    raw_cpu = store[1:].view(2, 6, 7, 3)
    params = torch.tensor([(0, 0, 7, 6, 0), (0, 0, 7, 6, 1)], dtype=torch.int32)
    scale, shift = consts()
    ref = crop_resize_norm_ref(raw_cpu, params, 8, scale, shift)
    raw = store.to(dev())[1:].view(2, 6, 7, 3)
    assert raw.data_ptr() % 16 == 1
    y = crop_resize_norm(raw, params.to(dev()), 8, scale, shift)
    assert torch.equal(bits(y), bits(ref))


def test_kernel_clamps_a_bad_device_table():
    """A device table is not validated on the host; whatever it holds, the kernel clamps every coordinate into the
    image, exactly as the mirror does."""
    raw = raw5()[:4]
    bad = torch.tensor([(-5, -7, 100, 100, 1), (60, 40, 3, 3, 0), (10, 10, 0, -2, 7), (50, 30, 2 ** 30, 2 ** 30, 0)],
                       dtype=torch.int32)
    scale, shift = consts()
    p64 = bad.to(torch.int64)
    x0 = p64[:, 0].clamp(0, W5 - 1)
    y0 = p64[:, 1].clamp(0, H5 - 1)
    fixed = torch.stack([x0, y0, torch.minimum(p64[:, 2].clamp(min=1), W5 - x0),
                         torch.minimum(p64[:, 3].clamp(min=1), H5 - y0), (p64[:, 4] != 0).long()], 1).to(torch.int32)
    ref = crop_resize_norm_ref(raw, fixed, 16, scale, shift)  # valid rows: passes the host validation
    y = crop_resize_norm(raw.to(dev()), bad.to(dev()), 16, scale, shift)
    assert torch.equal(bits(y), bits(ref))


@pytest.mark.parametrize("S,off", [(32, 64), (20, 64), (32, 3)])  # off = 3 elements: out is not 16-byte aligned
def test_out_view_leaves_its_surroundings(ref5, S, off):
    scale, shift = consts()
    n = 5 * S * S * 3
    buf = torch.full((off + n + 64,), -7.0, dtype=torch.bfloat16, device=dev())
    out = buf[off:off + n].view(5, S, S, 3)
    got = crop_resize_norm(raw5().to(dev()), torch.tensor(ROWS5, dtype=torch.int32, device=dev()), S, scale, shift,
                           out=out)
    assert got is out
    assert torch.equal(bits(out), bits(ref5[S].permute(0, 2, 3, 1)))
    assert (buf[:off] == -7.0).all() and (buf[off + n:] == -7.0).all()


def test_ring_reuse_with_a_consumer_that_never_synchronises(tmp_path):
    images, labels = synthetic_image_set(50, size=24, classes=10, seed=2)
    write_image_shards(str(tmp_path), images, labels, per_shard=20)
    S, batch = 16, 8
    loader = DeviceLoader(str(tmp_path), batch, S, dev(), seed=6, depth=2)
    a = torch.randn(8192, 8192, device=dev(), dtype=torch.bfloat16)
    kept = []
    for _ in range(13):  # 6 steps per epoch: two epoch boundaries; 13 batches through 2 slots
        kept.append(loader.next())
        a @ a  # keeps the stream busy, so the producer runs ahead of the kernels that read its slots
    torch.cuda.synchronize()
    samp = ShardedSampler(50, batch, seed=6)
    for step, (x, y, i) in enumerate(kept):
        epoch, idx = samp.at(step)
        assert torch.equal(i, torch.from_numpy(idx)), step
        assert torch.equal(y.cpu(), torch.from_numpy(labels[idx])), step
        p = torch.from_numpy(train_params(idx, epoch, 6, 24, 24))
        ref = crop_resize_norm_ref(torch.from_numpy(images[idx]), p, S, loader.scale, loader.shift)
        assert x.is_cuda and x.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(bits(x), bits(ref)), step  # a slot overwritten before its kernel ran shows up here
    c = loader.counters()
    assert c["batches"] == 13 and c["waits"] <= 13 and c["gather_ms"] > 0
    loader.close()
    assert loader._thread is None
    assert not [t for t in threading.enumerate() if t.name == "dtg-data-producer"]


def test_ring_seek_with_a_consumer_that_never_synchronises(tmp_path):
    """3 batches through 2 slots, seek(1) while their kernels are still queued behind the matmuls, 4 more: a ring
    that forgot a slot's consumed event at the seek would refill it before its kernel ran"""
    images, labels = synthetic_image_set(50, size=24, classes=10, seed=2)
    write_image_shards(str(tmp_path), images, labels, per_shard=20)
    S, batch = 16, 8
    a = torch.randn(8192, 8192, device=dev(), dtype=torch.bfloat16)
    kept = []
    with DeviceLoader(str(tmp_path), batch, S, dev(), seed=6, depth=2) as loader:
        for n in (3, 4):
            for _ in range(n):
                a @ a  # keeps the stream busy in front of every augmentation launch
                kept.append(loader.next())
            if n == 3:
                loader.seek(1)  # no synchronise before or after
        torch.cuda.synchronize()
        assert loader.step == 5 and loader.counters()["batches"] == 7
    samp = ShardedSampler(50, batch, seed=6)
    for step, (x, y, i) in zip((0, 1, 2, 1, 2, 3, 4), kept):
        epoch, idx = samp.at(step)
        assert torch.equal(i, torch.from_numpy(idx)), step
        assert torch.equal(y.cpu(), torch.from_numpy(labels[idx])), step
        p = torch.from_numpy(train_params(idx, epoch, 6, 24, 24))
        ref = crop_resize_norm_ref(torch.from_numpy(images[idx]), p, S, loader.scale, loader.shift)
        assert torch.equal(bits(x), bits(ref)), step


def test_example_runs_and_resumes_on_data(tmp_path):
    data, ck = str(tmp_path / "data"), str(tmp_path / "ck")
    images, labels = synthetic_image_set(100, size=40, classes=10, seed=1)
    write_image_shards(data, images, labels, per_shard=64)
    script = os.path.join(ROOT, "examples", "ResNet50", "resnet50_train.py")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DTG_FAULT"):
        env.pop(k, None)

    def launch(last):
        cmd = [sys.executable, script, "--tiny", "--data_dir", data, "--batch", "8", "--steps", str(last),
               "--log_every", "1", "--ckpt_dir", ck]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
        assert r.returncode == 0, r.stdout + r.stderr[-3000:]
        losses = [float(v) for v in re.findall(r"step \d+ loss (\S+)", r.stdout)]
        assert losses and all(np.isfinite(losses)), r.stdout
        return r.stdout, losses

    out1, l1 = launch(4)
    assert "done at global step 4" in out1 and len(l1) == 4 and "loader: batches" in out1
    out2, l2 = launch(6)
    assert "resumed from" in out2 and "(global step 4)" in out2 and "done at global step 6" in out2, out2
    assert len(l2) == 2
