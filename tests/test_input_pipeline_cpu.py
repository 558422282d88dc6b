"""The input pipeline off the GPU: record shards, the sharded sampler, the augmentation parameters, the exact PyTorch
mirror of the crop/resize/normalize kernel, the native host gather, the loader on the CPU, and a stop/resume of
``resnet50_train.py --tiny --data_dir`` on 2 gloo ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dtg
from dtg.data import (DeviceLoader, ShardSet, ShardedSampler, eval_params, synthetic_image_set, train_params,
                      validate_params, write_image_shards, write_shard)
from dtg.ops.augment import crop_resize_norm, crop_resize_norm_ref, norm_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the five parameter rows of the GPU test (tests/test_input_pipeline_gpu.py), for raw [5, 37, 53, 3]
H5, W5 = 37, 53
ROWS5 = [(0, 0, 53, 37, 0),    # full image
         (0, 0, 53, 37, 1),    # full image, flipped
         (52, 36, 1, 1, 0),    # the 1x1 crop at (36, 52)
         (0, 0, 8, 8, 0),      # 8x8 at the origin: upscales
         (36, 28, 17, 9, 1)]   # flipped, touches both far edges


def raw5():
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, 256, (5, H5, W5, 3), dtype=torch.uint8, generator=g)


def bits(t):
    return t.contiguous().view(torch.int16)


# ---- shards --------------------------------------------------------------------------------------------------
def test_shards_round_trip_over_two_shards(tmp_path):
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (11, 7, 5, 3), dtype=np.uint8)
    lab = rng.integers(0, 10, 11).astype(np.int64)
    write_shard(str(tmp_path / "a.dtgrec"), image=img[:6], label=lab[:6])
    write_shard(str(tmp_path / "b.dtgrec"), image=img[6:], label=lab[6:])
    s = ShardSet(str(tmp_path))
    assert len(s) == 11 and s.fields == {"image": ("uint8", (7, 5, 3)), "label": ("int64", ())}
    shard, local = s.locate([0, 5, 6, 10])
    assert shard.tolist() == [0, 0, 1, 1] and local.tolist() == [0, 5, 0, 4]
    idx = [10, 0, 6, 5, 5]
    assert np.array_equal(s.take("image", idx), img[idx]) and np.array_equal(s.take("label", idx), lab[idx])
    for sh in s.shards:  # structure of arrays, every array 64-byte aligned in its (page-aligned) mapping
        assert all(a.ctypes.data % 64 == 0 for a in sh.arrays.values())
    with pytest.raises(IndexError):
        s.locate([11])


def test_shards_refuse_bad_files(tmp_path):
    img = np.zeros((4, 7, 5, 3), dtype=np.uint8)
    lab = np.arange(4, dtype=np.int64)
    (tmp_path / "good").mkdir()
    good = write_shard(str(tmp_path / "good" / "a.dtgrec"), image=img, label=lab)
    assert len(ShardSet(str(tmp_path / "good"))) == 4
    blob = open(good, "rb").read()
    for name, data in (("magic", b"NOTAREC!" + blob[8:]), ("truncated", blob[:-1]),
                       ("header_only", blob[:40])):
        d = tmp_path / name
        d.mkdir()
        (d / "a.dtgrec").write_bytes(data)
        with pytest.raises(ValueError):
            ShardSet(str(d))
    d = tmp_path / "mismatch"
    d.mkdir()
    write_shard(str(d / "a.dtgrec"), image=img, label=lab)
    write_shard(str(d / "b.dtgrec"), image=np.zeros((4, 7, 6, 3), dtype=np.uint8), label=lab)
    with pytest.raises(ValueError, match="differ"):
        ShardSet(str(d))
    with pytest.raises(ValueError):
        ShardSet(str(tmp_path / "good" / "nothing_here"))


# ---- sampler -------------------------------------------------------------------------------------------------
def test_sampler_disjoint_ranks_equal_one_big_rank():
    n, batch, world = 103, 4, 3
    ranks = [ShardedSampler(n, batch, world, r, seed=7) for r in range(world)]
    one = ShardedSampler(n, batch * world, 1, 0, seed=7)
    assert all(s.steps_per_epoch == 8 for s in ranks) and one.steps_per_epoch == 8
    seen = {0: [], 1: []}
    for step in range(16):
        parts = [s.at(step) for s in ranks]
        assert all(e == step // 8 for e, _ in parts)
        sets = [set(i.tolist()) for _, i in parts]
        assert all(len(x) == batch for x in sets) and len(set.union(*sets)) == batch * world  # disjoint
        cat = np.concatenate([i for _, i in parts])
        assert np.array_equal(cat, one.at(step)[1])
        seen[step // 8].extend(cat.tolist())
    for e in (0, 1):  # no index repeats within an epoch; the dropped tail is the last 7 of the permutation
        assert len(set(seen[e])) == len(seen[e]) == 96 and max(seen[e]) < n and min(seen[e]) >= 0
    assert seen[0] != seen[1]


def test_sampler_random_access_equals_iteration_and_instances_agree():
    a, b = ShardedSampler(103, 4, 3, 2, seed=1), ShardedSampler(103, 4, 3, 2, seed=1)
    it = iter(a)
    seq = [next(it) for _ in range(12)]  # crosses the epoch boundary at step 8
    for step in (11, 3, 8, 0, 7):  # random access, out of order
        e, idx = b.at(step)
        assert e == seq[step][0] and np.array_equal(idx, seq[step][1])
    assert not np.array_equal(ShardedSampler(103, 4, 3, 2, seed=2).at(0)[1], seq[0][1])
    plain = ShardedSampler(10, 2, 1, 0, shuffle=False)
    assert plain.at(1)[1].tolist() == [2, 3] and plain.at(5)[1].tolist() == [0, 1]


# ---- augmentation parameters -----------------------------------------------------------------------------------
def test_train_params_inside_image_and_independent_of_batching():
    idx = np.arange(1000)
    p = train_params(idx, 3, 11, 64, 64)
    assert p.dtype == np.int32 and p.shape == (1000, 5)
    validate_params(p, 64, 64)
    x0, y0, cw, ch, flip = p.T
    assert (x0 >= 0).all() and (y0 >= 0).all() and (cw >= 1).all() and (ch >= 1).all()
    assert (x0 + cw <= 64).all() and (y0 + ch <= 64).all() and set(flip.tolist()) == {0, 1}
    assert 300 < flip.sum() < 700 and len({tuple(r) for r in p.tolist()}) > 900  # a fair bit; rows vary
    # a sample's row is the same whichever batch, order or rank slice it is computed in
    perm = np.random.default_rng(0).permutation(1000)
    assert np.array_equal(train_params(perm, 3, 11, 64, 64), p[perm])
    assert np.array_equal(train_params(idx[123:131], 3, 11, 64, 64), p[123:131])
    assert np.array_equal(train_params([999], 3, 11, 64, 64), p[999:])
    assert not np.array_equal(train_params(idx, 4, 11, 64, 64), p)  # another epoch, other draws
    assert not np.array_equal(train_params(idx, 3, 12, 64, 64), p)  # another seed
    # a non-square image whose aspect no try can reach in bounds still gets boxes inside it
    validate_params(train_params(idx, 0, 0, 8, 200), 8, 200)


def test_eval_params_and_validation():
    p = eval_params(3, 64, 48)
    assert p.tolist() == [[3, 4, 42, 56, 0]] * 3
    validate_params(p, 64, 48)
    for bad in ((0, 0, 49, 64, 0), (1, 0, 48, 64, 0), (0, 1, 48, 64, 0), (-1, 0, 4, 4, 0), (0, 0, 0, 4, 0),
                (0, 0, 4, 0, 0), (0, 0, 4, 4, 2)):
        with pytest.raises(ValueError):
            validate_params(np.array([bad], dtype=np.int32), 64, 48)
    with pytest.raises(ValueError):
        validate_params(np.zeros((1, 5), dtype=np.int64), 64, 48)
    # the wrapper validates a host table before anything runs
    scale, shift = norm_constants()
    with pytest.raises(ValueError):
        crop_resize_norm(torch.zeros(1, 64, 48, 3, dtype=torch.uint8), torch.tensor([[1, 0, 48, 64, 0]],
                         dtype=torch.int32), 8, scale, shift)


# ---- the mirror ----------------------------------------------------------------------------------------------
def _bf16_bits_rne(f):
    """fp32 value -> bf16 bits by integer round-to-nearest-even (finite inputs)."""
    u = int(np.float32(f).view(np.uint32))
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return u - 65536 if u >= 32768 else u  # as int16


def _pixelwise(raw, rows, S, scale, shift):
    """The specification, one output value at a time in Python integers."""
    raw, sc, sh = raw.numpy(), scale.numpy(), shift.numpy()
    out = np.zeros((len(rows), S, S, 3), dtype=np.int16)
    for n, (x0, y0, cw, ch, flip) in enumerate(rows):
        step_x, step_y = (cw << 16) // S, (ch << 16) // S
        for oy in range(S):
            v = min(max(oy * step_y + (step_y >> 1) - 32768, 0), (ch - 1) << 16)
            iy, fy = v >> 16, (v >> 8) & 255
            iy1 = min(iy + 1, ch - 1)
            for ox in range(S):
                sx = S - 1 - ox if flip else ox
                u = min(max(sx * step_x + (step_x >> 1) - 32768, 0), (cw - 1) << 16)
                ix, fx = u >> 16, (u >> 8) & 255
                ix1 = min(ix + 1, cw - 1)
                for c in range(3):
                    a, b = int(raw[n, y0 + iy, x0 + ix, c]), int(raw[n, y0 + iy, x0 + ix1, c])
                    e, d = int(raw[n, y0 + iy1, x0 + ix, c]), int(raw[n, y0 + iy1, x0 + ix1, c])
                    p = (a * (256 - fx) + b * fx) * (256 - fy) + (e * (256 - fx) + d * fx) * fy
                    assert 0 <= p <= 255 * 65536
                    m = np.float32(p) * sc[c]  # fp32, rounded
                    out[n, oy, ox, c] = _bf16_bits_rne(m + sh[c])  # fp32, rounded; then RNE to bf16
    return torch.from_numpy(out)


@pytest.mark.parametrize("S", [32, 20])
def test_mirror_equals_pixelwise_integers(S):
    raw, params = raw5(), torch.tensor(ROWS5, dtype=torch.int32)
    scale, shift = norm_constants()
    y = crop_resize_norm_ref(raw, params, S, scale, shift)
    assert y.shape == (5, 3, S, S) and y.dtype == torch.bfloat16
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(bits(y.permute(0, 2, 3, 1)), _pixelwise(raw, ROWS5, S, scale, shift))
    # the CPU dispatch of the public op is the mirror, out= included
    out = torch.zeros(5, S, S, 3, dtype=torch.bfloat16)
    assert crop_resize_norm(raw, params, S, scale, shift, out=out) is out
    assert torch.equal(bits(out), bits(y.permute(0, 2, 3, 1)))


@pytest.mark.parametrize("S", [48, 100, 64])
def test_mirror_on_a_linear_ramp(S):
    """Full-image resize of v(x, y) = 2x + y (+ channel) against the ramp's value at the sample position.

    The bound, from the two quantisations and the output format -- not tuned:
    * the source step is floor(W * 2^16 / S) * 2^-16, at most 2^-16 short, and its half is floored once more, so
      the position of output o is at most (o + 1) * 2^-16 <= S * 2^-16 pixels short of (o + 1/2) * W / S - 1/2;
    * the weight keeps the top 8 fraction bits: the position is at most 2^-8 pixels short again;
    * bilinear interpolation of a linear ramp at that quantised position is exact in the integers, and clamping
      both positions into [0, W - 1] cannot move them apart, so the value is at most
      (slope_x + slope_y) * (S * 2^-16 + 2^-8) below the analytic one, never above;
    * mean 0 / std 1 make the affine an exact power-of-two scaling, and bf16 keeps 8 significand bits (7 stored):
      round-to-nearest is off by at most half a unit in the last place, a relative error of at most 2^-8 (the two
      fp32 roundings, 2^-24 each, are counted too).
    """
    H = W = 64
    ax, ay = 2, 1
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.stack([ax * xx + ay * yy + c for c in range(3)], axis=-1)
    assert img.max() <= 255
    raw = torch.from_numpy(img.astype(np.uint8))[None]
    scale, shift = norm_constants(mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
    got = crop_resize_norm_ref(raw, torch.tensor([[0, 0, W, H, 0]], dtype=torch.int32), S, scale, shift)
    got = got.permute(0, 2, 3, 1)[0].to(torch.float64).numpy()
    pos = np.clip((np.arange(S) + 0.5) * W / S - 0.5, 0, W - 1)  # the analytic sample position (H == W)
    want = (ax * pos[None, :] + ay * pos[:, None])[..., None] + np.arange(3)
    quant = (ax + ay) * (S * 2.0 ** -16 + 2.0 ** -8)
    fmt = want * (2.0 ** -8 + 2 * 2.0 ** -24)
    err = got - want
    print("S=%d: error in [%.5f, %.5f], quantisation bound %.5f" % (S, err.min(), err.max(), quant))
    assert (err <= fmt).all() and (err >= -(quant + fmt)).all()


# ---- host gather ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nthreads", [1, 3])
def test_gather_rows_against_fancy_indexing(tmp_path, nthreads):
    from dtg import _runtime
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (13, 7, 5, 3), dtype=np.uint8)  # row_bytes = 105: no multiple of 8
    write_shard(str(tmp_path / "a.dtgrec"), image=img[:8], label=np.arange(8, dtype=np.int64))
    write_shard(str(tmp_path / "b.dtgrec"), image=img[8:], label=np.arange(8, 13, dtype=np.int64))
    s = ShardSet(str(tmp_path))
    assert s.row_bytes("image") == 105
    idx = np.array([12, 0, 7, 8, 7, 7, 3, 12, 9, 1, 0], dtype=np.int64)  # repeats, both shards
    dst = np.full((len(idx) + 1, 7, 5, 3), 0xAB, dtype=np.uint8)  # one row more: it must stay untouched
    _runtime.gather_rows(dst.ctypes.data, s.addresses("image", idx), 105, nthreads)
    assert np.array_equal(dst[:-1], img[idx]) and (dst[-1] == 0xAB).all()
    lab = np.zeros(len(idx), dtype=np.int64)
    _runtime.gather_rows(lab.ctypes.data, s.addresses("label", idx), 8, nthreads)
    assert np.array_equal(lab, idx)
    _runtime.gather_rows(dst.ctypes.data, np.zeros(0, dtype=np.int64), 105, nthreads)  # empty: a no-op
    with pytest.raises(ValueError):
        _runtime.gather_rows(dst.ctypes.data, np.zeros(2, dtype=np.int64), 105, nthreads)  # null sources
    with pytest.raises(IndexError):
        s.addresses("image", [13])


# ---- the loader on the CPU --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def image_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("records")
    images, labels = synthetic_image_set(50, size=24, classes=10, seed=3)
    write_image_shards(str(d), images, labels, per_shard=20)
    return str(d), images, labels


def test_loader_cpu_ranks_make_the_global_batch(image_dir):
    d, images, labels = image_dir
    with DeviceLoader(d, 8, 16, "cpu", world=1, rank=0, seed=5, depth=2) as one, \
            DeviceLoader(d, 4, 16, "cpu", world=2, rank=0, seed=5, depth=2) as r0, \
            DeviceLoader(d, 4, 16, "cpu", world=2, rank=1, seed=5, depth=3) as r1:
        for step in range(8):  # 6 steps per epoch: crosses into epoch 1
            x, y, i = one.next()
            parts = [r0.next(), r1.next()]
            assert x.shape == (8, 3, 16, 16) and x.dtype == torch.bfloat16
            assert x.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(i, torch.cat([p[2] for p in parts]))
            assert torch.equal(y, torch.cat([p[1] for p in parts]))
            assert torch.equal(bits(x), bits(torch.cat([p[0] for p in parts])))
            assert torch.equal(y, torch.from_numpy(labels[i.numpy()]))
            # and the images are the mirror of the gathered records under the sample's own parameters
            p = train_params(i.numpy(), step // 6, 5, 24, 24)
            ref = crop_resize_norm_ref(torch.from_numpy(images[i.numpy()]), torch.from_numpy(p), 16, one.scale,
                                       one.shift)
            assert torch.equal(bits(x), bits(ref))
        assert one.counters()["batches"] == 8 and one.counters()["gather_ms"] > 0
    assert one._thread is None and r0._thread is None


def test_loader_cpu_seek_and_close(image_dir):
    import threading
    d, _, _ = image_dir
    a = DeviceLoader(d, 8, 16, "cpu", seed=2, depth=3)
    seq = [a.next() for _ in range(7)]
    b = DeviceLoader(d, 8, 16, "cpu", seed=2, depth=3)
    b.next()
    b.seek(5)
    assert b.step == 5
    for k in (5, 6):
        x, y, i = b.next()
        assert torch.equal(i, seq[k][2]) and torch.equal(y, seq[k][1]) and torch.equal(bits(x), bits(seq[k][0]))
    b.seek(0)  # backwards too
    assert torch.equal(b.next()[2], seq[0][2])
    ev = DeviceLoader(d, 8, 16, "cpu", train=False)  # evaluation: in order, the centre box, no flip
    assert ev.next()[2].tolist() == list(range(8))
    for l in (a, b, ev):
        l.close()
        l.close()
    assert not [t for t in threading.enumerate() if t.name == "dtg-data-producer"]
    with pytest.raises(RuntimeError):
        a.next()


def test_loader_cpu_seek_inside_a_full_ring(image_dir):
    """depth 2 and three batches taken: both slots have been through the ring when the seek comes, and the batches
    after it are those of a fresh loader's steps 1..3 bit for bit"""
    d, _, _ = image_dir
    with DeviceLoader(d, 8, 16, "cpu", seed=4, depth=2) as fresh, DeviceLoader(d, 8, 16, "cpu", seed=4, depth=2) as a:
        want = [fresh.next() for _ in range(4)]
        for k in range(3):
            assert torch.equal(a.next()[2], want[k][2])
        a.seek(1)
        for k in (1, 2, 3):
            x, y, i = a.next()
            assert torch.equal(i, want[k][2]) and torch.equal(y, want[k][1]) and torch.equal(bits(x), bits(want[k][0]))
        assert a.step == 4 and a.counters()["batches"] == 6


def test_loader_cpu_producer_failure_reaches_next(image_dir):
    import threading
    d, _, _ = image_dir
    loader = DeviceLoader(d, 8, 16, "cpu", seed=1, depth=2)
    loader.shards.close()  # the fields stay in the header, their arrays are gone: the address lookup fails
    with pytest.raises(RuntimeError) as e:
        loader.next()
    assert "DeviceLoader: the producer thread failed" in str(e.value) and isinstance(e.value.__cause__, KeyError)
    assert loader._thread is None
    assert not [t for t in threading.enumerate() if t.name == "dtg-data-producer"]
    loader.close()


def test_data_feed_hook_follows_the_global_step(image_dir):
    """One process: the hook feeds the batch of the session's step, the same one again when a run does not advance
    it, and a restored session continues where the first stopped."""
    from dtg.data import DataFeedHook
    d, _, labels = image_dir

    def job(ckpt, last):
        dtg.reset_default_graph()
        x_ph, y_ph = dtg.placeholder(name="images"), dtg.placeholder(name="labels")
        gs = dtg.train.get_or_create_global_step()
        bump = dtg.assign_add(gs, 1)
        loader = DeviceLoader(d, 8, 16, "cpu", seed=9)
        fed = []
        with dtg.train.MonitoredTrainingSession(checkpoint_dir=ckpt, hooks=[
                dtg.train.StopAtStepHook(last_step=last), DataFeedHook(loader, x_ph, y_ph, gs)],
                save_checkpoint_secs=None, save_checkpoint_steps=100, log_step_count_steps=None,
                save_summaries_steps=None) as sess:
            first = int(sess.run(gs))  # a run that only reads: consumes nothing
            while not sess.should_stop():
                y, step = sess.run([y_ph, bump])
                fed.append((int(step) - 1, np.asarray(y).tolist()))
        assert loader._thread is None  # end() closed it
        return first, fed

    ck = os.path.join(d, "hook_ckpt")
    f1, fed1 = job(ck, 3)
    f2, fed2 = job(ck, 7)
    assert (f1, f2) == (0, 3) and [s for s, _ in fed1 + fed2] == list(range(7))
    samp = ShardedSampler(50, 8, seed=9)
    for step, y in fed1 + fed2:
        assert y == labels[samp.at(step)[1]].tolist()


# ---- resume of the example on 2 gloo ranks ------------------------------------------------------------------------
def _clean_env():
    e = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DTG_FAULT"):
        e.pop(k, None)
    return e


def test_resnet_example_data_dir_resume_bit_equal(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _cluster import free_ports
    data = str(tmp_path / "data")
    images, labels = synthetic_image_set(40, size=36, classes=10, seed=1)  # 5 steps per epoch at 2 x 4
    write_image_shards(data, images, labels, per_shard=16)
    script = os.path.join(ROOT, "examples", "ResNet50", "resnet50_train.py")

    def launch(ck, last):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(free_ports(1)[0]), script, "--tiny", "--batch", "4", "--steps",
               str(last), "--save_every", "100", "--log_every", "1", "--ckpt_dir", ck, "--data_dir", data,
               "--data_seed", "4"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=_clean_env())
        assert r.returncode == 0, r.stdout + r.stderr[-3000:]
        assert "done at global step %d" % last in r.stdout and "loader: batches" in r.stdout, r.stdout
        return r.stdout

    full, parts = str(tmp_path / "ck_full"), str(tmp_path / "ck_parts")
    launch(full, 6)
    launch(parts, 3)
    out = launch(parts, 6)
    assert "resumed from" in out and "(global step 3)" in out, out
    ra = dtg.train.NewCheckpointReader(dtg.train.latest_checkpoint(full))
    rb = dtg.train.NewCheckpointReader(dtg.train.latest_checkpoint(parts))
    keys = sorted(ra.get_variable_to_shape_map())
    assert keys == sorted(rb.get_variable_to_shape_map()) and len(keys) > 10
    assert int(ra.get_tensor("global_step")) == int(rb.get_tensor("global_step")) == 6
    for k in keys:
        assert np.array_equal(np.asarray(ra.get_tensor(k)), np.asarray(rb.get_tensor(k))), k
