#!/usr/bin/env python3
"""mlm_mask (csrc/kernels/mlm_mask.hip) against the two ways of masking without it, on one GPU.

Device events around ``--launches`` back-to-back calls, every shape warmed, ``--rounds`` rounds alternating the paths
on the same inputs, at [256, 128] and [256, 512] with P = 20 / 80:

* ``hip``    the kernel: one launch from the device twins of a record batch to the five int64 tensors;
* ``aten``   the mirror ``mlm_mask_ref`` on the same device tensors: the chain of ATen launches (hashes, two sorts,
             gathers, wheres) one would assemble from framework ops; the same bits;
* ``host``   the mirror on the host tensors (pinned) plus the copies of its five results to the device, in wall time:
             what masking in the loader's producer thread would cost per batch.

Reported per shape: median and min..max over the rounds of each path, and the ATen op count of the chain.

    python tools/bench_mlm_mask.py [--launches 20 --rounds 5] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dtg  # noqa: E402,F401
from dtg.data import synthetic_token_set  # noqa: E402
from dtg.ops.mlm import mlm_mask, mlm_mask_ref  # noqa: E402

SHAPES = ((256, 128, 20), (256, 512, 80))
IDS = dict(mask_id=3, vocab_lo=4, vocab_hi=30522, special_ids=(0, 1, 2, 3))


def count_ops(fn):
    from torch.utils._python_dispatch import TorchDispatchMode

    class Counter(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Counter.n += 1
            return func(*args, **(kwargs or {}))

    with Counter():
        fn()
    return Counter.n


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches  # ms per call


def timed_wall(fn, launches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / launches


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlm_mask.py measures on a GPU; none is available")
    dev = torch.device("cuda", 0)
    results = []
    for B, S, P in SHAPES:
        f = synthetic_token_set(B, seq=S, vocab_hi=IDS["vocab_hi"], seed=S)
        host = tuple(torch.from_numpy(x).pin_memory() for x in (f["input_ids"], f["a_len"], f["length"],
                                                                 np.arange(B, dtype=np.int64)))
        d = tuple(t.to(dev) for t in host)
        kw = dict(IDS, seed=1, epoch=0, P=P)
        out = tuple(torch.empty(s, dtype=torch.int64, device=dev) for s in [(B, S)] * 3 + [(B, P)] * 2)

        def hip():
            mlm_mask(*d, out=out, **kw)

        def aten():
            mlm_mask_ref(*d, **kw)

        def on_host():
            for o, r in zip(out, mlm_mask_ref(*host, **kw)):
                o.copy_(r, non_blocking=True)

        hip()
        same = all(torch.equal(x, y) for x, y in zip(out, mlm_mask_ref(*d, **kw)))
        ops = count_ops(aten)
        for fn in (hip, aten, on_host):  # warm every path
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        rows = []
        for r in range(a.rounds):
            row = {"round": r, "hip_ms": timed(hip, a.launches), "aten_ms": timed(aten, a.launches),
                   "host_ms": timed_wall(on_host, max(2, a.launches // 4))}
            rows.append(row)
            print("[%d, %d] P=%d round %d: mlm_mask %.4f ms, ATen chain %.4f ms, host mirror + copies %.4f ms" % (
                B, S, P, r, row["hip_ms"], row["aten_ms"], row["host_ms"]), flush=True)
        res = {"B": B, "S": S, "P": P, "launches": a.launches, "rounds": rows, "aten_ops": ops, "hip_launches": 1,
               "bit_equal_to_mirror": bool(same), "predictions": int((out[4] >= 0).sum())}
        for k in ("hip", "aten", "host"):
            v = np.array([x[k + "_ms"] for x in rows])
            res.update({k + "_ms_median": float(np.median(v)), k + "_ms_min": float(v.min()),
                        k + "_ms_max": float(v.max())})
        print("[%d, %d] P=%d: mlm_mask median %.4f ms [%.4f, %.4f]; ATen chain (%d ops) %.4f ms [%.4f, %.4f]; host "
              "mirror + copies %.4f ms [%.4f, %.4f]; bit-equal %s" % (
                  B, S, P, res["hip_ms_median"], res["hip_ms_min"], res["hip_ms_max"], ops, res["aten_ms_median"],
                  res["aten_ms_min"], res["aten_ms_max"], res["host_ms_median"], res["host_ms_min"],
                  res["host_ms_max"], same), flush=True)
        results.append(res)
    print(json.dumps(results))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
