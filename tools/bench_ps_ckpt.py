#!/usr/bin/env python3
"""What a checkpoint costs the parameter server's serve thread (parallel/ps_ckpt.py), on one MI355X.

State sizes: ResNet-50 with momentum SGD and BERT-base with Adam (real models, slots filled).  Per model, over
``--rounds`` alternating rounds:

  enqueue   time the calling thread spends in ``PSCheckpointer.maybe_save`` until it returns (pack launches, the
            device copy of the BN buffers, events, the hand-over to the writer thread);
  oracle    time the calling thread spends in the route before the packed image, ``flat_arrays_per_param``: one
            blocking device-to-host copy per parameter and slot (plus a permute per channels_last conv weight);
  pack      device time of the ``state_pack`` launches (events), and parameter bytes read + written / that time,
            beside the 5.28 TB/s copy ceiling of profiles/r05_hbm_probe;
  to file   time from the enqueue to the ``checkpoint`` state file naming the bundle.

Then the one-card async rehearsal (tools/async_ps_rehearsal.sh, 1 PS + 2 workers over gloo with host staging) with
and without ``--save_every 20``: updates/sec for both -- a protocol rehearsal, not a throughput claim.

    python tools/bench_ps_ckpt.py [--out profiles/ps_ckpt/table.md] [--no-rehearsal]
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import dtg  # noqa: E402,F401
from dtg.ops import snapshot as S  # noqa: E402
from dtg.optim import FusedAdam, FusedSGD  # noqa: E402
from dtg.parallel import FlatParams  # noqa: E402
from dtg.parallel.ps_ckpt import PSCheckpointer  # noqa: E402
from dtg.train.saver import flat_arrays_per_param, latest_checkpoint  # noqa: E402

COPY_CEILING_TBS = 5.28  # profiles/r05_hbm_probe/README.md, copy


def _resnet50(dev):
    from dtg.models import resnet
    model = resnet.resnet50().to(dev).to(memory_format=torch.channels_last)
    flat = FlatParams(model)
    return flat, FusedSGD(flat, lr=0.1, momentum=0.9), ("momentum",)


def _bert_base(dev):
    from dtg.models import bert
    model = bert.BertForPreTraining(bert.BertConfig.base()).to(dev)
    flat = FlatParams(model)
    return flat, FusedAdam(flat, lr=1e-4), ("m", "v")


def _pack_ms(ck, flat, iters=20):
    """Device time of one snapshot's pack launches (events around ``iters`` back-to-back snapshots)."""
    snap = ck.snap
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        for g in flat:
            S.state_pack(snap.plans[g.name], snap._bufs(g), snap.dev_img[g.name])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _model_rows(name, make, dev, rounds):
    flat, opt, slots = make(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    for g in flat:
        for k in slots:
            opt.new_slot(g, k).copy_(torch.randn(g.numel, device=dev, generator=gen))
    opt.step_count = 1
    n_param = sum(p.numel() for g in flat for p in g.params)
    n_keys = sum(len(g.params) for g in flat) * (1 + len(slots))
    d = tempfile.mkdtemp(prefix="dtg_ps_ckpt_")
    try:
        ck = PSCheckpointer(flat, opt, d, every_n=1, max_to_keep=1)
        ck.maybe_save(1)  # allocates the device images and the pinned host images
        ck.wait()
        flat_arrays_per_param(flat, opt)
        torch.cuda.synchronize()
        enq, orc, pack, tofile = [], [], [], []
        for r in range(rounds):
            step = 2 + r
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert ck.maybe_save(step)
            enq.append(time.perf_counter() - t0)
            ck.wait()
            assert latest_checkpoint(d).endswith("-%d" % step)
            tofile.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            flat_arrays_per_param(flat, opt)
            orc.append(time.perf_counter() - t0)
            pack.append(_pack_ms(ck, flat) * 1e-3)
        ck.flush()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    med = statistics.median
    moved = 2 * 4 * n_param * (1 + len(slots))
    return {"model": name, "param_elements": n_param, "keys": n_keys, "slots": list(slots),
            "enqueue_ms": [t * 1e3 for t in enq], "oracle_ms": [t * 1e3 for t in orc],
            "pack_ms": [t * 1e3 for t in pack], "to_file_s": tofile,
            "enqueue_ms_median": med(enq) * 1e3, "oracle_ms_median": med(orc) * 1e3,
            "pack_ms_median": med(pack) * 1e3, "pack_tbs": moved / med(pack) / 1e12,
            "copy_ceiling_tbs": COPY_CEILING_TBS, "to_file_s_median": med(tofile),
            "enqueue_cheaper_every_round": max(enq) < min(orc)}


def _rehearsal(extra):
    d = tempfile.mkdtemp(prefix="dtg_ps_ckpt_reh_")
    try:
        cmd = ["bash", os.path.join(ROOT, "tools", "async_ps_rehearsal.sh"), "2", "--steps", "60", "--batch", "16",
               "--image", "128"] + [x.replace("@D", d) for x in extra]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        m = re.search(r"^\[ps\] ([0-9.]+) updates/sec", r.stdout, re.M)
        saved = re.search(r"^\[ps\] checkpoints at (.*)$", r.stdout, re.M)
        if r.returncode != 0 or not m:
            return {"error": (r.stdout + r.stderr)[-2000:]}
        return {"updates_per_sec": float(m.group(1)), "checkpoints": saved.group(1) if saved else None}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the markdown table here")
    ap.add_argument("--no-rehearsal", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ps_ckpt needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    where = "%s, torch %s, hip %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip)
    lines = ["Measured on: %s (one device, %d alternating rounds; median, min..max)" % (where, a.rounds), "",
             "| model | parameter elements | keys | maybe_save on the caller, ms | per-parameter route on the caller, ms "
             "| pack launches, ms | pack TB/s (copy ceiling %.2f) | enqueue -> state file, s |" % COPY_CEILING_TBS,
             "|---|---|---|---|---|---|---|---|"]

    def span(v, f="%.2f"):
        return (f + " (" + f + ".." + f + ")") % (statistics.median(v), min(v), max(v))
    for name, make in (("resnet50 + momentum", _resnet50), ("bert_base + adam", _bert_base)):
        row = _model_rows(name, make, dev, a.rounds)
        row["where"] = where
        print(json.dumps(row), flush=True)
        lines.append("| %s | %d | %d | %s | %s | %s | %.2f | %s |"
                     % (name, row["param_elements"], row["keys"], span(row["enqueue_ms"]), span(row["oracle_ms"], "%.1f"),
                        span(row["pack_ms"], "%.3f"), row["pack_tbs"], span(row["to_file_s"])))
        torch.cuda.empty_cache()
    if not a.no_rehearsal:
        lines += ["", "One-card async rehearsal (ResNet-50, 1 PS + 2 workers, batch 16, 128 px, 60 steps per worker; a "
                  "protocol rehearsal over gloo with host staging, not a throughput claim):", "",
                  "| run | PS updates/sec | checkpoints |", "|---|---|---|"]
        for label, extra in (("no checkpoints", []), ("--save_every 20", ["--ckpt_dir", "@D", "--save_every", "20"])):
            res = _rehearsal(extra)
            print(json.dumps({"rehearsal": label, **res}), flush=True)
            lines.append("| %s | %s | %s |" % (label, res.get("updates_per_sec", "failed"), res.get("checkpoints", "-")))
    table = "\n".join(lines) + "\n"
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table)


if __name__ == "__main__":
    main()
