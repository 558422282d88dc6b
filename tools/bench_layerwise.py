#!/usr/bin/env python3
"""What the layer-wise optimizers (FusedLAMB, FusedLARS) and global-norm clipping cost next to the elementwise
applies, on the real flat layouts of ResNet-50 (~25.6 M elements, 161 parameters, most of them far smaller than a
chunk) and BERT-base (~110 M elements).

Per model, in the same run and alternating over ``--rounds`` rounds:

  passes  adam_apply / momentum_apply (the elementwise baselines, optim.hip) and each new pass of layerwise.hip
          over every flat group: seg_sqnorm (g alone; w and g), lamb_moments, lamb_apply, lars_apply, seg_finalize
  steps   FusedAdam vs FusedLAMB vs FusedLAMB + clip vs FusedAdam + clip;  FusedSGD (momentum) vs FusedLARS

Bytes per element are algorithmic, from the kernels' access lists with e = gradient element size (2 in the bf16
``compute`` group, 4 in ``fp32``) and mir = 2 where the group has a bf16 mirror:

  adam_apply 24 + e + mir     momentum_apply / lars_apply 16 + e + mir     seg_sqnorm(g) e     seg_sqnorm(w, g) 4 + e
  lamb_moments 20 + e         lamb_apply 16 + mir

The gradient is NOT zeroed in these runs (a timed window repeats a step thousands of times on the same gradient,
with a learning rate of 1e-6 so the values stay put); the byte counts leave the zeroing store out accordingly.
TB/s = bytes x elements / time: an algorithmic rate, what the infinity cache serves is not subtracted (the
ResNet-50 buffers fit in it, the BERT ones do not).  Timing: device events around a window of about ``--window``
seconds of back-to-back launches.  Needs a GPU; prints the device it ran on.

    python tools/bench_layerwise.py [--out profiles/layerwise_optim/table.md]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dtg  # noqa: E402,F401
from dtg.ops import layerwise as L  # noqa: E402
from dtg.ops import optim_kernels as K  # noqa: E402
from dtg.optim import FusedAdam, FusedLAMB, FusedLARS, FusedSGD  # noqa: E402
from dtg.parallel import FlatParams  # noqa: E402


def _model(name, dev):
    if name == "resnet50":
        from dtg.models import resnet
        return resnet.resnet50().to(dev).to(memory_format=torch.channels_last)
    from dtg.models import bert
    return bert.BertForPreTraining(bert.BertConfig.base()).to(dev)


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def _bytes(flat, fixed, per_e, per_mir):
    """Total bytes of a pass over every group: (fixed + per_e * e + per_mir * mir) per real (unpadded) element."""
    total = 0
    for g in flat:
        n = sum(p.numel() for p in g.params)
        total += n * (fixed + per_e * g.grad.element_size() + per_mir * (2 if g.mirror is not None else 0))
    return total


def _variants(flat):
    """name -> (callable, bytes).  One plan, one set of slots, shared by the pass variants."""
    hyper = torch.tensor([1e-6, 10.0], device=flat.groups["compute"].master.device)
    plan = L.LayerwisePlan(flat)
    groups = list(flat)
    spans = [plan.span(g) for g in groups]
    for g in groups:
        g.grad.copy_(torch.randn(g.numel, device=g.grad.device) * 1e-3)
        g.state_buffer("v").fill_(1e-6)
    adapt, wd = [g.name == "compute" for g in groups], [0.01 if g.name == "compute" else 0.0 for g in groups]

    def each(fn):
        def run():
            for g, s in zip(groups, spans):
                fn(g, s)
        return run

    v = {
        "pass adam_apply": (each(lambda g, s: K.adam(g.master, g.grad, g.state_buffer("m"), g.state_buffer("v"), hyper,
                                                     g.mirror, wd=0.01)), _bytes(flat, 24, 1, 1)),
        "pass momentum_apply": (each(lambda g, s: K.momentum(g.master, g.grad, g.state_buffer("momentum"), hyper,
                                                             g.mirror, wd=5e-5)), _bytes(flat, 16, 1, 1)),
        "pass seg_sqnorm(g)": (each(lambda g, s: L.seg_sqnorm(plan, s, None, g.grad)), _bytes(flat, 0, 1, 0)),
        "pass seg_sqnorm(w,g)": (each(lambda g, s: L.seg_sqnorm(plan, s, g.master, g.grad)), _bytes(flat, 4, 1, 0)),
        "pass lamb_moments": (each(lambda g, s: L.lamb_moments(plan, s, g.master, g.grad, g.state_buffer("m"),
                                                               g.state_buffer("v"), hyper, 0.9, 0.999, 1e-6, 0.01)),
                              _bytes(flat, 20, 1, 0)),
        "pass lamb_apply": (each(lambda g, s: L.lamb_apply(plan, s, g.master, g.mirror, g.state_buffer("m"),
                                                           g.state_buffer("v"), hyper, 0.9, 0.999, 1e-6, 0.01)),
                            _bytes(flat, 16, 0, 1)),
        "pass lars_apply": (each(lambda g, s: L.lars_apply(plan, s, g.master, g.mirror, g.grad,
                                                           g.state_buffer("momentum"), hyper, 0.9, 5e-5)),
                            _bytes(flat, 16, 1, 1)),
        "pass seg_finalize": (lambda: L.seg_finalize(plan, L.LAMB, adapt, wd, clip_norm=1.0), 8 * plan.n_chunks),
    }
    opts = {
        "step FusedAdam": (FusedAdam(flat, lr=1e-6), _bytes(flat, 24, 1, 1)),
        "step FusedAdam+clip": (FusedAdam(flat, lr=1e-6, clip_norm=1.0), _bytes(flat, 24, 2, 1)),
        "step FusedLAMB": (FusedLAMB(flat, lr=1e-6), _bytes(flat, 36, 1, 1)),
        "step FusedLAMB+clip": (FusedLAMB(flat, lr=1e-6, clip_norm=1.0), _bytes(flat, 36, 2, 1)),
        "step FusedSGD momentum": (FusedSGD(flat, lr=1e-6, momentum=0.9, weight_decay=5e-5), _bytes(flat, 16, 1, 1)),
        "step FusedLARS": (FusedLARS(flat, lr=1e-6), _bytes(flat, 20, 2, 1)),
    }
    for name, (opt, nbytes) in opts.items():
        v[name] = ((lambda o: lambda: o.step(zero_grad=False))(opt), nbytes)
    return v, plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--models", default="resnet50,bert_base")
    ap.add_argument("--out", default=None, help="also write the markdown table here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_layerwise needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    where = "%s, torch %s, hip %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip)
    lines = ["Measured on: %s (one device, device events, %d rounds alternating over the variants, ~%.2f s windows)"
             % (where, a.rounds, a.window), ""]
    for model in a.models.split(","):
        torch.manual_seed(0)
        flat = FlatParams(_model(model, dev))
        variants, plan = _variants(flat)
        n = sum(p.numel() for g in flat for p in g.params)
        small = sum(1 for g in flat for p in g.params if p.numel() < L.CHUNK)
        iters = {}
        for name, (fn, _) in variants.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            iters[name] = max(5, int(a.window / _time(fn, 5)))
        t = {name: [] for name in variants}
        for _ in range(a.rounds):
            for name, (fn, _) in variants.items():
                t[name].append(_time(fn, iters[name]))
        med = {name: statistics.median(x) for name, x in t.items()}
        base = variants["pass adam_apply"][1] / med["pass adam_apply"]
        lines += ["**%s**: %d elements in %d parameters (%d below one chunk of %d), %d chunks" %
                  (model, n, plan.n_rows, small, L.CHUNK, plan.n_chunks), "",
                  "| variant | ms (min..max) | B/elem | TB/s | rate / adam_apply |", "|---|---|---|---|---|"]
        for name, (_, nbytes) in variants.items():
            rate = nbytes / med[name]
            row = {"model": model, "variant": name, "ms": med[name] * 1e3, "min_ms": min(t[name]) * 1e3,
                   "max_ms": max(t[name]) * 1e3, "bytes_per_elem": nbytes / n, "tbs": rate / 1e12,
                   "vs_adam_apply": rate / base, "where": where}
            print(json.dumps(row), flush=True)
            lines.append("| %s | %.4f (%.4f..%.4f) | %.1f | %.2f | %.2f |" %
                         (name, row["ms"], row["min_ms"], row["max_ms"], row["bytes_per_elem"], row["tbs"],
                          row["vs_adam_apply"]))
        for a_, b_ in (("step FusedLAMB", "step FusedAdam"), ("step FusedLAMB+clip", "step FusedAdam"),
                       ("step FusedAdam+clip", "step FusedAdam"), ("step FusedLARS", "step FusedSGD momentum")):
            lines.append("")
            lines.append("%s / %s: %.2fx the time" % (a_, b_, med[a_] / med[b_]))
        lines.append("")
        del flat, variants, plan
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
