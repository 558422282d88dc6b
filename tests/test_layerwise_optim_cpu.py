"""Layer-wise adaptive optimizers (FusedLAMB, FusedLARS) and global-norm clipping on the CPU mirrors
(ops/layerwise.py, optim/fused.py) against an independent per-tensor fp64 reference, through every step entry of
the flat optimizers (whole groups, bucket ranges, ``grads=``, ``step_sum``, two gloo ranks), checkpoints and the
example scripts."""
import os
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# fp32 mirror against the fp64 reference over three steps: fp32 rounds at 6e-8 per operation, an element sees a few
# tens of operations per step and the norms a few thousand adds (relative error ~ sqrt(n) * 6e-8 in practice,
# n * 6e-8 = 2e-4 of the NORM at worst, which enters the update, itself ~ lr * |w|, not the weight)
RTOL, ATOL = 1e-4, 1e-6


class Toy(torch.nn.Module):
    """Parameters in both flat groups: 2-D weights (compute: one of them longer than a chunk, one tiny) and 1-D
    biases (fp32)."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(7)
        P = torch.nn.Parameter
        self.w1 = P(torch.randn(40, 70, generator=g) * 0.1)   # 2800 elements: two chunks
        self.b1 = P(torch.randn(70, generator=g) * 0.1)
        self.w2 = P(torch.randn(70, 5, generator=g) * 0.1)
        self.b2 = P(torch.randn(5, generator=g) * 0.1)
        self.w3 = P(torch.randn(3, 3, generator=g))

    def forward(self, x):
        h = torch.tanh(x @ self.w1 + self.b1)
        return (h @ self.w2 + self.b2) @ torch.ones(5, 3) @ self.w3


def _grads(steps=3, scales=(1.0, 0.3, 1e-3), seed=11):
    """Per step a dict name -> gradient; the scales make the global norm cross a clip threshold of 1."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in range(steps):
        out.append({n: torch.randn(p.shape, generator=g) * scales[s] for n, p in Toy().named_parameters()})
    return out


def _set_grads(model, gd):
    for n, p in model.named_parameters():
        p.grad.copy_(gd[n])


def _build(make, dtype=torch.float32):
    from dtg.parallel import FlatParams
    model = Toy()
    flat = FlatParams(model, compute_dtype=dtype)
    return model, flat, make(flat)


def _reference(kind, grads, lr, gscale=1.0, clip=None, wd=0.01, b1=0.9, b2=0.999, eps=1e-6, mu=0.9, eta=0.001,
               lars_eps=0.0, masters=None):
    """Per-tensor fp64 reference over ordinary tensors (no flat buffers).  2-D parameters are the compute group
    (weight decay, adaptation), 1-D the fp32 group (neither).  Returns (weights, clip factors per step)."""
    w = {n: p.detach().double().clone() for n, p in Toy().named_parameters()}
    if masters is not None:
        w = {n: v.double().clone() for n, v in masters.items()}
    st0 = {n: torch.zeros_like(v) for n, v in w.items()}
    st1 = {n: torch.zeros_like(v) for n, v in w.items()}
    cs = []
    for t, gd in enumerate(grads, 1):
        gd = {n: v.double() for n, v in gd.items()}
        c = 1.0
        if clip is not None:
            gn = gscale * sum(float((v * v).sum()) for v in gd.values()) ** 0.5
            c = clip / max(gn, clip)
        cs.append(c)
        for n in w:
            comp = w[n].dim() > 1
            wdn = wd if comp else 0.0
            g = gd[n] * gscale * c
            if kind in ("lamb", "adam"):
                st0[n] = b1 * st0[n] + (1 - b1) * g
                st1[n] = b2 * st1[n] + (1 - b2) * g * g
                u = (st0[n] / (1 - b1 ** t)) / ((st1[n] / (1 - b2 ** t)).sqrt() + eps) + wdn * w[n]
                r = 1.0
                if kind == "lamb" and comp:
                    nw, nu = float(w[n].norm()), float(u.norm())
                    r = nw / nu if nw > 0 and nu > 0 else 1.0
                w[n] = w[n] - lr * r * u
            elif kind == "lars":
                r = 1.0
                nw, ng = float(w[n].norm()), float(gd[n].norm())
                if comp and nw > 0 and ng > 0:
                    r = eta * nw / (gscale * c * ng + wdn * nw + lars_eps)
                st0[n] = mu * st0[n] + lr * r * (g + wdn * w[n])
                w[n] = w[n] - st0[n]
            elif kind == "momentum":
                st0[n] = mu * st0[n] + g + wdn * w[n]
                w[n] = w[n] - lr * st0[n]
            else:
                raise AssertionError(kind)
    return w, cs


def _cases():
    from dtg.optim import FusedAdam, FusedLAMB, FusedLARS, FusedSGD
    return {
        "lamb": (lambda f: FusedLAMB(f, lr=0.01), dict(kind="lamb", lr=0.01)),
        "lamb_clip": (lambda f: FusedLAMB(f, lr=0.01, clip_norm=1.0), dict(kind="lamb", lr=0.01, clip=1.0)),
        "lars": (lambda f: FusedLARS(f, lr=0.5, weight_decay=0.01, eta=0.02),
                 dict(kind="lars", lr=0.5, wd=0.01, eta=0.02)),
        "lars_clip": (lambda f: FusedLARS(f, lr=0.5, weight_decay=0.01, eta=0.02, eps=1e-9, clip_norm=1.0),
                      dict(kind="lars", lr=0.5, wd=0.01, eta=0.02, lars_eps=1e-9, clip=1.0)),
        "adam_clip": (lambda f: FusedAdam(f, lr=0.01, clip_norm=1.0), dict(kind="adam", lr=0.01, clip=1.0)),
        "momentum_clip": (lambda f: FusedSGD(f, lr=0.05, momentum=0.9, weight_decay=0.01, clip_norm=1.0),
                          dict(kind="momentum", lr=0.05, clip=1.0)),
    }


@pytest.mark.parametrize("name", ["lamb", "lamb_clip", "lars", "lars_clip", "adam_clip", "momentum_clip"])
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_three_steps_match_fp64_per_tensor_reference(name, gscale):
    make, ref_kw = _cases()[name]
    grads = _grads()
    model, flat, opt = _build(make)
    cs = []
    for gd in grads:
        _set_grads(model, gd)
        opt.step(grad_scale=gscale)
        cs.append(float(opt._plan().cfac[0]))
        assert all(float(g.grad.abs().sum()) == 0 for g in flat)  # zeroed by the step
    want, want_c = _reference(grads=grads, gscale=gscale, **ref_kw)
    if "clip" in name:
        assert want_c[0] < 1.0 and want_c[-1] == 1.0, want_c  # the threshold bites first, then lets go
    assert cs == pytest.approx(want_c, rel=1e-5)
    for n, p in model.named_parameters():
        assert torch.allclose(p.detach().double(), want[n], rtol=RTOL, atol=ATOL), (name, n)
    assert opt.step_count == 3 and float(opt.hyper[1]) == 3.0


def test_bf16_group_writes_mirror_and_zeroes_grad():
    from dtg.optim import FusedLAMB, FusedLARS
    for make in (lambda f: FusedLAMB(f, lr=0.01, clip_norm=1.0), lambda f: FusedLARS(f, lr=0.5, eta=0.02)):
        model, flat, opt = _build(make, torch.bfloat16)
        _set_grads(model, _grads()[0])
        before = flat.groups["compute"].master.clone()
        opt.step()
        g = flat.groups["compute"]
        assert not torch.equal(g.master, before)
        assert torch.equal(g.mirror, g.master.to(torch.bfloat16)) and float(g.grad.abs().sum()) == 0


def _param_ranges(flat, perm_seed=3):
    """One range per parameter (offset to the next parameter's offset, as DataParallel's buckets), permuted."""
    out = []
    for g in flat:
        offs = list(g.offsets) + [g.numel]
        out += [(g, offs[i], offs[i + 1], lambda: None) for i in range(len(g.offsets))]
    order = torch.randperm(len(out), generator=torch.Generator().manual_seed(perm_seed)).tolist()
    return [out[i] for i in order]


@pytest.mark.parametrize("name", ["lamb", "lamb_clip", "lars_clip", "adam_clip"])
def test_ranges_bit_equal_to_whole_step_and_cut_raises(name):
    make, _ = _cases()[name]
    grads = _grads()
    runs = []
    for ranged in (False, True):
        model, flat, opt = _build(make, torch.bfloat16)
        for gd in grads:
            _set_grads(model, gd)
            opt.step(grad_scale=0.5, ranges=_param_ranges(flat) if ranged else None)
        runs.append([g.master.clone() for g in flat] + [b.clone() for g in flat for b in g.state.values()] +
                    [g.grad.clone() for g in flat] + [flat.groups["compute"].mirror.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    g = flat.groups["compute"]
    w1 = g.names.index("w1")
    lo = g.offsets[w1]
    before = g.master.clone()
    with pytest.raises(ValueError, match="cuts parameter"):
        opt.step(ranges=[(g, lo, lo + 100, lambda: None)])
    with pytest.raises(ValueError, match="cuts parameter"):
        opt.step(ranges=[(g, lo + 64, g.numel, lambda: None)])
    assert torch.equal(g.master, before)  # refused before any kernel ran
    assert opt.step_count == 3 and float(opt.hyper[1]) == 3.0  # ... and before the step was counted


@pytest.mark.parametrize("name", ["lamb_clip", "lars", "adam_clip"])
def test_step_sum_equals_step_on_summed_gradient(name):
    make, _ = _cases()[name]
    srcs_by_step = [_grads(seed=20 + c) for c in range(3)]  # three contributions
    runs = []
    for mode in ("sum", "grads"):
        model, flat, opt = _build(make)
        for s in range(3):
            sources = []
            for c in range(3):
                _set_grads(model, srcs_by_step[c][s])
                sources.append([g.grad.clone() for g in flat])
            flat.zero_grad()
            if mode == "sum":
                opt.step_sum(sources, grad_scale=1.0 / 3)
            else:
                total = [(a.float() + b.float()) + c.float() for a, b, c in zip(*sources)]
                opt.step(grad_scale=1.0 / 3, zero_grad=False, grads=total)
        runs.append([g.master.clone() for g in flat])
        assert opt.step_count == 3
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert all(torch.isfinite(t).all() for t in runs[0])


def test_zero_norms_take_ratio_one_and_stay_finite():
    from dtg.optim import FusedLAMB, FusedLARS
    for kind, make in (("lamb", lambda f: FusedLAMB(f, lr=0.01, weight_decay=0.0)),
                       ("lars", lambda f: FusedLARS(f, lr=0.5, eta=0.02))):
        model, flat, opt = _build(make)
        g = flat.groups["compute"]
        iw, ig = g.names.index("w2"), g.names.index("w3")
        with torch.no_grad():
            g.master_view(iw).zero_()        # an all-zero weight
        gd = _grads()[0]
        gd["w3"] = torch.zeros_like(gd["w3"])  # an all-zero gradient
        masters = {n: v.clone() for n, v in flat.named_masters()}
        _set_grads(model, gd)
        opt.step()
        plan = opt._plan()
        lo = plan.span(g).r_lo
        assert float(plan.ratio[lo + iw]) == 1.0 and float(plan.ratio[lo + ig]) == 1.0, (kind, plan.ratio)
        assert float(plan.ratio[lo + g.names.index("w1")]) != 1.0
        assert all(torch.isfinite(x.master).all() for x in flat) and torch.isfinite(plan.ratio).all()
        want, _ = _reference(kind, [gd], lr=opt.lr, wd=opt.weight_decay, eta=0.02, masters=masters)
        for n, v in flat.named_masters():
            assert torch.allclose(v.double(), want[n], rtol=RTOL, atol=ATOL), (kind, n)


def test_defaults_unchanged_and_make_optimizer_names():
    from dtg.optim import FusedAdam, FusedLAMB, FusedLARS, FusedSGD, make_optimizer
    grads = _grads()
    for without, with_none in ((lambda f: FusedAdam(f, lr=0.01), lambda f: FusedAdam(f, lr=0.01, clip_norm=None)),
                               (lambda f: FusedSGD(f, lr=0.05), lambda f: FusedSGD(f, lr=0.05, clip_norm=None))):
        runs = []
        for make in (without, with_none):
            model, flat, opt = _build(make, torch.bfloat16)
            assert not opt._normed
            for gd in grads:
                _set_grads(model, gd)
                opt.step(grad_scale=0.5)
            assert opt._lw_plan is None  # today's path: no tables, no norm pass
            runs.append([g.master.clone() for g in flat] + [b.clone() for g in flat for b in g.state.values()])
        assert all(torch.equal(a, b) for a, b in zip(*runs))
    _, flat, _ = _build(lambda f: None)
    assert isinstance(make_optimizer("lamb", flat, 0.01), FusedLAMB)
    assert isinstance(make_optimizer("lars", flat, 0.1), FusedLARS)
    assert make_optimizer("lamb", flat, 0.01, clip_norm=1.0).clip_norm == 1.0
    with pytest.raises(ValueError, match="unknown optimizer"):
        make_optimizer("lion", flat, 0.01)
    with pytest.raises(ValueError):
        FusedAdam(flat, lr=0.01, clip_norm=0.0)


@pytest.mark.parametrize("name", ["lamb_clip", "lars"])
def test_checkpoint_roundtrip_then_step_is_bit_equal(name, tmp_path):
    from dtg.train import restore_flat, save_flat
    make, _ = _cases()[name]
    grads = _grads()
    model, flat, opt = _build(make, torch.bfloat16)
    for gd in grads[:2]:
        _set_grads(model, gd)
        opt.step()
    prefix = save_flat(flat, str(tmp_path / "ck"), global_step=2, optimizer=opt)
    _set_grads(model, grads[2])
    opt.step()
    model2, flat2, opt2 = _build(make, torch.bfloat16)
    assert restore_flat(flat2, prefix, optimizer=opt2) == 2 and opt2.step_count == 2
    slots = {"lamb_clip": {"m", "v"}, "lars": {"momentum"}}[name]
    assert all(set(g.state) == slots for g in flat2)  # no new checkpoint key: the slots Adam / momentum SGD have
    _set_grads(model2, grads[2])
    opt2.step()
    for a, b in zip(flat, flat2):
        assert torch.equal(a.master, b.master) and torch.equal(a.mirror if a.mirror is not None else a.master,
                                                               b.mirror if b.mirror is not None else b.master)
        assert all(torch.equal(a.state[k], b.state[k]) for k in slots)


def _rank(rank, world, port, q):
    """LAMB + clip through DataParallel.step on 2 gloo ranks with per-rank gradients == one process stepping on
    the mean gradient (grad_scale 1/2 on the sum), bit for bit."""
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        import dtg  # noqa: F401
        from dtg.optim import FusedLAMB
        from dtg.parallel import DataParallel, FlatParams, comm
        comm.init("gloo")
        xs = [torch.randn(6, 40, generator=torch.Generator().manual_seed(100 * s + r)) * (8.0 if s == 0 else 0.05)
              for s in range(3) for r in range(world)]
        model = Toy()
        flat = FlatParams(model, compute_dtype=torch.float32)
        dp = DataParallel(flat, bucket_mb=0.001)
        assert len(dp.buckets) > 2
        opt = FusedLAMB(flat, lr=0.01, clip_norm=1.0)
        ref_model = Toy()
        ref_flat = FlatParams(ref_model, compute_dtype=torch.float32)
        ref = FusedLAMB(ref_flat, lr=0.01, clip_norm=1.0)
        cs = []
        for s in range(3):
            k = (1.0, 1e-2, 1e-5)[s]  # loss scale: the gradient norm crosses the clip threshold
            (model(xs[s * world + rank]).square().sum() * k).backward()
            dp.step(opt)
            for r in range(world):  # both shards' gradients accumulate into the flat buffer: their sum
                (ref_model(xs[s * world + r]).square().sum() * k).backward()
            ref.step(grad_scale=1.0 / world)
            cs.append(float(ref._plan().cfac[0]))
        assert cs[0] < 1.0 and cs[-1] == 1.0, cs
        for a, b in zip(flat, ref_flat):
            assert torch.equal(a.master, b.master), (a.master - b.master).abs().max()
            assert all(torch.equal(a.state[k], b.state[k]) for k in ("m", "v"))
        assert torch.equal(opt._plan().ratio, ref._plan().ratio)
        comm.shutdown()
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, traceback.format_exc()))
        raise


def test_lamb_clip_two_gloo_ranks_equals_mean_gradient_step():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _cluster import free_ports
    port = free_ports(1)[0]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    res = dict(q.get(timeout=5) for _ in range(2))
    assert res == {0: "ok", 1: "ok"}, res


def _clean_env():
    e = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DTG_FAULT"):
        e.pop(k, None)
    return e


@pytest.mark.parametrize("script,extra,slot", [
    (("BERT", "bert_train.py"), ["--opt", "lamb", "--clip_norm", "1.0", "--warmup", "2"], "emb.word/m"),
    (("ResNet50", "resnet50_train.py"), ["--opt", "lars"], "fc.weight/momentum"),
])
def test_examples_run_and_resume_with_the_new_optimizers(script, extra, slot, tmp_path):
    import dtg
    ck = str(tmp_path / "ck")
    path = os.path.join(ROOT, "examples", *script)

    def launch(last):
        cmd = [sys.executable, path, "--tiny", "--batch", "4", "--steps", str(last), "--save_every", "2",
               "--log_every", "2", "--ckpt_dir", ck] + extra
        return subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=_clean_env())

    r1 = launch(2)
    assert r1.returncode == 0, r1.stdout + r1.stderr[-3000:]
    assert "done at global step 2" in r1.stdout and "nan" not in r1.stdout.lower(), r1.stdout
    r2 = launch(4)
    assert r2.returncode == 0, r2.stdout + r2.stderr[-3000:]
    assert "resumed from" in r2.stdout and "(global step 2)" in r2.stdout and "done at global step 4" in r2.stdout
    assert "nan" not in r2.stdout.lower(), r2.stdout
    rd = dtg.train.NewCheckpointReader(dtg.train.latest_checkpoint(ck))
    keys = set(rd.get_variable_to_shape_map())
    assert int(rd.get_tensor("optimizer/step")) == 4 and slot in keys, sorted(keys)[:20]
