"""The BERT row, head and loss kernels (csrc/kernels/transformer.hip, heads.hip, softmax_xent.hip) at the
sizes where their stride loops repeat and where the launchers pick the template instantiations that the
hidden=128 model tests never reach.

Two comparison rules:

* exact (``torch.equal``) where the arithmetic is exact: copies, products rounded once, and fp32 sums of
  small integers (bf16 inputs drawn as integers in [-4, 4]: every partial sum is an exact fp32 integer in
  any order, so one dropped or doubled row changes the result);
* per row otherwise: ``err(row) = max_j |out - ref64| / max_j |ref64|`` against an fp64 reference built
  from the same bf16 / fp32 inputs, asserted on the maximum over rows.  A bf16 rounding moves a value by at
  most 2^-8 of itself and these outputs pass at most two (the stored sum s, and the output), so the bound
  is 2^-7 of the row's scale unless a comment next to the constant derives another one.  No bound comes
  from the kernels' own output.

Every check prints its figure before it asserts.
"""
import pytest
import torch

import dtg  # noqa: F401
from dtg.ops import lib, transformer as T

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")

# two bf16 roundings of 2^-8 each.  Largest figures measured on an MI355X: 6.2e-3 for y of the T = 4101 LayerNorm
# (stored sum and output both rounded), 3.9e-3 for every output that is rounded once (the fp64 -> bf16 floor)
BF16_ROW = 2.0 ** -7
F32_EPS = 2.0 ** -24  # fp32 unit roundoff
EPS = 1e-12


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def randn(g, *shape, scale=1.0, dtype=torch.bfloat16):
    return (torch.randn(*shape, device=dev, generator=g) * scale).to(dtype)


def ints(g, *shape, dtype=torch.bfloat16):
    """integers in [-4, 4]: exact in bf16, and every fp32 sum of fewer than 2^22 of them is exact"""
    return torch.randint(-4, 5, shape, device=dev, generator=g).to(dtype)


def row_err(out, ref64):
    d = (out.double() - ref64).abs().amax(-1)
    s = ref64.abs().amax(-1).clamp_min(torch.finfo(torch.float64).tiny)
    return (d / s).max().item()


def check_rows(name, out, ref64, bound=BF16_ROW):
    assert out.shape == ref64.shape, (name, out.shape, ref64.shape)
    assert torch.isfinite(out.float()).all(), name
    e = row_err(out, ref64)
    print(f"[rows] {name}: err={e:.3e} bound={bound:.3e} (fp64->bf16 floor {row_err(ref64.bfloat16(), ref64):.3e})")
    assert e <= bound, (name, e, bound)


def check_cols(name, out, terms64, base64=None, frac=None):
    """Column sums: |out - sum(terms)| <= frac * sum|terms| per column.  frac defaults to 1 / (10 T): a tenth
    of what dropping one average row would change."""
    ref = terms64.sum(0)
    scale = terms64.abs().sum(0)
    if base64 is not None:
        ref = ref + base64
        scale = scale + base64.abs()
    if frac is None:
        frac = 1.0 / (10 * terms64.shape[0])
    e = ((out.double() - ref).abs() / scale.clamp_min(torch.finfo(torch.float64).tiny)).max().item()
    print(f"[cols] {name}: err={e:.3e} bound={frac:.3e}")
    assert torch.isfinite(out).all(), name
    assert e <= frac, (name, e, frac)
    return ref, scale


# ---------------------------------------------------------------------------------------------- LayerNorm
def ln_fwd_ref(h, res, gamma, beta, p_in, seed_in, p_out, seed_out):
    """fp64, nothing rounded on the way: (s, y)"""
    s = h.double()
    if p_in > 0:
        keep = T.dropout_keep(seed_in, h.numel(), p_in, dev).view_as(h)
        s = torch.where(keep, s / (1.0 - p_in), torch.zeros((), dtype=torch.float64, device=dev))
    if res is not None:
        s = s + res.double()
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    y = (s - mean) * torch.rsqrt(var + EPS) * gamma.double() + beta.double()
    if p_out > 0:
        keep = T.dropout_keep(seed_out, h.numel(), p_out, dev).view_as(h)
        y = torch.where(keep, y / (1.0 - p_out), torch.zeros((), dtype=torch.float64, device=dev))
    return s, y


def ln_bwd_ref(dy, s, gamma, mean, rstd, p_in, seed_in, p_out, seed_out):
    """fp64 from the backward kernel's own inputs (dy, the stored s, the saved mean / rstd):
    (ds, dh, dgamma terms, dbeta terms), the terms as [T, H] so a test can sum and scale per column"""
    g = dy.double()
    if p_out > 0:
        keep = T.dropout_keep(seed_out, dy.numel(), p_out, dev).view_as(dy)
        g = torch.where(keep, g / (1.0 - p_out), torch.zeros((), dtype=torch.float64, device=dev))
    r = rstd.double()[:, None]
    xh = (s.double() - mean.double()[:, None]) * r
    gg = g * gamma.double()
    a = gg.mean(-1, keepdim=True)
    b = (gg * xh).mean(-1, keepdim=True)
    ds = r * (gg - a - xh * b)
    dh = ds
    if p_in > 0:
        keep = T.dropout_keep(seed_in, dy.numel(), p_in, dev).view_as(dy)
        dh = torch.where(keep, ds / (1.0 - p_in), torch.zeros((), dtype=torch.float64, device=dev))
    return ds, dh, g * xh, g


def check_ln_stats(name, s_out, mean, rstd):
    """mean / rstd are the statistics of the STORED (bf16) sum.  An fp32 sum of H terms along the kernel's
    chains is within H * 2^-24 of the sum of magnitudes; rstd carries half the variance's relative error plus
    the rsqrt ulps, bounded here by (H + 8) * 2^-24 as well."""
    H = s_out.shape[1]
    s64 = s_out.double()
    m64 = s64.mean(-1)
    r64 = torch.rsqrt(((s64 - m64[:, None]) ** 2).mean(-1) + EPS)
    em = ((mean.double() - m64).abs() / s64.abs().mean(-1)).max().item()
    er = ((rstd.double() - r64).abs() / r64).max().item()
    print(f"[stat] {name}: mean err={em:.3e} rstd err={er:.3e} bound={(H + 8) * F32_EPS:.3e}")
    assert em <= (H + 8) * F32_EPS and er <= (H + 8) * F32_EPS, (name, em, er)


def ln_case(Tn, H, p_in, p_out, with_res, seed, int_dy=True):
    g = gen(seed)
    c = dict(T=Tn, H=H, p_in=p_in, p_out=p_out)
    c["h"] = randn(g, Tn, H)
    c["res"] = randn(g, Tn, H) if with_res else None
    c["gamma"] = torch.rand(H, device=dev, generator=g) + 0.5
    c["beta"] = torch.randn(H, device=dev, generator=g)
    c["dy"] = ints(g, Tn, H) if int_dy else randn(g, Tn, H)
    return c


def ln_run(c, want_dh=True, with_dbias=True, rows=None):
    """forward + backward of case c on the kernels (rows: the backward of that slice of rows only, fed the
    forward's s / mean / rstd of those rows).  The parameter gradients start non-zero: accumulation is part
    of the contract."""
    L = lib()
    if "y" not in c:
        c["y"], c["s"], c["mean"], c["rstd"] = L.ln_fwd(c["h"], c["res"], c["gamma"], c["beta"], EPS, c["p_in"], 11,
                                                        c["p_out"], 13, True)
    r = slice(0, c["T"]) if rows is None else rows
    H = c["H"]
    dg = torch.full((H,), 0.5, device=dev)
    db = torch.full((H,), 3.0, device=dev)
    dz = torch.full((H,), 0.25, device=dev) if with_dbias else None
    ds, dh = L.ln_bwd(c["dy"][r].contiguous(), c["s"][r].contiguous(), c["gamma"], c["mean"][r].contiguous(),
                      c["rstd"][r].contiguous(), dg, db, c["p_in"], 11, c["p_out"], 13, want_dh, dz)
    return dict(ds=ds, dh=dh, dg=dg, db=db, dz=dz, rows=r)


def check_ln_fwd(name, c):
    s64, y64 = ln_fwd_ref(c["h"], c["res"], c["gamma"], c["beta"], c["p_in"], 11, c["p_out"], 13)
    check_rows(name + " s", c["s"], s64)
    check_ln_stats(name, c["s"], c["mean"], c["rstd"])
    check_rows(name + " y", c["y"], y64)


def check_ln_bwd(name, c, o):
    """ds / dh per row, dgamma / dbias per column, dbeta exact (integer dy, no output dropout)"""
    r = o["rows"]
    assert r.start == 0  # the dropout masks are indexed from the first row of the tensor
    ds64, dh64, tg, tb = ln_bwd_ref(c["dy"][r], c["s"][r], c["gamma"], c["mean"][r], c["rstd"][r], c["p_in"], 11,
                                    c["p_out"], 13)
    check_rows(name + " ds", o["ds"], ds64)
    if o["dh"] is not None:
        check_rows(name + " dh", o["dh"], dh64)
    half = torch.full((c["H"],), 0.5, device=dev, dtype=torch.float64)
    check_cols(name + " dgamma", o["dg"], tg, half)
    if c["p_out"] == 0:
        assert torch.equal(o["db"], (tb.sum(0) + 3.0).float()), name + " dbeta"
    else:
        check_cols(name + " dbeta", o["db"], tb, 6 * half)
    if o["dz"] is not None and o["dh"] is not None:
        # the fused branch-bias gradient is defined as the column sum of the STORED (bf16) dh, which the
        # per-row check above ties to fp64; summing the unrounded dh instead would differ by the T rounding
        # errors, more than the tenth of a row this bound allows
        check_cols(name + " dbias", o["dz"], o["dh"].double(), half / 2)
    return ds64, dh64, tg, tb


@pytest.fixture(scope="module")
def ln_big():
    """T = 4096 + 5 rows at H = 768: the grid is capped at 1024 blocks of 4 rows, so the first five waves take
    a second row (the prefetch pipeline and the LDS accumulators carried across rows), 4101 % 4 = 1 exercises
    the row guard, and 1024 partial rows take ln_param_reduce's unrolled 8-loads-in-flight loop."""
    c = ln_case(4101, 768, 0.1, 0.0, True, 21)
    return c, ln_run(c)


def test_ln_multi_row_forward(ln_big):
    c, _ = ln_big
    check_ln_fwd("ln T=4101", c)


def test_ln_multi_row_backward(ln_big):
    c, o = ln_big
    ds64, dh64, tg, tb = check_ln_bwd("ln T=4101", c, o)
    # an fp32 evaluation of the dgamma reference stays inside the per-column bound, so the bound asks nothing
    # of the kernel that fp32 cannot give
    xh32 = (c["s"].float() - c["mean"][:, None]) * c["rstd"][:, None]
    g32 = (c["dy"].float() * xh32).sum(0)
    e32 = ((g32.double() - tg.sum(0)).abs() / tg.abs().sum(0)).max().item()
    print(f"[cols] fp32 evaluation of the dgamma reference: err={e32:.3e} bound={1.0 / (10 * c['T']):.3e}")
    assert e32 <= 1.0 / (10 * c["T"])


def test_ln_rows_do_not_depend_on_the_pass(ln_big):
    """the row math of a wave's second row equals that of a first row: the first 7 rows of the T = 4101 call
    and a T = 7 call on those rows agree bit for bit"""
    c, o = ln_big
    o7 = ln_run(c, rows=slice(0, 7))
    assert torch.equal(o7["ds"], o["ds"][:7])
    assert torch.equal(o7["dh"], o["dh"][:7])
    check_ln_bwd("ln T=7 of 4101", c, o7)
    # the rows a wave took second (4096..4100), recomputed as first rows: ds does not see the dropout index
    tail = ln_run(c, rows=slice(4096, 4101))
    assert torch.equal(tail["ds"], o["ds"][4096:])


@pytest.mark.parametrize("H", [512, 1280, 2048])
def test_ln_instantiations(H):
    """H = 512: ln_bwd<2>; H = 1280: ln_fwd<4> and ln_bwd<8> with 60 KiB of dynamic LDS; H = 2048 (the
    largest the bindings admit): the full <4> / <8> with 96 KiB"""
    c = ln_case(7, H, 0.1, 0.0, True, 22 + H)
    o = ln_run(c)
    check_ln_fwd(f"ln H={H}", c)
    check_ln_bwd(f"ln H={H}", c, o)


def test_ln_both_dropouts():
    c = ln_case(37, 768, 0.1, 0.1, True, 23, int_dy=False)
    o = ln_run(c)
    check_ln_fwd("ln p_in=p_out=0.1", c)
    check_ln_bwd("ln p_in=p_out=0.1", c, o)
    # the masks are there: about a tenth of y is dropped, and dh is zero exactly where the input mask drops
    keep_out = T.dropout_keep(13, c["y"].numel(), 0.1, dev).view_as(c["y"])
    keep_in = T.dropout_keep(11, c["y"].numel(), 0.1, dev).view_as(c["y"])
    assert (c["y"][~keep_out] == 0).all() and (o["dh"][~keep_in] == 0).all()
    assert 0.05 < (~keep_out).float().mean().item() < 0.15


def test_ln_without_branch_gradient():
    """want_dh = False, dbias = None (the want_z == false path): same ds, no dh"""
    c = ln_case(37, 768, 0.1, 0.0, True, 24)
    full = ln_run(c)
    o = ln_run(c, want_dh=False, with_dbias=False)
    assert o["dh"] is None
    assert torch.equal(o["ds"], full["ds"])
    check_ln_bwd("ln want_dh=False", c, o)


def test_ln_stored_sum_is_the_rounded_sum():
    c = ln_case(37, 768, 0.0, 0.0, True, 25)
    o = ln_run(c)
    assert torch.equal(c["s"], (c["h"].float() + c["res"].float()).bfloat16())
    assert o["dh"].data_ptr() == o["ds"].data_ptr()  # no input dropout: dh is ds
    check_ln_fwd("ln p=0", c)
    check_ln_bwd("ln p=0", c, o)


# ------------------------------------------------------------------------------------- attention softmax
@pytest.mark.parametrize("Sk", [7, 64, 192, 1000, 1024])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attn_softmax_rows(Sk, p):
    """Sk = 7, 64: <1>; 192: <4>; 1000, 1024: <16>.  21 rows: a row tail of 1 in the last block."""
    g = gen(30 + Sk)
    B, rpb = 3, 7
    rows = B * rpb
    sc = randn(g, rows, Sk, scale=3.0, dtype=torch.float32)
    am = torch.ones(B, Sk, device=dev)
    nmask = 2 if Sk == 7 else 9
    am[1, Sk - nmask:] = 0  # one batch entry has its last keys masked
    mask = lib().mask_additive(am)
    assert torch.equal(mask, (1.0 - am) * -10000.0)
    P, Pd = lib().attn_softmax_fwd(sc, mask, rpb, p, 77)
    p64 = torch.softmax(sc.double() + mask.double().repeat_interleave(rpb, 0), -1)
    check_rows(f"attn Sk={Sk} p={p} P", P, p64)
    assert (P[rpb:2 * rpb, Sk - nmask:] == 0).all()
    # each row of the stored P sums to 1 within the bf16 bound (one rounding per element: 2^-8 of the sum)
    esum = (P.double().sum(-1) - 1.0).abs().max().item()
    print(f"[rows] attn Sk={Sk} p={p} |sum P - 1|={esum:.3e} bound={BF16_ROW:.3e}")
    assert esum <= BF16_ROW
    if p > 0:
        keep = T.attn_dropout_keep(77, P.numel(), p, dev).view_as(P)
        pd64 = torch.where(keep, p64 / (1.0 - p), torch.zeros((), dtype=torch.float64, device=dev))
        check_rows(f"attn Sk={Sk} p={p} Pd", Pd, pd64)
        assert (Pd[~keep] == 0).all()
    else:
        assert Pd.data_ptr() == P.data_ptr()
    dPd = randn(g, rows, Sk, dtype=torch.float32)
    dS = lib().attn_softmax_bwd(P, Pd, dPd, 0.5)
    pg = Pd.double() * dPd.double()
    ds64 = 0.5 * (pg - P.double() * pg.sum(-1, keepdim=True))
    check_rows(f"attn Sk={Sk} p={p} dS", dS, ds64)


# -------------------------------------------------------------------------------------------------- colsum
@pytest.mark.parametrize("N", [776, 264])
def test_colsum_exact(N):
    """T = 2100 with N = 776 (4 column blocks -> 64 splits, step 512) runs the 4-rows-per-iteration loop of
    the bias-gradient path and then its tail; N = 264 cuts the column guard inside the second block"""
    g = gen(40 + N)
    Tn = 2100
    x = ints(g, Tn, N)
    exact = x.double().sum(0)
    out = torch.arange(N, device=dev, dtype=torch.float32) - 100.0  # fp32 accumulate: the atomic path
    lib().colsum(x, out, True)
    assert torch.equal(out, (exact + torch.arange(N, device=dev) - 100.0).float())
    o1 = torch.full((N,), 7.0, device=dev)  # fp32, not accumulating: partials + reduce, overwrites
    lib().colsum(x, o1, False)
    assert torch.equal(o1, exact.float())
    sel = torch.randint(0, 2, (Tn,), device=dev, generator=g)
    o2 = torch.full((2, N), 7.0, device=dev, dtype=torch.bfloat16)  # bf16 with a 2-way selector
    lib().colsum(x, o2.view(-1), False, sel, 2)
    ref = torch.stack([x.double()[sel == v].sum(0) for v in range(2)])
    assert torch.equal(o2, ref.float().bfloat16())  # the exact fp32 sum, rounded once


# ---------------------------------------------------------------------------------------------- embeddings
@pytest.mark.parametrize("with_tt", [True, False])
def test_emb_fwd_rows(with_tt):
    g = gen(50)
    V, H, B, S = 50, 768, 6, 7  # 42 rows: a row tail of 2
    word, pos, typ = randn(g, V, H), randn(g, S + 3, H), randn(g, 2, H)
    ids = torch.randint(0, V, (B * S,), device=dev, generator=g)
    ids[0], ids[1] = 0, V - 1
    tt = torch.randint(0, 2, (B * S,), device=dev, generator=g) if with_tt else None
    s = lib().emb_fwd(ids, tt, word, pos, typ, S)
    ref = word.double()[ids] + pos.double()[torch.arange(B * S, device=dev) % S]
    if with_tt:
        ref = ref + typ.double()[tt]
    check_rows(f"emb_fwd tt={with_tt}", s, ref)  # an fp32 sum of three, rounded once


def emb_bwd_inputs(g, Tn, H, V, special):
    ids = torch.randint(0, V, (Tn,), device=dev, generator=g)
    for i, v in enumerate(special):
        ids[3 * i + 1] = v
    ds = ints(g, Tn, H)
    g0 = ints(g, V, H)
    ref = g0.double().index_add(0, ids, ds.double())
    assert ref.abs().max().item() <= 256  # integers up to 256 are exact in bf16: the result is exact
    return ids, ds, g0, ref


def test_emb_word_bwd_sorted_exact():
    ids, ds, g0, ref = emb_bwd_inputs(gen(51), 300, 768, 70, [0, 69])
    gW = g0.clone()
    srt, perm = torch.sort(ids)
    lib().emb_word_bwd(ds, srt, perm, gW)
    assert torch.equal(gW, ref.bfloat16())


def test_emb_word_bwd_owned_partial_tile_exact():
    """V = 70: the last vocabulary tile holds rows 64..69 only; H = 1024: the 128 KiB LDS accumulator"""
    ids, ds, g0, ref = emb_bwd_inputs(gen(52), 300, 1024, 70, [0, 63, 64, 69])
    gW = g0.clone()
    assert lib().emb_word_bwd_owned(ds, ids, gW) is True
    assert torch.equal(gW, ref.bfloat16())


def test_emb_word_bwd_owned_refuses_what_does_not_fit():
    ids, ds, g0, _ = emb_bwd_inputs(gen(53), 40, 1032, 70, [0, 69])
    gW = g0.clone()
    assert lib().emb_word_bwd_owned(ds, ids, gW) is False
    assert torch.equal(gW, g0)


# --------------------------------------------------------------------------------------------------- heads
@pytest.mark.parametrize("H", [768, 1024])
def test_gather_rows_exact(H):
    g = gen(60 + H)
    B, P, S = 3, 7, 16  # 21 rows: a row tail of 1
    src = randn(g, B * S, H)
    pos = torch.randint(0, S, (B, P), device=dev, generator=g)
    pos[0, 3:] = 0      # padded positions
    pos[1, :] = S - 1   # one repeated position
    out = lib().gather_rows(src, pos, S)
    idx = (torch.arange(B, device=dev)[:, None] * S + pos).reshape(-1)
    assert torch.equal(out, src.index_select(0, idx))


@pytest.mark.parametrize("H", [768, 1024])
def test_scatter_cls_rows_exact(H):
    """pos = None: row i of src lands on row i * S; onto zeros that is a copy, and no other row changes"""
    g = gen(61 + H)
    B, S = 5, 6
    dst = randn(g, B * S, H)
    dst[::S] = 0
    before = dst.clone()
    src = randn(g, B, H)
    lib().scatter_rows_add(dst, None, src, S)
    exp = before.clone()
    exp[::S] = src
    assert torch.equal(dst, exp)


@pytest.mark.parametrize("H", [768, 1024])
def test_nsp_loss_fwd_bwd(H):
    """B = 37: the 16-row loops of both kernels repeat (3 rows for some waves, 2 for others); H > 512: the
    64-chunk column loop of the forward repeats.  The reference is the documented semantics: mean over B of
    the 2-way cross-entropy plus `extra`; dlogits = (p - onehot) * gout / B."""
    g = gen(62 + H)
    B = 37
    pooled = torch.tanh(torch.randn(B, H, device=dev, generator=g)).bfloat16()
    wn = randn(g, 2, H, scale=0.1)
    bn = torch.randn(2, device=dev, generator=g)
    labels = torch.randint(0, 2, (B,), device=dev, generator=g)
    labels[0], labels[1] = 0, 1
    extra = torch.tensor([1.75], device=dev)
    out, probs = lib().nsp_loss_fwd(pooled, wn, bn, labels, extra)
    x, w = pooled.double(), wn.double()
    logits = x @ w.t() + bn.double()
    lse = torch.logsumexp(logits, -1)
    p64 = torch.softmax(logits, -1)
    loss64 = (lse - logits.gather(1, labels[:, None])[:, 0]).mean() + 1.75
    # a logit is an fp32 dot product: H/64 fused multiply-adds per lane, 6 shuffle levels and the bias, each
    # rounding at most 2^-24 of the sum of |terms|; a probability moves by at most the two logits' errors,
    # plus a few ulps of the fast exp and the division
    delta = (H // 64 + 8) * F32_EPS * (x.abs() @ w.abs().t()).sum(-1).max().item()
    tol_p = 2 * delta + 8 * F32_EPS
    ep = (probs.double() - p64).abs().max().item()
    el = abs(out.item() - loss64.item())
    tol_l = 2 * delta + 16 * F32_EPS * max(1.0, abs(loss64.item()))
    print(f"[nsp] H={H} probs err={ep:.3e} bound={tol_p:.3e}; loss err={el:.3e} bound={tol_l:.3e}")
    assert ep <= tol_p and el <= tol_l
    # backward from the kernel's own probabilities; gwn / gbn accumulate onto what is there
    gout = torch.tensor([0.5], device=dev)
    gwn0 = randn(g, 2, H, scale=0.05)
    gbn0 = torch.tensor([0.3, -0.2], device=dev)
    gwn, gbn = gwn0.clone(), gbn0.clone()
    dpre = lib().nsp_loss_bwd(pooled, wn, probs, labels, gout, gwn, gbn)
    dl = (probs.double() - torch.nn.functional.one_hot(labels, 2).double()) * (0.5 / B)
    check_rows(f"nsp H={H} dpre", dpre, (dl @ w) * (1.0 - x * x))
    terms = dl[:, :, None] * x[:, None, :]  # [B, 2, H]
    ref_w = gwn0.double() + terms.sum(0)
    mag_w = gwn0.double().abs() + terms.abs().sum(0)
    # one bf16 rounding of the result (2^-8, factor 2), plus the fp32 accumulation over the B rows
    ew = ((gwn.double() - ref_w).abs() - (BF16_ROW * ref_w.abs() + (B + 16) * F32_EPS * mag_w)).max().item()
    print(f"[nsp] H={H} gwn worst excess over its per-column bound: {ew:.3e}")
    assert ew <= 0
    ref_b = gbn0.double() + dl.sum(0)
    eb = ((gbn.double() - ref_b).abs() / (gbn0.double().abs() + dl.abs().sum(0))).max().item()
    print(f"[nsp] H={H} gbn err={eb:.3e} bound={(B + 4) * F32_EPS:.3e}")
    assert eb <= (B + 4) * F32_EPS  # B sequential fp32 additions of terms that carry two roundings each


def test_row_sum_exact():
    x = ints(gen(63), 5000, dtype=torch.float32)  # n > 1024: the stride loop repeats, with a tail
    out = lib().row_sum(x, 0.125)
    assert out.item() == x.double().sum().item() * 0.125


@pytest.mark.parametrize("n", [1003, 4096 * 256 * 8 + 1003])
def test_mul_bf16_exact(n):
    """1003: 125 vectors and a 3-element scalar tail; the large one wraps the 4096-block grid-stride loop"""
    g = gen(64)
    a, b = randn(g, n), randn(g, n)
    assert torch.equal(lib().mul_bf16(a, b), (a.float() * b.float()).bfloat16())


@pytest.mark.parametrize("dt", [torch.int64, torch.float32])
def test_mask_additive_exact(dt):
    m = torch.randint(0, 2, (17, 59), device=dev, generator=gen(65)).to(dt)  # 1003 elements
    out = lib().mask_additive(m)
    assert out.dtype == torch.float32 and out.shape == m.shape
    assert torch.equal(out, (1.0 - m.float()) * -10000.0)


def test_zero_byte_tail():
    big = torch.full((2048,), 1.5, device=dev, dtype=torch.bfloat16)
    lib().zero_(big[:1001])  # 2002 bytes: 125 vectors and 2 tail bytes
    assert (big[:1001] == 0).all() and (big[1001:] == 1.5).all()


# ------------------------------------------------------------------------------------ softmax cross-entropy
XENT_PATHS = [("fp32", 257), ("fp32", 1000), ("bf16", 1001), ("bf16", 1008), ("bf16-unaligned", 1008)]
# lse = M + log(S): M is exact; S sums V <= 1008 terms exp(x - M), each within ~4e-6 relative (the fast exp
# rounds x * log2(e) to fp32: up to 40 * 1.45 * 2^-24 = 3.5e-6 for arguments down to -40, plus its ulps)
# along chains of about 14 fp32 additions (8e-7); log S keeps that as an absolute error; the fast log and the
# final addition at |lse| <= 16 add about 1.5e-6.  About 1e-5 in all; the bound is twice that.
XENT_LSE_TOL = 2e-5
# a probability exp(x - lse) inherits lse's absolute error as a relative one, plus the exp's own 4e-6; the
# row's scale is at least the largest probability, so 2.4e-5 of it, factor 2
XENT_F32_GRAD = 5e-5


def xent_logits(path, B, V, g, neg_inf=False, labels=None):
    """logits of the path's dtype; 'bf16-unaligned' is a contiguous view that starts 2 bytes into its storage,
    so the launcher's alignment test sends a vector-eligible shape down the scalar path"""
    x = torch.randn(B, V, device=dev, generator=g) * 3
    if neg_inf:  # a third of the non-label columns: masked out
        cols = torch.arange(V, device=dev)
        m = (cols % 3 == 1)[None, :] & (cols[None, :] != labels[:, None])
        x = x.masked_fill(m, float("-inf"))
    if path == "fp32":
        return x
    if path == "bf16":
        return x.bfloat16()
    store = torch.empty(B * V + 8, device=dev, dtype=torch.bfloat16)
    view = store[1:1 + B * V].view(B, V)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 2
    return view


def xent_labels(B, V, g):
    labels = torch.randint(0, V, (B,), device=dev, generator=g)
    labels[0], labels[1], labels[2], labels[5] = 0, V - 1, -1, -1
    return labels


def check_xent(name, x, labels, scale, gval):
    """forward with want_grad, and the backward from the saved lse, against fp64, row by row"""
    L = lib()
    B, V = x.shape
    loss, dx, lse = L.softmax_xent(x, labels, scale, True)
    x64 = x.double()
    lse64 = torch.logsumexp(x64, -1)
    valid = labels >= 0
    lab = labels.clamp_min(0)
    loss64 = torch.where(valid, lse64 - x64.gather(1, lab[:, None])[:, 0], torch.zeros_like(lse64))
    el = (lse.double() - lse64).abs().max().item()
    eo = (loss.double() - loss64).abs().max().item()
    print(f"[xent] {name}: lse err={el:.3e} loss err={eo:.3e} bound={XENT_LSE_TOL:.3e}")
    assert torch.isfinite(lse).all() and torch.isfinite(loss).all(), name
    assert el <= XENT_LSE_TOL and eo <= XENT_LSE_TOL, (name, el, eo)
    assert (loss[~valid] == 0).all()
    onehot = torch.zeros(B, V, device=dev, dtype=torch.float64)
    onehot[valid, labels[valid]] = 1.0
    soft = torch.exp(x64 - lse64[:, None])
    g = torch.tensor(gval, device=dev)
    dxb = L.softmax_xent_bwd(x, labels, lse, g, scale)
    bound = XENT_F32_GRAD if x.dtype == torch.float32 else BF16_ROW
    for what, got, sc in (("fwd dx", dx, scale), ("bwd dx", dxb, scale * gval)):
        assert got.dtype == x.dtype and got.shape == x.shape
        assert (got[~valid] == 0).all(), (name, what)  # ignored rows: exactly zero
        if valid.any():
            check_rows(f"xent {name} {what}", got[valid], ((soft - onehot) * sc)[valid], bound)
    return x64, dx, lse


@pytest.mark.parametrize("path,V", XENT_PATHS)
def test_softmax_xent_rows(path, V):
    g = gen(70 + V)
    B = 9
    labels = xent_labels(B, V, g)
    x = xent_logits(path, B, V, g)
    check_xent(f"{path} V={V}", x, labels, 0.25, 0.5)


@pytest.mark.parametrize("path,V", XENT_PATHS)
def test_softmax_xent_forward_grad_is_the_backward(path, V):
    """want_grad: the forward's dx is a second evaluation of the backward's expression with g = 1"""
    g = gen(71 + V)
    B = 9
    labels = xent_labels(B, V, g)
    x = xent_logits(path, B, V, g)
    _, dx, lse = lib().softmax_xent(x, labels, 0.25, True)
    dxb = lib().softmax_xent_bwd(x, labels, lse, torch.ones((), device=dev), 0.25)
    assert torch.equal(dx, dxb)


@pytest.mark.parametrize("path,V", XENT_PATHS)
def test_softmax_xent_minus_inf_columns(path, V):
    """-inf in a third of the non-label columns (an additive vocabulary mask): finite loss and lse that match
    fp64, and exactly zero gradient at those columns -- on the vector path and on both scalar paths"""
    g = gen(72 + V)
    B = 9
    labels = xent_labels(B, V, g)
    x = xent_logits(path, B, V, g, neg_inf=True, labels=labels.clamp_min(0))
    x64, dx, _ = check_xent(f"{path} V={V} -inf", x, labels, 0.25, 0.5)
    assert torch.isinf(x64).sum().item() >= B * (V // 3 - 1)
    assert (dx[torch.isinf(x64)] == 0).all()


def test_softmax_xent_every_row_ignored():
    g = gen(73)
    B, V = 9, 1008
    x = xent_logits("bf16", B, V, g)
    labels = torch.full((B,), -1, device=dev)
    loss, dx, lse = lib().softmax_xent(x, labels, 1.0, True)
    assert (loss == 0).all() and (dx == 0).all()
    assert (lse.double() - torch.logsumexp(x.double(), -1)).abs().max().item() <= XENT_LSE_TOL
    dxb = lib().softmax_xent_bwd(x, labels, lse, torch.ones((), device=dev), 1.0)
    assert (dxb == 0).all()
