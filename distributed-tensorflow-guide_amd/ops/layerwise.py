"""Per-parameter reductions and layer-wise applies over flat groups (csrc/kernels/layerwise.hip) with a CPU
reference path: the primitives of ``FusedLAMB``, ``FusedLARS`` and global-norm clipping (optim/fused.py).

One :class:`LayerwisePlan` covers every flat group of an optimizer: ``rows`` (host int64 [P, 3] = offset in the
row's group, numel, first chunk) and the (row, chunk within row) table with one chunk per ``CHUNK`` elements of a
parameter, built once.  It also owns the scratch of a step, none of which is optimizer state: ``partials``
([2, C]: per-chunk sums of squares), ``norms`` ([P, 2]: the per-parameter sums), ``ratio`` ([P]: trust ratios) and
``cfac`` (the clip factor, a device scalar that stays 1 while nothing clips).  Alignment padding between parameters
belongs to no chunk: it is never read into a norm and never written.

The CPU path keeps the kernels' structure (per-chunk partials, per-parameter sums of a parameter's partials, the
global sum over all partials), so applying a group range by range gives the same bits as applying it whole there too.
"""
import bisect
from collections import namedtuple

import torch
import torch.nn.functional as F

from ._native import lib

CHUNK = 2048      # elements per chunk (= kLwChunk; the extension exports it as LW_CHUNK)
SERIAL = 8        # serial adds per lane per chunk (LW_SERIAL)
TREE_DEPTH = 8    # reduction tree depth of a 256-lane workgroup (LW_TREE_DEPTH)
NONE, LARS, LAMB = 0, 1, 2

# rows [g_lo, g_hi) are the span's group, rows [r_lo, r_hi) / chunks [c_lo, c_hi) the span itself
Span = namedtuple("Span", "g_lo g_hi r_lo r_hi c_lo c_hi")


class LayerwisePlan:
    def __init__(self, groups):
        groups = list(groups)
        if not 1 <= len(groups) <= 4:
            raise ValueError("1..4 flat groups, got %d" % len(groups))
        rows, self._group = [], {}
        chunk = 0
        for g in groups:
            lo = len(rows)
            for off, p in zip(g.offsets, g.params):
                n = p.numel()
                rows.append((int(off), n, chunk))
                chunk += (n + CHUNK - 1) // CHUNK
            self._group[g.name] = (lo, len(rows), [int(o) for o in g.offsets], g.numel)
        self.names = [g.name for g in groups]
        self.group_rows = [self._group[n][1] for n in self.names]
        self.rows = torch.tensor(rows, dtype=torch.int64).reshape(len(rows), 3)
        self.n_rows, self.n_chunks = len(rows), chunk
        self.device = groups[0].master.device
        self.partials = torch.zeros(2 * chunk, dtype=torch.float32, device=self.device)
        self.norms = torch.zeros(len(rows), 2, dtype=torch.float32, device=self.device)
        self.ratio = torch.ones(len(rows), dtype=torch.float32, device=self.device)
        self.cfac = torch.ones(1, dtype=torch.float32, device=self.device)
        self.rows_dev = self.chunks_dev = None
        if self.device.type == "cuda":
            chunks = lib().lw_chunk_table(self.rows)  # validates the rows
            self.rows_dev = self.rows.to(self.device)
            self.chunks_dev = chunks.to(self.device)
        self._rows = rows

    def _chunk0(self, r):
        return self._rows[r][2] if r < self.n_rows else self.n_chunks

    def span(self, g, lo=None, hi=None):
        """The rows / chunks of group ``g`` (an object with ``.name``), or of its element range [lo, hi), which must
        begin and end between parameters (a DataParallel bucket does); a range that cuts a parameter raises."""
        g_lo, g_hi, offs, numel = self._group[g.name]
        if lo is None:
            return Span(g_lo, g_hi, g_lo, g_hi, self._chunk0(g_lo), self._chunk0(g_hi))
        if not 0 <= lo <= hi <= numel:
            raise ValueError("range [%d, %d) is outside group %r of %d elements" % (lo, hi, g.name, numel))
        a, b = bisect.bisect_left(offs, lo), bisect.bisect_left(offs, hi)
        for i, edge in ((a - 1, lo), (b - 1, hi)):
            if i >= 0 and offs[i] < edge < offs[i] + self._rows[g_lo + i][1]:
                raise ValueError("range [%d, %d) of group %r cuts parameter %d ([%d, %d))"
                                 % (lo, hi, g.name, i, offs[i], offs[i] + self._rows[g_lo + i][1]))
        return Span(g_lo, g_hi, g_lo + a, g_lo + b, self._chunk0(g_lo + a), self._chunk0(g_lo + b))

    def _tab(self, s):
        return self.rows, self.rows_dev, self.chunks_dev, s.g_lo, s.g_hi, s.c_lo, s.c_hi

    def _cpu_rows(self, s):
        for r in range(s.r_lo, s.r_hi):
            off, n, c0 = self._rows[r]
            yield r, slice(off, off + n), c0, (n + CHUNK - 1) // CHUNK


def _chunk_sqsum(x, k):
    """fp32 sums of squares of the k chunks of the 1-D fp32 tensor x."""
    return F.pad(x, (0, k * CHUNK - x.numel())).view(k, CHUNK).square().sum(1)


def seg_sqnorm(plan, span, master=None, grad=None):
    """partials[0, c] = sum master^2, partials[1, c] = sum grad^2 over every chunk c of the span (either input may
    be None: its slot stays as it is)."""
    any_ = master if master is not None else grad
    if any_.is_cuda:
        return lib().seg_sqnorm(master, grad, plan.partials, *plan._tab(span))
    C = plan.n_chunks
    for _, sl, c0, k in plan._cpu_rows(span):
        if k and master is not None:
            plan.partials[c0:c0 + k] = _chunk_sqsum(master[sl], k)
        if k and grad is not None:
            plan.partials[C + c0:C + c0 + k] = _chunk_sqsum(grad[sl].float(), k)


def _lamb_u(w, m, v, t, b1, b2, eps, wd):
    return (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps) + wd * w


def lamb_moments(plan, span, master, grad, m, v, hyper, b1, b2, eps, wd, gscale=1.0, clip=False, zero_grad=False):
    """The first LAMB pass over the span: with g^ = grad * gscale * (cfac if clip else 1) updates m and v, writes
    the partials of sum w^2 and sum u^2 (u = m^ / (sqrt(v^) + eps) + wd * w, not stored) and zeroes the gradient
    when asked (it is the last reader)."""
    if master.is_cuda:
        return lib().lamb_moments(master, grad, m, v, hyper, plan.partials, *plan._tab(span), b1, b2, eps, wd, gscale,
                                  plan.cfac if clip else None, zero_grad)
    t = float(hyper[1])
    gs = gscale * float(plan.cfac[0]) if clip else gscale
    C = plan.n_chunks
    for _, sl, c0, k in plan._cpu_rows(span):
        if not k:
            continue
        g = grad[sl].float() * gs
        m[sl].mul_(b1).add_(g, alpha=1 - b1)
        v[sl].mul_(b2).addcmul_(g, g, value=1 - b2)
        plan.partials[c0:c0 + k] = _chunk_sqsum(master[sl], k)
        plan.partials[C + c0:C + c0 + k] = _chunk_sqsum(_lamb_u(master[sl], m[sl], v[sl], t, b1, b2, eps, wd), k)
        if zero_grad:
            grad[sl].zero_()


def lamb_apply(plan, span, master, mirror, m, v, hyper, b1, b2, eps, wd):
    """w -= lr * ratio[row] * u over the span (u recomputed from m, v, w); refreshes the mirror."""
    if master.is_cuda:
        return lib().lamb_apply(master, mirror, m, v, hyper, plan.ratio, *plan._tab(span), b1, b2, eps, wd)
    lr, t = float(hyper[0]), float(hyper[1])
    for r, sl, _, k in plan._cpu_rows(span):
        if not k:
            continue
        master[sl].sub_(_lamb_u(master[sl], m[sl], v[sl], t, b1, b2, eps, wd), alpha=lr * float(plan.ratio[r]))
        if mirror is not None:
            mirror[sl].copy_(master[sl])


def lars_apply(plan, span, master, mirror, grad, mom, hyper, mu, wd, gscale=1.0, clip=False, zero_grad=False):
    """m = mu * m + lr * ratio[row] * (g^ + wd * w); w -= m over the span; refreshes the mirror, zeroes the gradient
    when asked."""
    if master.is_cuda:
        return lib().lars_apply(master, mirror, grad, mom, hyper, plan.ratio, *plan._tab(span), mu, wd, gscale,
                                plan.cfac if clip else None, zero_grad)
    lr = float(hyper[0])
    gs = gscale * float(plan.cfac[0]) if clip else gscale
    for r, sl, _, k in plan._cpu_rows(span):
        if not k:
            continue
        g = grad[sl].float() * gs + wd * master[sl]
        mom[sl].mul_(mu).add_(g, alpha=lr * float(plan.ratio[r]))
        master[sl].sub_(mom[sl])
        if mirror is not None:
            mirror[sl].copy_(master[sl])
        if zero_grad:
            grad[sl].zero_()


def seg_finalize(plan, rule, adapt, wd, clip_norm=None, gscale=1.0, eta=0.0, eps=0.0):
    """One launch over every group.  With ``clip_norm``: cfac = clip_norm / max(gscale * ||g||, clip_norm) from the
    gradient partials of ALL groups.  With ``rule`` LARS / LAMB: norms[p] = the sums of parameter p's partials (in
    chunk order) and ratio[p] -- LARS eta * ||w|| / (gscale * cfac * ||g|| + wd * ||w|| + eps), LAMB ||w|| / ||u||
    -- where p's group adapts and both norms are > 0, else 1.  ``adapt`` / ``wd``: one entry per group."""
    adapt, wd = [bool(a) for a in adapt], [float(x) for x in wd]
    clip = float(clip_norm) if clip_norm is not None else 0.0
    if plan.partials.is_cuda:
        return lib().seg_finalize(plan.partials, plan.rows, plan.rows_dev, plan.chunks_dev, plan.group_rows,
                                  [int(a) for a in adapt], wd, rule, clip, gscale, eta, eps, plan.norms, plan.ratio,
                                  plan.cfac)
    C = plan.n_chunks
    if clip > 0.0:
        gn = gscale * plan.partials[C:].sum().sqrt()
        plan.cfac[0] = clip / torch.clamp(gn, min=clip)
    if rule == NONE:
        return
    c = float(plan.cfac[0])
    gi = 0
    for r, (_, n, c0) in enumerate(plan._rows):
        while r >= plan.group_rows[gi]:
            gi += 1
        k = (n + CHUNK - 1) // CHUNK
        a, b = plan.partials[c0:c0 + k].sum(), plan.partials[C + c0:C + c0 + k].sum()
        plan.norms[r, 0], plan.norms[r, 1] = a, b
        ratio = 1.0
        if adapt[gi] and a > 0 and b > 0:
            n0, n1 = float(a.sqrt()), float(b.sqrt())
            ratio = eta * n0 / (gscale * c * n1 + wd[gi] * n0 + eps) if rule == LARS else n0 / n1
        plan.ratio[r] = ratio
