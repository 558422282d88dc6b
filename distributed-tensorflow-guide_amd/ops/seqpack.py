"""Packed token rows: BERT without padding (csrc/kernels/seqpack.hip).

A batch of ``B`` records of lengths ``len[b] <= S`` has ``T = sum(len)`` token rows.  The padded layout is
``[B * S, W]`` (row ``b * S + s``); the packed layout is ``[T_alloc, W]`` with record ``b`` at rows ``cu[b] ..
cu[b] + len[b] - 1`` and ``T_alloc`` = ``T`` rounded up to ``ROW_ALIGN`` = 64 rows (``ops/gemm.py`` wants ``M % 8 ==
0``, and the row kernels get whole workgroups).  The tail rows ``T .. T_alloc - 1`` belong to no token: ``seq_unpad``
writes zeros there, so every gradient that enters the packed encoder is exactly zero on them.

    cu = seq_offsets(lengths, S)                       int32 [B + 1], exclusive prefix sum of clamp(len, 0, S)
    seq_pad(x [T_alloc, W], cu, B, S)                  -> [B * S, W], zeros on every padding row
    seq_unpad(x [B * S, W], cu, B, S, T_alloc)         -> [T_alloc, W], zeros on the tail rows
    emb_fwd_packed(ids, tt, word, pos, typ, cu, T_alloc)   = seq_unpad(emb_fwd(ids, tt, ...))
    seq_gather_ids(ids, tt, cu, T_alloc)               -> (ids [T_alloc], token types [T_alloc]); tail id 0
    emb_pos_bwd_packed(ds [T_alloc, H], cu, B, S, gP)  gP[p] += sum over b with len[b] > p of ds[cu[b] + p]
    attn_packed_fwd(qkv [T_alloc, 3H], cu, B, S, nh, p, seed)   -> (ctx [T_alloc, H], lse [nh, T_alloc]): the fused
    attn_packed_bwd(qkv, ctx, dout, lse, cu, B, S, nh, p, seed) -> dqkv [T_alloc, 3H]     attention, the length as mask
    attn_packed_long_fwd / attn_packed_long_bwd                 the same at 128 < S <= 512 (backward: dKV + dQ launches)

A packed row whose index would fall outside ``[0, T_alloc)`` -- a host ``T_alloc`` smaller than the device lengths
imply -- is skipped: never read, never written.  GPU bf16 tensors go through the HIP kernels (a missing extension is
an error).  The kernels take 16-byte accesses only: a row width that is no multiple of 8, an unaligned base or a
non-contiguous view is refused by the binding with a message naming the operand (no scalar path; make it
``.contiguous()`` first).  Everything else -- CPU tensors, the fp32 / fp64 oracle -- takes the ``*_ref`` mirrors, the
same rules in PyTorch operations, which are also what the kernels are tested against.

``SeqPack`` carries one batch's geometry; ``pad_rows`` / ``unpad_rows`` are the autograd forms (each one's backward is
the other).
"""
import numpy as np
import torch

from ._native import lib
from .transformer import attention_ref

ROW_ALIGN = 64


def _native(x):
    return x.is_cuda and x.dtype == torch.bfloat16


# ---- mirrors ------------------------------------------------------------------------------------------------------
def seq_offsets_ref(lengths, S):
    n = lengths.to(torch.int64).clamp(0, S)
    return torch.cat([n.new_zeros(1), torch.cumsum(n, 0)]).to(torch.int32)


def _coords(cu, B, S, T_alloc):
    """-> (t [B, S] int64 packed row of every padded coordinate, valid [B, S] bool)."""
    cu = cu.to(torch.int64)
    base = cu[:-1].view(B, 1)
    n = (cu[1:] - cu[:-1]).clamp(0, S).view(B, 1)
    s = torch.arange(S, device=cu.device, dtype=torch.int64).view(1, S)
    t = base + s
    return t, (s < n) & (t >= 0) & (t < T_alloc)


def seq_pad_ref(src, cu, B, S):
    T_alloc = src.shape[0]
    t, valid = _coords(cu, B, S, T_alloc)
    dst = src.new_zeros((B * S,) + tuple(src.shape[1:]))
    v = valid.reshape(-1)
    dst[v] = src[t.reshape(-1)[v]]
    return dst


def seq_unpad_ref(src, cu, B, S, T_alloc):
    t, valid = _coords(cu, B, S, T_alloc)
    dst = src.new_zeros((T_alloc,) + tuple(src.shape[1:]))
    v = valid.reshape(-1)
    dst[t.reshape(-1)[v]] = src[v]
    return dst


def emb_fwd_packed_ref(ids, token_types, word, pos, typ, cu, T_alloc):
    """The kernel's sum ``word + (pos + type)``, in fp32 for bf16 tables, on the real positions; zero tail rows."""
    B, S = ids.shape
    up = torch.float32 if word.dtype == torch.bfloat16 else word.dtype
    rest = pos[:S].to(up).unsqueeze(0)
    if token_types is not None:
        rest = rest + typ[token_types].to(up)
    x = (word[ids].to(up) + rest).to(word.dtype)
    return seq_unpad_ref(x.reshape(B * S, -1), cu, B, S, T_alloc)


def seq_gather_ids_ref(ids, token_types, cu, T_alloc):
    B, S = ids.shape
    io = seq_unpad_ref(ids.reshape(-1), cu, B, S, T_alloc)
    return io, (seq_unpad_ref(token_types.reshape(-1), cu, B, S, T_alloc) if token_types is not None else None)


def emb_pos_bwd_packed_ref(ds, cu, B, S, gP):
    up = torch.float32 if ds.dtype == torch.bfloat16 else ds.dtype
    add = seq_pad_ref(ds, cu, B, S).view(B, S, -1).to(up).sum(0)
    gP[:S] = (gP[:S].to(up) + add).to(gP.dtype)


# ---- ops ----------------------------------------------------------------------------------------------------------
def seq_offsets(lengths, S):
    if lengths.is_cuda:
        return lib().seq_offsets(lengths.contiguous(), int(S))
    return seq_offsets_ref(lengths, S)


def seq_pad(src, cu, B, S, out=None):
    if _native(src):
        return lib().seq_pad(src, cu, int(B), int(S), out)
    res = seq_pad_ref(src, cu, B, S)
    return res if out is None else out.copy_(res)


def seq_unpad(src, cu, B, S, T_alloc, out=None):
    if _native(src):
        return lib().seq_unpad(src, cu, int(B), int(S), int(T_alloc), out)
    res = seq_unpad_ref(src, cu, B, S, T_alloc)
    return res if out is None else out.copy_(res)


def emb_fwd_packed(ids, token_types, word, pos, typ, cu, T_alloc, out=None):
    if _native(word):
        return lib().emb_fwd_packed(ids.contiguous(), None if token_types is None else token_types.contiguous(),
                                    word, pos, typ, cu, int(T_alloc), out)
    res = emb_fwd_packed_ref(ids, token_types, word, pos, typ, cu, T_alloc)
    return res if out is None else out.copy_(res)


def seq_gather_ids(ids, token_types, cu, T_alloc):
    if ids.is_cuda:
        io, to = lib().seq_gather_ids(ids.contiguous(), None if token_types is None else token_types.contiguous(),
                                      cu, int(T_alloc))
        return io, (to if token_types is not None else None)
    return seq_gather_ids_ref(ids, token_types, cu, T_alloc)


def emb_pos_bwd_packed(ds, cu, B, S, gP):
    """Adds into ``gP`` (the position table's gradient), like ``emb_pos_bwd``."""
    if _native(ds):
        lib().emb_pos_bwd_packed(ds, cu, gP, int(B), int(S))
    else:
        emb_pos_bwd_packed_ref(ds, cu, B, S, gP)


# ---- fused attention on packed rows (csrc/kernels/attention_packed.hip) -------------------------------------------
def attn_packed_ref(qkv, cu, B, S, nh, p=0.0, seed=0):
    """The mirror: ``seq_unpad_ref(attention_ref(seq_pad_ref(qkv), length mask from cu))`` -- qkv [T_alloc, 3H] ->
    context [T_alloc, H], zeros on the rows of no record.  Plain PyTorch operations, differentiable by autograd: the
    CPU path and the oracle of the kernels.  The dropout index is the padded ``((b * nh + h) * S + q) * S + key``."""
    T_alloc = qkv.shape[0]
    _, valid = _coords(cu, B, S, T_alloc)
    mask_add = (1.0 - valid.to(torch.float32)) * -10000.0
    ctx = attention_ref(seq_pad_ref(qkv, cu, B, S), mask_add, B, S, nh, p, seed)
    return seq_unpad_ref(ctx, cu, B, S, T_alloc)


def attn_packed_supported(S, dh):
    """Whether the packed attention kernels take this shape (head dim 64, S = 64 or 128)."""
    return bool(lib().attn_packed_supported(int(S), int(dh)))


def attn_packed_fwd(qkv, cu, B, S, nh, p, seed, out=None):
    """qkv [T_alloc, 3 * nh * 64] -> (ctx [T_alloc, nh * 64], lse fp32 [nh, T_alloc]): ``attn_fused_fwd`` on the
    packed rows, the length as the mask; zeros on the tail rows.  CPU / fp32 tensors take the mirror (lse None)."""
    if _native(qkv):
        ctx, lse = lib().attn_packed_fwd(qkv, cu, int(B), int(S), int(nh), float(p), int(seed), out)
        return ctx, lse
    res = attn_packed_ref(qkv, cu, B, S, nh, p, seed)
    return (res if out is None else out.copy_(res)), None


def attn_packed_bwd(qkv, ctx, dout, lse, cu, B, S, nh, p, seed, dbias=None, out=None):
    """-> dqkv [T_alloc, 3 * nh * 64], zeros on the tail rows; ``dbias`` (fp32 [3 * nh * 64]) gets the column sums
    of dqkv ADDED.  CPU / fp32 tensors: autograd through the mirror."""
    if _native(qkv):
        return lib().attn_packed_bwd(qkv, ctx, dout, lse, cu, int(B), int(S), int(nh), float(p), int(seed), dbias, out)
    with torch.enable_grad():
        x = qkv.detach().requires_grad_(True)
        (res,) = torch.autograd.grad(attn_packed_ref(x, cu, B, S, nh, p, seed), x, dout)
    if dbias is not None:
        dbias += res.sum(0).to(dbias.dtype)
    return res if out is None else out.copy_(res)


def attn_packed_long_supported(S, dh):
    """Whether the long packed attention kernels take this shape (head dim 64, S % 64 == 0, 128 < S <= 512)."""
    return bool(lib().attn_packed_long_supported(int(S), int(dh)))


def attn_packed_long_fwd(qkv, cu, B, S, nh, p, seed, out=None):
    """``attn_packed_fwd`` at 128 < S <= 512: the same kernel over ceil(S / 128) query blocks per record and head.
    CPU / fp32 tensors take the mirror (lse None), which knows no limit on S."""
    if _native(qkv):
        ctx, lse = lib().attn_packed_long_fwd(qkv, cu, int(B), int(S), int(nh), float(p), int(seed), out)
        return ctx, lse
    res = attn_packed_ref(qkv, cu, B, S, nh, p, seed)
    return (res if out is None else out.copy_(res)), None


def attn_packed_long_bwd(qkv, ctx, dout, lse, cu, B, S, nh, p, seed, dbias=None, out=None):
    """``attn_packed_bwd`` at 128 < S <= 512: a dKV and a dQ launch that each recompute P from the LSE.  CPU / fp32
    tensors: autograd through the mirror."""
    if _native(qkv):
        return lib().attn_packed_long_bwd(qkv, ctx, dout, lse, cu, int(B), int(S), int(nh), float(p), int(seed), dbias,
                                          out)
    return attn_packed_bwd(qkv, ctx, dout, lse, cu, B, S, nh, p, seed, dbias, out)


# ---- one batch's geometry -----------------------------------------------------------------------------------------
class SeqPack:
    """``B`` records of ``S`` positions: ``lengths`` int32 [B] and ``cu`` int32 [B + 1] on the device,
    ``host_lengths`` a small numpy copy, and the Python ints ``T`` = sum(clamp(len, 0, S)) and ``T_alloc`` (``T``
    rounded up to 64 rows, at least 64) computed from the host copy: no device read anywhere."""
    __slots__ = ("B", "S", "lengths", "cu", "T", "T_alloc", "host_lengths")

    def __init__(self, B, S, lengths, cu, T, T_alloc, host_lengths):
        self.B, self.S, self.lengths, self.cu, self.T, self.T_alloc = B, S, lengths, cu, T, T_alloc
        self.host_lengths = host_lengths

    @classmethod
    def from_lengths(cls, lengths_device, host_lengths, S):
        """lengths_device: int32 [B] where the model runs; host_lengths: the same values on the host (anything
        ``numpy.asarray`` takes; it is copied).  One ``seq_offsets`` launch."""
        host = np.array(host_lengths, dtype=np.int64, copy=True).reshape(-1)
        S = int(S)
        if lengths_device.dtype != torch.int32 or tuple(lengths_device.shape) != (host.size,):
            raise ValueError("lengths_device must be int32 [%d], got %s %s" % (host.size, lengths_device.dtype,
                                                                              tuple(lengths_device.shape)))
        T = int(np.clip(host, 0, S).sum())
        T_alloc = max(ROW_ALIGN, -(-T // ROW_ALIGN) * ROW_ALIGN)
        return cls(host.size, S, lengths_device, seq_offsets(lengths_device, S), T, T_alloc, host)

    def chunk(self, i, A):
        """The pack of micro-batch ``i`` of ``A`` equal slices along the batch (gradient accumulation): its ``T``
        from ``host_lengths``, its offsets from one ``seq_offsets`` launch on the slice of ``lengths``."""
        i, A = int(i), int(A)
        if A < 1 or not 0 <= i < A or self.B % A:
            raise ValueError("chunk(%d, %d) of a pack of %d records" % (i, A, self.B))
        if A == 1:
            return self
        b = self.B // A
        return SeqPack.from_lengths(self.lengths[i * b:(i + 1) * b], self.host_lengths[i * b:(i + 1) * b], self.S)

    def __repr__(self):
        return "SeqPack(B=%d, S=%d, T=%d, T_alloc=%d)" % (self.B, self.S, self.T, self.T_alloc)


# ---- autograd -----------------------------------------------------------------------------------------------------
class _PadRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pack):
        ctx.pack = pack
        return seq_pad(x.contiguous(), pack.cu, pack.B, pack.S)

    @staticmethod
    def backward(ctx, dy):
        p = ctx.pack
        return seq_unpad(dy.contiguous(), p.cu, p.B, p.S, p.T_alloc), None


class _UnpadRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pack):
        ctx.pack = pack
        return seq_unpad(x.contiguous(), pack.cu, pack.B, pack.S, pack.T_alloc)

    @staticmethod
    def backward(ctx, dy):
        p = ctx.pack
        return seq_pad(dy.contiguous(), p.cu, p.B, p.S), None


def pad_rows(x, pack):
    """[T_alloc, W] -> [B * S, W]; the backward is ``seq_unpad``: zero gradient on the tail rows."""
    if x.shape[0] != pack.T_alloc:
        raise ValueError("pad_rows: %d rows, the pack has T_alloc %d" % (x.shape[0], pack.T_alloc))
    return _PadRows.apply(x, pack)


def unpad_rows(x, pack):
    """[B * S, W] -> [T_alloc, W]; the backward is ``seq_pad``: zero gradient on the padding rows."""
    if x.shape[0] != pack.B * pack.S:
        raise ValueError("unpad_rows: %d rows, the pack has B * S = %d" % (x.shape[0], pack.B * pack.S))
    return _UnpadRows.apply(x, pack)
