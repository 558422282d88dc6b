"""The KV cache of incremental decoding (csrc/kernels/attention_decode.hip, ops/transformer.py::attn_decode).

Per layer ``k[i]`` / ``v[i]`` are ``[B, heads, S_max, head_dim]``: one head's keys are one contiguous stream of rows.
Record b holds ``lens0[b] + t`` keys: ``lens0`` (int32 on the device) are the prompt lengths ``prefill`` left, ``t``
counts the decode steps since, on the host -- the decode loop never reads a device value back.  ``max_len0`` is the
host's copy of ``max(lens0)``, from which the launches size their grids.

``dtype=torch.float8_e4m3fn`` is the quantised cache (csrc/kernels/attention_decode_fp8.hip): ``k`` / ``v`` hold e4m3
codes, and ``k_scale[i]`` / ``v_scale[i]`` (fp32 ``[B, heads, S_max]``, None for every other dtype) one scale per row.
"""
import torch


class KVCache:
    def __init__(self, cfg, B, S_max, device=None, dtype=torch.bfloat16):
        if B < 1 or S_max < 1:
            raise ValueError("KVCache: B and S_max must be positive (got %d, %d)" % (B, S_max))
        self.B, self.S_max, self.heads = B, S_max, cfg.heads
        shape = (B, cfg.heads, S_max, cfg.hidden // cfg.heads)
        self.k = [torch.zeros(shape, device=device, dtype=dtype) for _ in range(cfg.layers)]
        self.v = [torch.zeros(shape, device=device, dtype=dtype) for _ in range(cfg.layers)]
        self.quantised = dtype == torch.float8_e4m3fn
        self.k_scale, self.v_scale = ([torch.ones(shape[:3], device=device, dtype=torch.float32)
                                       if self.quantised else None for _ in range(cfg.layers)] for _ in range(2))
        self.lens0 = torch.zeros(B, device=device, dtype=torch.int32)
        self.max_len0 = 0
        self.t = 0

    @property
    def max_len(self):
        """>= every record's cached length, on the host"""
        return self.max_len0 + self.t

    def reset(self, lengths):
        """New prompts: ``lengths`` (a list of B ints) become ``lens0`` and the step count returns to 0."""
        if len(lengths) != self.B:
            raise ValueError("KVCache: %d lengths for %d records" % (len(lengths), self.B))
        self.lens0.copy_(torch.tensor(lengths, dtype=torch.int32))
        self.max_len0 = max(lengths)
        self.t = 0

    def advance(self, T, n_new=None):
        """After ``T`` more rows per record went through ``attn_extend``: every record grew by T (``t += T``), or, with
        ``n_new`` (int32 [B] on the device, each in [0, T]), record b grew by ``n_new[b]``: ``lens0 += n_new`` on the
        device and the host's bound ``max_len0 += T``.  Nothing is read back."""
        if n_new is None:
            self.t += T
        else:
            self.lens0 += n_new
            self.max_len0 += T
