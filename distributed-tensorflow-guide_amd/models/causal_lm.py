"""A decoder-only language model on BERT's blocks: the embeddings, ``cfg.layers`` post-LN layers whose attention is
causal (csrc/kernels/attention_causal.hip on the fused path -- attention_causal_packed.hip on packed rows --,
``attention_ref(causal=True)`` on the reference path; with ``cfg.window = W`` a position sees the last W tokens only:
csrc/kernels/attention_window.hip on padded rows, which a pack re-pads around, and ``attention_ref(window=W)``), and
the masked-LM head (transform + tied decoder + cross-entropy) applied to EVERY position ``t`` with label
``ids[b, t + 1]``: the next-token loss.  No next-sentence head, no new kernels for the head and no parameters beyond
``BertForPreTraining``'s (its pooler / NSP weights stay in the checkpoint and receive no gradient).
"""
import dataclasses

import torch
import torch.nn.functional as F

from ..ops import seqpack
from ..ops import transformer as T
from . import bert_fused
from .bert import BertConfig, BertForPreTraining
from .kv_cache import KVCache


class CausalLM(BertForPreTraining):
    def __init__(self, cfg=None, seed=1234):
        super().__init__(dataclasses.replace(cfg or BertConfig.base(), causal=True), seed)

    @staticmethod
    def next_token_labels(ids, attention_mask=None):
        """[B, S] labels: ``ids[b, t + 1]`` at position t, -1 at a record's last real position and on padding."""
        labels = torch.full_like(ids, -1)
        labels[:, :-1] = ids[:, 1:]
        if attention_mask is not None:
            labels[:, :-1][attention_mask[:, 1:] == 0] = -1
        return labels

    def hidden_states(self, ids, attention_mask=None, pack=None, p_h=0.0, p_a=0.0):
        """-> [B * S, H] after the last layer (token types all 0); position t depends on tokens <= t only."""
        B, S = ids.shape
        cfg = self.cfg
        mask_add = T.mask_additive(attention_mask) if attention_mask is not None else None
        tt = torch.zeros_like(ids)
        if self.fused_ok(ids):
            seq = bert_fused.embeddings(self, ids, tt, S, p_h, self._seed(0, 0), pack)
            for i, layer in enumerate(self.layers):
                seq = bert_fused.encoder_layer(layer, seq, mask_add, B, S, cfg, p_h, p_a, self._seed(i + 1, 1),
                                               self._seed(i + 1, 2), self._seed(i + 1, 3), pack)
            return seq if pack is None else seqpack.pad_rows(seq, pack)
        return self._reference_encoder(ids, tt, mask_add, p_h, p_a, pack)

    def logits(self, ids, attention_mask=None):
        """-> [B * S, V] next-token logits, no dropout; the head in plain torch (no evaluation wiring yet)."""
        hm = self.hidden_states(ids, attention_mask)
        dt = hm.dtype
        t = F.gelu(F.linear(hm, self.mlm_w, self.mlm_b.to(dt)), approximate="tanh")
        t = T.layer_norm_ref(t, None, self.mlm_ln_g.to(dt), self.mlm_ln_b.to(dt), self.cfg.eps)
        return F.linear(t, self.emb.word, self.mlm_bias.to(dt))

    # -- incremental decoding (models/kv_cache.py, csrc/kernels/attention_decode.hip) --------------------------
    def _decode_native(self, ids):
        """True: the HIP path (GPU, bf16 weights); False: the torch mirrors (CPU, or fp32 / fp64 weights).  A bf16
        model on the GPU that is not on the fused path (``fused`` off, a head dim other than 64, ...) is an error."""
        if not (ids.is_cuda and self.emb.word.dtype == torch.bfloat16):
            return False
        cfg = self.cfg
        if not self.fused_ok(ids.new_empty(1, 64)) or cfg.hidden != cfg.heads * 64:
            raise RuntimeError("incremental decoding needs the fused path (fused = %r, head dim %s; 64 required)"
                               % (self.fused, cfg.hidden / cfg.heads))
        return True

    @torch.no_grad()
    def prefill(self, ids, lengths, cache):
        """The prompts' forward -> [B, V] logits at each record's last real position, leaving every layer's keys and
        values in ``cache``.  ids [B, S0] (anything at and beyond a record's length), lengths: B host ints >= 1.  The
        prompt is padded to a multiple of 64 for the causal kernels and key-masked by length; no dropout."""
        cfg = self.cfg
        B, S0 = ids.shape
        lengths = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if len(lengths) != B or min(lengths) < 1 or max(lengths) > S0:
            raise ValueError("prefill: %d records need %d lengths in [1, %d] (got %r)" % (B, B, S0, lengths))
        S = (S0 + 63) // 64 * 64
        if max(lengths) > cache.S_max or S > cfg.max_position:
            raise ValueError("prefill: the prompt (%d tokens, padded to %d) exceeds the cache (%d) or the position "
                             "table (%d)" % (max(lengths), S, cache.S_max, cfg.max_position))
        native = self._decode_native(ids)
        cache.reset(lengths)
        ids = F.pad(ids, (0, S - S0))
        real = torch.arange(S, device=ids.device).unsqueeze(0) < cache.lens0.unsqueeze(1)
        mask_add = T.mask_additive(real.float())
        if native:
            bert_fused._causal_attn(S, 3 * cfg.hidden, cfg.heads, cfg.window)
            seq = bert_fused.embeddings(self, ids, torch.zeros_like(ids), S, 0.0, 0)
        else:
            e = self.emb
            seq = (e.word[ids] + e.pos[:S].unsqueeze(0) + e.tok_type[0]).reshape(B * S, -1)
            seq = T.layer_norm_ref(seq, None, e.ln_g.to(seq.dtype), e.ln_b.to(seq.dtype), cfg.eps)

        def attn(qkv):
            if cfg.window:
                return T.attn_window_fwd(qkv, mask_add, B, S, cfg.heads, cfg.window)[0]
            return T.attn_causal_fwd(qkv, mask_add, B, S, cfg.heads)[0]

        for i, layer in enumerate(self.layers):
            seq, qkv = bert_fused.infer_layer(layer, seq, cfg, attn)
            T.kv_cache_fill(qkv, cache.lens0, cache.k[i], cache.v[i], B, S, cfg.heads)
        last = (cache.lens0.long() - 1).view(B, 1)  # the head runs on these B rows only
        if native:
            hm = bert_fused.lib().gather_rows(seq, last, S)
        else:
            hm = seq.view(B, S, -1)[torch.arange(B, device=ids.device), last.view(-1)]
        return bert_fused.infer_head(self, hm)

    @torch.no_grad()
    def decode_step(self, ids_new, cache):
        """One more token per record: ids_new [B] sits at position ``cache.lens0 + cache.t`` -> [B, V] logits of the
        token after it.  Every layer runs on B rows, with ``attn_decode`` (which appends the token's keys and values
        to the cache) in place of the attention; nothing is read back from the device."""
        cfg = self.cfg
        if cache.max_len >= min(cache.S_max, cfg.max_position):
            raise ValueError("decode_step: position %d is beyond the cache (%d) or the position table (%d)"
                             % (cache.max_len, cache.S_max, cfg.max_position))
        e = self.emb
        x = T.emb_fwd_at(ids_new, cache.lens0, cache.t, e.word, e.pos, e.tok_type)
        if self._decode_native(ids_new):
            x = bert_fused.lib().ln_fwd(x, None, e.ln_g, e.ln_b, cfg.eps, 0.0, 0, 0.0, 0, False)[0]
        else:
            x = T.layer_norm_ref(x, None, e.ln_g.to(x.dtype), e.ln_b.to(x.dtype), cfg.eps)
        for i, layer in enumerate(self.layers):
            x, _ = bert_fused.infer_layer(
                layer, x, cfg, lambda qkv: T.attn_decode(qkv, cache.lens0, cache.t, cache.max_len, cache.k[i],
                                                         cache.v[i], cfg.window)[0])
        cache.t += 1
        return bert_fused.infer_head(self, x)

    def generate(self, ids, lengths, max_new_tokens, eos_id=None):
        """Greedy continuation -> [B, max_new_tokens] int64: ``prefill`` on the prompts (ids [B, S0], lengths: B host
        ints), then one ``decode_step`` per token, in eval mode under no_grad (the training flag is restored).  With
        ``eos_id`` a record's tokens after its first ``eos_id`` are ``eos_id``."""
        cfg = self.cfg
        lengths = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if max_new_tokens < 1:
            raise ValueError("generate: max_new_tokens must be positive (got %d)" % max_new_tokens)
        S_max = max(lengths) + max_new_tokens
        if S_max > cfg.max_position:
            raise ValueError("generate: prompt (%d) + max_new_tokens (%d) exceeds max_position = %d"
                             % (max(lengths), max_new_tokens, cfg.max_position))
        was_training = self.training
        self.eval()
        try:
            cache = KVCache(cfg, ids.shape[0], S_max, ids.device, self.emb.word.dtype)
            tok = torch.argmax(self.prefill(ids, lengths, cache), -1)
            out = [tok]
            for _ in range(max_new_tokens - 1):
                tok = torch.argmax(self.decode_step(tok, cache), -1)
                out.append(tok)
        finally:
            self.train(was_training)
        out = torch.stack(out, 1)
        if eos_id is not None:
            out = torch.where((out == eos_id).cumsum(1) > 0, eos_id, out)
        return out

    def forward(self, ids, attention_mask=None, num_valid=None, pack=None):
        """Next-token cross-entropy, summed over the labelled positions and divided by ``num_valid`` (default: the
        count of labels >= 0, read back to the host).  ids / attention_mask: [B, S]; pack: as in
        ``BertForPreTraining.forward`` (a causal layer runs the packed causal kernels on the packed rows; with
        ``bert_fused._PACKED_ATTN`` off it re-pads around the padded causal kernels)."""
        pack = self._check_pack(pack if pack is not None else self.seq_pack, ids)
        if self.training:
            self._step += 1
        labels = self.next_token_labels(ids, attention_mask).reshape(-1)
        nv = int((labels >= 0).sum()) if num_valid is None else num_valid
        p_h = self.cfg.dropout if self.training else 0.0
        p_a = self.cfg.attn_dropout if self.training else 0.0
        seq = self.hidden_states(ids, attention_mask, pack, p_h, p_a)
        if self.fused_ok(ids):
            return bert_fused.mlm_head(self, seq, labels, nv)
        return self._reference_mlm(seq, labels, nv)
