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

    def _extend_rows(self, ids, cache, n_new):
        """ids [B, T] at positions ``cache.lens0 + cache.t + i`` -> hidden rows [B, T, H] after the last layer; the
        cache grows by T (by ``n_new``, int32 [B] on the device, when given).  At most 64 tokens per record go through
        one ``attn_extend``, so a longer T runs in pieces."""
        cfg, e = self.cfg, self.emb
        B, Tn = ids.shape
        native = self._decode_native(ids)
        out = []
        for s in range(0, Tn, 64):
            piece = ids[:, s:s + 64].contiguous()
            Tp = piece.shape[1]
            nn = None if n_new is None else (n_new - s).clamp(0, Tp)
            x = T.emb_fwd_span(piece, cache.lens0, cache.t, e.word, e.pos, e.tok_type)
            if native:
                x = bert_fused.lib().ln_fwd(x, None, e.ln_g, e.ln_b, cfg.eps, 0.0, 0, 0.0, 0, False)[0]
            else:
                x = T.layer_norm_ref(x, None, e.ln_g.to(x.dtype), e.ln_b.to(x.dtype), cfg.eps)
            for i, layer in enumerate(self.layers):
                x, _ = bert_fused.infer_layer(
                    layer, x, cfg, lambda qkv: T.attn_extend(qkv, cache.lens0, cache.t, cache.max_len, cache.k[i],
                                                             cache.v[i], Tp, cfg.window, nn)[0])
            cache.advance(Tp, nn)
            out.append(x.view(B, Tp, -1))
        return out[0] if len(out) == 1 else torch.cat(out, 1)

    @torch.no_grad()
    def extend(self, ids, cache, n_new=None):
        """Several more tokens per record: ids [B, T] sit at positions ``cache.lens0 + cache.t + i`` -> [B, T, V]
        logits of the token after each.  Every layer runs on B * T rows, with ``attn_extend`` (which appends the
        tokens' keys and values to the cache) in place of the attention; nothing is read back from the device.
        ``n_new`` (B ints, or int32 [B] on the device): record b has only ``n_new[b]`` tokens; the logits of its other
        rows mean nothing, and the cache's bound ``max_len`` still grows by T."""
        cfg = self.cfg
        if cache.quantised:
            raise ValueError("extend: the quantised (FP8) cache is served by prefill (chunk = 0) and decode_step only")
        if ids.dim() != 2 or ids.shape[0] != cache.B or ids.shape[1] < 1:
            raise ValueError("extend: ids must be [%d, T >= 1] (got %r)" % (cache.B, tuple(ids.shape)))
        if cache.max_len + ids.shape[1] > min(cache.S_max, cfg.max_position):
            raise ValueError("extend: positions %d .. %d are beyond the cache (%d) or the position table (%d)"
                             % (cache.max_len, cache.max_len + ids.shape[1] - 1, cache.S_max, cfg.max_position))
        if n_new is not None:
            n_new = torch.as_tensor(n_new, dtype=torch.int32, device=ids.device)
        hm = self._extend_rows(ids, cache, n_new)
        return bert_fused.infer_head(self, hm.reshape(-1, hm.shape[-1])).view(ids.shape[0], ids.shape[1], -1)

    def _prefill_chunked(self, ids, lengths, cache, chunk):
        """``prefill`` through ``extend``'s rows, ``chunk`` tokens per record at a time: no padding to 64, so any prompt
        up to ``max_position`` tokens, and activations of B * chunk rows."""
        cfg = self.cfg
        B, top = ids.shape[0], max(lengths)
        if top > min(cache.S_max, cfg.max_position):
            raise ValueError("prefill: the prompt (%d tokens) exceeds the cache (%d) or the position table (%d)"
                             % (top, cache.S_max, cfg.max_position))
        cache.reset([0] * B)
        lens = torch.tensor(lengths, dtype=torch.int32, device=ids.device)
        last = None
        for s in range(0, top, chunk):
            piece = ids[:, s:min(s + chunk, top)]
            hm = self._extend_rows(piece, cache, (lens - s).clamp(0, piece.shape[1]))
            here = [b for b, n in enumerate(lengths) if s < n <= s + chunk]  # records that end in this piece
            if here:
                last = hm.new_empty(B, hm.shape[-1]) if last is None else last
                rows = torch.tensor(here, device=ids.device)
                last[rows] = hm[rows, torch.tensor([lengths[b] - 1 - s for b in here], device=ids.device)]
        return bert_fused.infer_head(self, last)

    @torch.no_grad()
    def prefill(self, ids, lengths, cache, chunk=0):
        """The prompts' forward -> [B, V] logits at each record's last real position, leaving every layer's keys and
        values in ``cache``.  ids [B, S0] (anything at and beyond a record's length), lengths: B host ints >= 1.  The
        prompt is padded to a multiple of 64 for the causal kernels and key-masked by length; no dropout.  With
        ``chunk > 0`` the prompt goes through ``attn_extend`` instead, ``chunk`` tokens per record at a time, without
        that padding."""
        cfg = self.cfg
        B, S0 = ids.shape
        lengths = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if len(lengths) != B or min(lengths) < 1 or max(lengths) > S0:
            raise ValueError("prefill: %d records need %d lengths in [1, %d] (got %r)" % (B, B, S0, lengths))
        if chunk > 0:
            if cache.quantised:
                raise ValueError("prefill: chunk > 0 goes through attn_extend, which does not serve the quantised "
                                 "(FP8) cache")
            return self._prefill_chunked(ids, lengths, cache, chunk)
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
            T.kv_cache_fill(qkv, cache.lens0, cache.k[i], cache.v[i], B, S, cfg.heads, cache.k_scale[i],
                            cache.v_scale[i])
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
                                                         cache.v[i], cfg.window, cache.k_scale[i],
                                                         cache.v_scale[i])[0])
        cache.t += 1
        return bert_fused.infer_head(self, x)

    def generate(self, ids, lengths, max_new_tokens, eos_id=None, prefill_chunk=0, cache_dtype=None):
        """Greedy continuation -> [B, max_new_tokens] int64: ``prefill`` on the prompts (ids [B, S0], lengths: B host
        ints; ``prefill_chunk`` is its ``chunk``), then one ``decode_step`` per token, in eval mode under no_grad (the
        training flag is restored).  With ``eos_id`` a record's tokens after its first ``eos_id`` are ``eos_id``.
        ``cache_dtype``: the cache's dtype (default: the weights'); ``torch.float8_e4m3fn`` is the quantised cache, which
        takes no ``prefill_chunk``."""
        cfg = self.cfg
        lengths = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if max_new_tokens < 1:
            raise ValueError("generate: max_new_tokens must be positive (got %d)" % max_new_tokens)
        if prefill_chunk > 0 and cache_dtype == torch.float8_e4m3fn:
            raise ValueError("generate: prefill_chunk > 0 goes through attn_extend, which does not serve the quantised "
                             "(FP8) cache")
        S_max = max(lengths) + max_new_tokens
        if S_max > cfg.max_position:
            raise ValueError("generate: prompt (%d) + max_new_tokens (%d) exceeds max_position = %d"
                             % (max(lengths), max_new_tokens, cfg.max_position))
        was_training = self.training
        self.eval()
        try:
            cache = KVCache(cfg, ids.shape[0], S_max, ids.device, cache_dtype or self.emb.word.dtype)
            tok = torch.argmax(self.prefill(ids, lengths, cache, prefill_chunk), -1)
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
