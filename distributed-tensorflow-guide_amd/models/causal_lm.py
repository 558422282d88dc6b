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
