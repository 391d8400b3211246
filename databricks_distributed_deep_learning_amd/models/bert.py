"""BERT-base / BERT-large encoder + sequence-classification or pretraining (MLM + NSP) heads (post-LN).

Parameter-for-parameter equivalent to HF ``BertForSequenceClassification``
(109,483,778 params for base with 2 labels) except that Q, K and V are one fused
``[3·hidden, hidden]`` projection (a single MFMA GEMM writing the packed QKV the
attention kernel reads).  ``from_hf_state_dict`` / ``to_hf_state_dict`` convert
between the two naming schemes so HF checkpoints load one-to-one.

The reference's NLP half is an empty README (``notebooks/nlp/README.md``); the
workload is defined by BASELINE.json:9,11.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..ops.bridge import GradBridge
from .layers import Dropout, Embedding, LayerNorm, Linear


def _bridge(h: torch.Tensor):
    return GradBridge() if (torch.is_grad_enabled() and h.requires_grad) else None


@dataclass
class BertConfig:
    vocab_size: int = 30522
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    max_position_embeddings: int = 512
    type_vocab_size: int = 2
    layer_norm_eps: float = 1e-12
    hidden_dropout_prob: float = 0.1
    attention_probs_dropout_prob: float = 0.1
    initializer_range: float = 0.02
    num_labels: int = 2

    @classmethod
    def base(cls, **kw):
        return cls(**kw)

    @classmethod
    def large(cls, **kw):
        d = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096)
        d.update(kw)
        return cls(**d)


class BertEmbeddings(nn.Module):
    def __init__(self, c: BertConfig):
        super().__init__()
        std = c.initializer_range
        self.word_embeddings = Embedding(c.vocab_size, c.hidden_size, std)
        self.position_embeddings = Embedding(c.max_position_embeddings, c.hidden_size, std)
        self.token_type_embeddings = Embedding(c.type_vocab_size, c.hidden_size, std)
        self.LayerNorm = LayerNorm(c.hidden_size, c.layer_norm_eps)
        self.dropout = Dropout(c.hidden_dropout_prob)

    def forward(self, input_ids, token_type_ids=None):
        B, S = input_ids.shape
        we = self.word_embeddings(input_ids)
        if token_type_ids is None:
            # position rows + token type 0 in one native pass; its backward writes both parameters'
            # gradient slots directly (ops/glue.py)
            r = ops.embedding_residual(self.position_embeddings.weight, self.token_type_embeddings.weight, S)
        else:
            r = self.position_embeddings.weight[:S].unsqueeze(0) + self.token_type_embeddings(token_type_ids)
        h = self.LayerNorm(we, residual=r)
        return self.dropout(h)


class BertLayer(nn.Module):
    def __init__(self, c: BertConfig):
        super().__init__()
        H, I, std = c.hidden_size, c.intermediate_size, c.initializer_range
        self.num_heads = c.num_attention_heads
        self.attn_dropout = c.attention_probs_dropout_prob
        self.qkv = Linear(H, 3 * H, init_std=std)
        self.attn_out = Linear(H, H, init_std=std)
        self.attn_ln = LayerNorm(H, c.layer_norm_eps)
        self.ffn_in = Linear(H, I, act="gelu", init_std=std)
        self.ffn_out = Linear(I, H, init_std=std)
        self.ffn_ln = LayerNorm(H, c.layer_norm_eps)
        self.dropout = Dropout(c.hidden_dropout_prob)
        for lin in (self.qkv, self.attn_out, self.ffn_in, self.ffn_out):
            nn.init.zeros_(lin.bias)

    def forward(self, h, mask: Optional[torch.Tensor] = None):
        # hidden dropout fused into the post-LN kernels: LN(dropout(sublayer) + h); each
        # residual gradient is bridged into the dgrad epilogue of the Linear that also
        # reads h (qkv / ffn_in) instead of an autograd add
        br1, br2 = _bridge(h), None
        qkv = self.qkv(h, grad_residual=br1)
        ctx = ops.attention(qkv, self.num_heads, mask, self.attn_dropout, self.training)
        h = self.attn_ln(self.attn_out(ctx), residual=h, dropout=self.dropout.p, residual_grad_to=br1)
        br2 = _bridge(h)
        # ffn_in's GELU backward runs in ffn_out's dgrad epilogue (ffn_out is its only consumer)
        f = self.ffn_out(self.ffn_in(h, grad_residual=br2), fuse_dgelu=True)
        return self.ffn_ln(f, residual=h, dropout=self.dropout.p, residual_grad_to=br2)


class BertModel(nn.Module):
    # ZeRO-1 gather waits (parallel/ddp.py): only dispatches to its children's forwards
    _ddl_gather_router = True

    def __init__(self, c: BertConfig):
        super().__init__()
        self.config = c
        self.embeddings = BertEmbeddings(c)
        self.layers = nn.ModuleList([BertLayer(c) for _ in range(c.num_hidden_layers)])
        self.pooler = Linear(c.hidden_size, c.hidden_size, act="tanh", init_std=c.initializer_range)
        nn.init.zeros_(self.pooler.bias)

    def forward(self, input_ids, attention_mask=None, token_type_ids=None):
        mask_bias = None
        if attention_mask is not None:
            mask_bias = (1.0 - attention_mask.float()) * -10000.0
        h = self.embeddings(input_ids, token_type_ids)
        for layer in self.layers:
            h = layer(h, mask_bias)
        pooled = self.pooler(ops.first_token(h))
        return h, pooled


class BertForSequenceClassification(nn.Module):
    def __init__(self, c: BertConfig):
        super().__init__()
        self.config = c
        self.bert = BertModel(c)
        self.dropout = Dropout(c.hidden_dropout_prob)
        self.classifier = Linear(c.hidden_size, c.num_labels, init_std=c.initializer_range)
        nn.init.zeros_(self.classifier.bias)

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None):
        _, pooled = self.bert(input_ids, attention_mask, token_type_ids)
        logits = self.classifier(self.dropout(pooled))
        if labels is not None:
            return ops.cross_entropy(logits, labels), logits
        return logits


class BertForPreTraining(nn.Module):
    """BERT with the two pretraining heads (HF ``BertForPreTraining``, 110,106,428 parameters for
    base): masked-LM -- transform (dense + GELU, LayerNorm), then a decoder whose weight IS the word
    embedding table (tied; registered once, under the embedding) with its own bias -- and
    next-sentence prediction on the pooled output.

    ``masked_lm_positions [B, P]`` (a fixed P per batch; padded slots carry label -100 and
    conventionally position 0): only those ``B * P`` rows are gathered and run through the MLM head,
    so the ``[rows, vocab]`` logits cover P rows per sequence instead of S.  Valid positions must be
    unique within a sequence (``ops.gather_rows``).  Without positions ``masked_lm_labels`` is
    ``[B, S]`` (HF style, -100 = not a target) and the head runs on every token.

    Returns ``(loss, (mlm_logits, nsp_logits))``: the loss is the sum of the objectives whose
    labels are given (None without any); ``mlm_logits`` is None whenever MLM labels are given -- the
    fused head (``ops.linear_cross_entropy``) never hands out the vocabulary-wide logits."""

    def __init__(self, c: BertConfig):
        super().__init__()
        self.config = c
        self.bert = BertModel(c)
        H, std = c.hidden_size, c.initializer_range
        self.mlm_dense = Linear(H, H, act="gelu", init_std=std)
        self.mlm_ln = LayerNorm(H, c.layer_norm_eps)
        self.mlm_bias = nn.Parameter(torch.zeros(c.vocab_size))
        self.seq_relationship = Linear(H, 2, init_std=std)
        nn.init.zeros_(self.mlm_dense.bias)
        nn.init.zeros_(self.seq_relationship.bias)

    @property
    def decoder_weight(self) -> nn.Parameter:
        # looked up on use: ``cast_params`` / ``.to()`` may replace the Parameter object
        return self.bert.embeddings.word_embeddings.weight

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, masked_lm_positions=None,
                masked_lm_labels=None, next_sentence_label=None):
        h, pooled = self.bert(input_ids, attention_mask, token_type_ids)
        nsp_logits = self.seq_relationship(pooled)
        labels = masked_lm_labels.reshape(-1) if masked_lm_labels is not None else None
        if masked_lm_positions is not None:
            rows = ops.gather_rows(h, masked_lm_positions, labels, -100)
        else:
            rows = h.reshape(-1, h.shape[-1])
        t = self.mlm_ln(self.mlm_dense(rows))
        loss = mlm_logits = None
        if labels is not None:
            loss = ops.linear_cross_entropy(t, self.decoder_weight, self.mlm_bias, labels, -100,
                                            defer_weight_ready=True)
        else:
            mlm_logits = ops.linear(t, self.decoder_weight, self.mlm_bias)
        if next_sentence_label is not None:
            nsp = ops.cross_entropy(nsp_logits, next_sentence_label)
            loss = nsp if loss is None else loss + nsp
        return loss, (mlm_logits, nsp_logits)


def bert_base(num_labels: int = 2, dropout: float = 0.1, **kw) -> BertForSequenceClassification:
    return BertForSequenceClassification(BertConfig.base(num_labels=num_labels, hidden_dropout_prob=dropout,
                                                         attention_probs_dropout_prob=dropout, **kw))


def bert_large(num_labels: int = 2, dropout: float = 0.1, **kw) -> BertForSequenceClassification:
    return BertForSequenceClassification(BertConfig.large(num_labels=num_labels, hidden_dropout_prob=dropout,
                                                          attention_probs_dropout_prob=dropout, **kw))


def bert_tiny(num_labels: int = 2, dropout: float = 0.1, **kw) -> BertForSequenceClassification:
    """2 layers, hidden 128, 2 heads: the BERT code path at test / smoke size."""
    d = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512,
             vocab_size=1024, max_position_embeddings=128)
    d.update(kw)
    return BertForSequenceClassification(BertConfig(num_labels=num_labels, hidden_dropout_prob=dropout,
                                                    attention_probs_dropout_prob=dropout, **d))


def bert_base_pretraining(dropout: float = 0.1, **kw) -> BertForPreTraining:
    return BertForPreTraining(BertConfig.base(hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout, **kw))


def bert_large_pretraining(dropout: float = 0.1, **kw) -> BertForPreTraining:
    return BertForPreTraining(BertConfig.large(hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout, **kw))


def bert_tiny_pretraining(dropout: float = 0.1, **kw) -> BertForPreTraining:
    """``bert_tiny``'s encoder with the pretraining heads (vocabulary 1024)."""
    d = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512,
             vocab_size=1024, max_position_embeddings=128)
    d.update(kw)
    return BertForPreTraining(BertConfig(hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout, **d))


# ------------------------------------------------------------ HF conversion
# HF ``BertForPreTraining`` head names <-> ours (``cls.predictions.decoder.*`` is the tied embedding
# table and ``cls.predictions.bias`` again: checked and dropped on import, re-emitted on export)
_HF_HEAD_MAP = {
    "cls.predictions.transform.dense.weight": "mlm_dense.weight",
    "cls.predictions.transform.dense.bias": "mlm_dense.bias",
    "cls.predictions.transform.LayerNorm.weight": "mlm_ln.weight",
    "cls.predictions.transform.LayerNorm.bias": "mlm_ln.bias",
    "cls.predictions.bias": "mlm_bias",
    "cls.seq_relationship.weight": "seq_relationship.weight",
    "cls.seq_relationship.bias": "seq_relationship.bias",
}
_HF_TIED = {"cls.predictions.decoder.weight": "bert.embeddings.word_embeddings.weight",
            "cls.predictions.decoder.bias": "cls.predictions.bias"}
_HF_LAYER_MAP = {
    "attention.output.dense": "attn_out",
    "attention.output.LayerNorm": "attn_ln",
    "intermediate.dense": "ffn_in",
    "output.dense": "ffn_out",
    "output.LayerNorm": "ffn_ln",
}


def from_hf_state_dict(sd: dict, num_layers: int) -> dict:
    """HF ``BertForSequenceClassification`` / ``BertForPreTraining`` state dict -> this model's."""
    out = {}
    for k, v in sd.items():
        if k.startswith("bert.embeddings.") and "position_ids" not in k and "token_type_ids" not in k:
            out[k] = v
        elif k.startswith("bert.pooler.dense."):
            out[k.replace("bert.pooler.dense.", "bert.pooler.")] = v
        elif k.startswith("classifier."):
            out[k] = v
        elif k in _HF_HEAD_MAP:
            out[_HF_HEAD_MAP[k]] = v
        elif k in _HF_TIED:
            if _HF_TIED[k] in sd and not torch.equal(v, sd[_HF_TIED[k]]):
                raise ValueError(f"{k} is not tied to {_HF_TIED[k]}: this model shares the two")
    for i in range(num_layers):
        p = f"bert.encoder.layer.{i}."
        for t in ("weight", "bias"):
            out[f"bert.layers.{i}.qkv.{t}"] = torch.cat(
                [sd[p + f"attention.self.{n}.{t}"] for n in ("query", "key", "value")], 0)
            for hf, ours in _HF_LAYER_MAP.items():
                out[f"bert.layers.{i}.{ours}.{t}"] = sd[p + f"{hf}.{t}"]
    return out


def to_hf_state_dict(sd: dict, num_layers: int) -> dict:
    out = {}
    for k, v in sd.items():
        if k.startswith("bert.embeddings.") or k.startswith("classifier."):
            out[k] = v
        elif k.startswith("bert.pooler."):
            out[k.replace("bert.pooler.", "bert.pooler.dense.")] = v
    ours_to_hf = {v: k for k, v in _HF_HEAD_MAP.items()}
    for k, v in sd.items():
        if k in ours_to_hf:
            out[ours_to_hf[k]] = v
    if "mlm_bias" in sd:
        out["cls.predictions.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"]
        out["cls.predictions.decoder.bias"] = sd["mlm_bias"]
    for i in range(num_layers):
        p = f"bert.encoder.layer.{i}."
        for t in ("weight", "bias"):
            q, kk, vv = sd[f"bert.layers.{i}.qkv.{t}"].chunk(3, 0)
            out[p + f"attention.self.query.{t}"] = q
            out[p + f"attention.self.key.{t}"] = kk
            out[p + f"attention.self.value.{t}"] = vv
            for hf, ours in _HF_LAYER_MAP.items():
                out[p + f"{hf}.{t}"] = sd[f"bert.layers.{i}.{ours}.{t}"]
    return out
