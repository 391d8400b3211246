"""Model zoo (N11): ResNet-18/34/50/101/152, BERT-base/large (+ a tiny test size), ViT-B/16,
GPT-2 small/medium/large (+ a tiny test size), Llama-family SmolLM-135M/360M/1.7B (+ a tiny test size)."""
from __future__ import annotations

import torch.nn as nn

from .resnet import ResNet, resnet18, resnet34, resnet50, resnet101, resnet152  # noqa: F401
from .bert import BertConfig, BertForSequenceClassification, bert_base, bert_large, bert_tiny  # noqa: F401
from .bert import BertForPreTraining, bert_base_pretraining, bert_large_pretraining, bert_tiny_pretraining  # noqa: F401
from .vit import ViTConfig, ViTForImageClassification, vit_b16  # noqa: F401
from .gpt2 import GPT2Config, GPT2LMHeadModel, KVCache, gpt2, gpt2_medium, gpt2_large, gpt2_tiny  # noqa: F401
from .llama import LlamaKVCache  # noqa: F401
from .llama import LlamaConfig, LlamaForCausalLM, llama_tiny, smollm_135m, smollm_360m, smollm_1p7b  # noqa: F401
from .layers import cast_params, convert_sync_batchnorm  # noqa: F401

_REGISTRY = {
    "resnet18": resnet18, "resnet34": resnet34, "resnet50": resnet50,
    "resnet101": resnet101, "resnet152": resnet152,
    "bert_base": bert_base, "bert_large": bert_large, "bert_tiny": bert_tiny,
    "bert_base_pretraining": bert_base_pretraining, "bert_large_pretraining": bert_large_pretraining,
    "bert_tiny_pretraining": bert_tiny_pretraining,
    "vit_b16": vit_b16,
    "gpt2": gpt2, "gpt2_medium": gpt2_medium, "gpt2_large": gpt2_large, "gpt2_tiny": gpt2_tiny,
    "llama_tiny": llama_tiny, "smollm_135m": smollm_135m, "smollm_360m": smollm_360m, "smollm_1p7b": smollm_1p7b,
}


def available_models():
    return sorted(_REGISTRY)


def build_model(name: str, num_classes: int = 1000, dropout: float = 0.1, image_size: int = 224) -> nn.Module:
    if name not in _REGISTRY:
        raise KeyError(f"unknown model {name!r}; have {available_models()}")
    if name.startswith("bert") and name.endswith("_pretraining"):
        return _REGISTRY[name](dropout=dropout)      # MLM + NSP heads: no label count
    if name.startswith("bert"):
        return _REGISTRY[name](num_labels=num_classes, dropout=dropout)
    if name.startswith("gpt"):
        return _REGISTRY[name](dropout=dropout)           # causal LM: no label count
    if name.startswith(("llama", "smollm")):
        return _REGISTRY[name]()                          # causal LM without dropout: neither is passed
    if name.startswith("vit"):
        return _REGISTRY[name](num_classes=num_classes, dropout=dropout, image_size=image_size)
    return _REGISTRY[name](num_classes=num_classes)


def count_params(m: nn.Module) -> int:
    return sum(p.numel() for p in m.parameters())
