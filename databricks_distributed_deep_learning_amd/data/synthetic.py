"""Synthetic, device-resident data loaders (north-star N3).

Replaces the Petastorm / Delta Lake reader named in BASELINE.json:5.  Batches
are generated once, directly on the rank's device, with per-rank seeds (so
ranks see different data, as a rank-sharded real loader would), and cycled —
no host->device copy and no host work in the training hot loop.

Image batches are NHWC, pre-normalised with the ImageNet mean/std the reference
uses (``notebooks/cv/onnx_experiments.py:63``), labels uniform in
[0, num_classes).  Token batches are ids uniform in [0, vocab) with an
all-ones attention mask by default (optionally random right-padding).
"""
from __future__ import annotations

from typing import Iterator, Optional, Tuple

import torch

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _gen(device, seed: int) -> torch.Generator:
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return g


class SyntheticImageNet:
    def __init__(self, batch_size: int, image_size: int = 224, num_classes: int = 1000,
                 device: Optional[torch.device] = None, dtype: torch.dtype = torch.float32,
                 rank: int = 0, seed: int = 1234, pool: int = 4, steps_per_epoch: int = 0,
                 channels_last: bool = True):
        self.batch_size, self.image_size, self.num_classes = batch_size, image_size, num_classes
        self.device = device or torch.device("cpu")
        self.dtype = dtype
        self.steps_per_epoch = steps_per_epoch
        g = _gen(self.device, seed * 1000 + rank)
        shape = (batch_size, image_size, image_size, 3) if channels_last else (batch_size, 3, image_size, image_size)
        self.pool = []
        for _ in range(max(1, pool)):
            x = torch.randn(shape, generator=g, device=self.device, dtype=torch.float32)
            x = x.to(dtype)
            y = torch.randint(0, num_classes, (batch_size,), generator=g, device=self.device)
            self.pool.append((x, y))
        self._i = 0

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        n = 0
        while self.steps_per_epoch <= 0 or n < self.steps_per_epoch:
            yield self.next()
            n += 1

    def next(self) -> Tuple[torch.Tensor, torch.Tensor]:
        b = self.pool[self._i % len(self.pool)]
        self._i += 1
        return b

    def __len__(self):
        return self.steps_per_epoch

    def state_dict(self):
        """Loader position (checkpoint / resume replays the same batch sequence)."""
        return {"index": self._i}

    def load_state_dict(self, st) -> None:
        self._i = int(st["index"])


class SyntheticTokens:
    def __init__(self, batch_size: int, seq_len: int = 128, vocab_size: int = 30522, num_labels: int = 2,
                 device: Optional[torch.device] = None, rank: int = 0, seed: int = 1234, pool: int = 4,
                 pad_fraction: float = 0.0, steps_per_epoch: int = 0, mlm_predictions: int = 0,
                 causal_lm: bool = False, docs_per_row: int = 0):
        """``mlm_predictions`` = P > 0 adds the masked-LM pretraining targets to every batch:
        ``masked_lm_positions [B, P]`` (unique per row, ascending, inside the row's unpadded length),
        ``masked_lm_labels [B, P]`` (a random number of trailing slots per row is padding: label
        -100, position 0; at least one slot per row is a target) and ``next_sentence_label [B]``.
        With 0 the batches are exactly those of a loader without the argument.

        ``causal_lm`` replaces ``labels`` by the next-token targets ``[B, S]``: ``labels[b, s]`` is
        ``input_ids[b, s + 1]``, -100 at the last position and wherever position ``s + 1`` is padding
        (the shift happens here, not in the model).  It draws nothing, so ids and masks are those of
        a loader without it.

        ``docs_per_row`` = k > 0 (with ``causal_lm``) packs k documents into every row: k - 1 distinct
        random cut points, so every document has at least one token.  The batch gains ``position_ids
        [B, S]`` (HF's packed-sequence convention: 0 at the first token of every document, previous + 1
        otherwise) and ``labels`` are -100 at the last token of every document as well.  The cuts come
        from a generator of their own, so ``input_ids`` are exactly those of a loader without the
        argument, and with 0 so is the whole batch."""
        self.batch_size, self.seq_len = batch_size, seq_len
        self.device = device or torch.device("cpu")
        self.steps_per_epoch = steps_per_epoch
        if docs_per_row < 0 or docs_per_row > seq_len:
            raise ValueError(f"docs_per_row={docs_per_row} must be in 0 .. seq_len ({seq_len})")
        if docs_per_row > 0 and not causal_lm:
            raise ValueError("docs_per_row packs causal-LM rows: it needs causal_lm=True")
        g = _gen(self.device, seed * 1000 + rank + 7)
        # (an offset no rank reaches: seed * 1000 + rank + 7 is the id stream of every rank)
        g_docs = _gen(self.device, seed * 1000 + rank + 7 + (1 << 40)) if docs_per_row > 0 else None
        self.pool = []
        for _ in range(max(1, pool)):
            ids = torch.randint(0, vocab_size, (batch_size, seq_len), generator=g, device=self.device)
            mask = None
            if pad_fraction > 0:
                lens = torch.randint(int(seq_len * (1 - pad_fraction)), seq_len + 1, (batch_size,),
                                     generator=g, device=self.device)
                mask = (torch.arange(seq_len, device=self.device)[None, :] < lens[:, None]).to(torch.int64)
            labels = torch.randint(0, num_labels, (batch_size,), generator=g, device=self.device)
            if causal_lm:
                labels = torch.full_like(ids, -100)
                labels[:, :-1] = ids[:, 1:] if mask is None else ids[:, 1:].masked_fill(mask[:, 1:] == 0, -100)
            batch = {"input_ids": ids, "attention_mask": mask, "labels": labels}
            if docs_per_row > 0:
                batch["position_ids"] = self._pack(docs_per_row, labels, g_docs)
            if mlm_predictions > 0:
                batch.update(self._mlm_targets(mlm_predictions, mask, vocab_size, pad_fraction, g))
            self.pool.append(batch)
        self._i = 0

    def _pack(self, k: int, labels: torch.Tensor, g) -> torch.Tensor:
        """Cut every row into k documents: returns ``position_ids`` and sets ``labels`` (in place) to -100
        at every document's last token."""
        B, S, dev = self.batch_size, self.seq_len, self.device
        # k - 1 distinct starts among 1 .. S-1: the k - 1 smallest of S - 1 random keys
        start = torch.zeros(B, S, dtype=torch.bool, device=dev)
        start[:, 0] = True
        if k > 1:
            cuts = torch.rand(B, S - 1, generator=g, device=dev).argsort(dim=1)[:, :k - 1] + 1
            start.scatter_(1, cuts, True)
        ar = torch.arange(S, device=dev)
        first = torch.where(start, ar[None, :], torch.zeros_like(ar)[None, :]).cummax(1).values
        labels[:, :-1].masked_fill_(start[:, 1:], -100)
        return ar[None, :] - first

    def _mlm_targets(self, P: int, mask, vocab_size: int, pad_fraction: float, g) -> dict:
        B, S, dev = self.batch_size, self.seq_len, self.device
        shortest = int(S * (1 - pad_fraction)) if mask is not None else S
        if P > shortest:
            raise ValueError(f"mlm_predictions={P} exceeds the shortest unpadded length {shortest}")
        # P distinct positions per row: the P smallest of S random keys, padded positions keyed last
        key = torch.rand(B, S, generator=g, device=dev)
        if mask is not None:
            key = key + (1 - mask).to(key.dtype) * 2.0
        pos = key.argsort(dim=1)[:, :P].sort(dim=1).values
        lab = torch.randint(0, vocab_size, (B, P), generator=g, device=dev)
        n_pad = torch.randint(0, P, (B,), generator=g, device=dev)          # 0 .. P-1: one target at least
        padded = torch.arange(P, device=dev)[None, :] >= (P - n_pad)[:, None]
        lab = lab.masked_fill(padded, -100)
        pos = pos.masked_fill(padded, 0)
        nsp = torch.randint(0, 2, (B,), generator=g, device=dev)
        return {"masked_lm_positions": pos, "masked_lm_labels": lab, "next_sentence_label": nsp}

    def __iter__(self):
        n = 0
        while self.steps_per_epoch <= 0 or n < self.steps_per_epoch:
            yield self.next()
            n += 1

    def next(self):
        b = self.pool[self._i % len(self.pool)]
        self._i += 1
        return b

    def __len__(self):
        return self.steps_per_epoch

    def state_dict(self):
        """Loader position (checkpoint / resume replays the same batch sequence)."""
        return {"index": self._i}

    def load_state_dict(self, st) -> None:
        self._i = int(st["index"])


def shard_indices(n: int, rank: int, world: int, shuffle: bool = False, seed: int = 0, drop_last: bool = True):
    """Rank-sharded index list (what a DistributedSampler yields) for real datasets."""
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(seed)) if shuffle else torch.arange(n)
    per = n // world if drop_last else -(-n // world)
    if not drop_last:
        idx = torch.cat([idx, idx[: per * world - n]])
    return idx[rank * per:(rank + 1) * per].tolist()
