#!/usr/bin/env python3
"""Extending a grouped-query KV cache by a chunk of tokens, on one GPU: prefix reuse, the grouped-query
chunk-attention kernel, chunked prefill.  SmolLM-135M (9 heads over 3 KV heads), bf16, random weights; the
best of ``--reps`` runs after one warm-up run of each arm, the arms alternating in one process.

    python benchmarks/llama_extend_bench.py [--reps 3] [--skip-ttft] [--skip-kernel] [--skip-chunked]

(a) Time to first token (host clock around work that ends in a device synchronise) for an 896-token prefix
    shared by every row plus 64 new tokens, B in {1, 8, 16}: a fresh cache that copies the batch-1 prefix
    cache and ``extend``s by the 64 tokens, against a full ``prefill`` of the 960 (all there was before).
(b) ``ops.attention_extend_gqa`` at T in {16, 64, 128} over n = 896 cached keys, B in {1, 16}, (H, Hkv) in
    {(9, 3), (32, 32)}, as call times (device events around back-to-back calls, launch overhead included;
    every call on another copy of the cache, copies totalling >= 512 MB), against
      - the composition that was possible before: ``ops.rope_qkv`` on the chunk (table rows n ..) plus
        ``ops.attention_extend`` over a cache already expanded to H heads (the expansion itself is NOT
        timed: it is a one-off cost of G times the memory, which favours this arm), and
      - ``F.scaled_dot_product_attention`` with an explicit ``[T, n + T]`` mask, handed rotated queries and
        the n + T expanded key rows in place (it neither rotates, gathers nor appends).
(c) ``prefill(chunk=128)`` against the whole ``prefill`` at S = 1024, B = 16: time and
    ``torch.cuda.max_memory_allocated`` above what was allocated before the call, on one preallocated cache.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROTATE_BYTES = 512 << 20


def _events(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us per call


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def _alternate(arms, reps):
    """{name: best seconds}: one warm-up run of each arm, then ``reps`` rounds, the arms alternating."""
    for _, fn in arms:
        fn()
    times = {name: [] for name, _ in arms}
    for _ in range(reps):
        for name, fn in arms:
            times[name].append(_timed(fn))
    return {name: min(v) for name, v in times.items()}, times


def _model(dev):
    import torch
    from databricks_distributed_deep_learning_amd import models
    from databricks_distributed_deep_learning_amd.models import cast_params
    torch.manual_seed(0)
    model = models.smollm_135m().to(dev).eval()
    cast_params(model, torch.bfloat16)
    return model


def bench_ttft(model, dev, reps):
    import torch
    from databricks_distributed_deep_learning_amd.models import LlamaKVCache
    P, T = 896, 64
    V = model.config.vocab_size
    head = torch.randint(0, V, (1, P), device=dev)
    prefix = LlamaKVCache.allocate(model, 1, P)
    model.prefill(head, torch.tensor([P], dtype=torch.int32, device=dev), prefix)
    for B in (1, 8, 16):
        tail = torch.randint(0, V, (B, T), device=dev)
        whole = torch.cat([head.expand(B, P), tail], 1)
        lens = torch.full((B,), P + T, dtype=torch.int32, device=dev)
        out = {}

        def reuse():
            cache = LlamaKVCache.allocate(model, B, 1024)
            cache.copy_prefix_(prefix)
            out["reuse"] = model.extend(tail, cache)

        def full():
            cache = LlamaKVCache.allocate(model, B, 1024)
            out["full"] = model.prefill(whole, lens, cache)

        best, times = _alternate([("reuse", reuse), ("full", full)], reps)
        agree = (out["reuse"].argmax(-1) == out["full"].argmax(-1)).float().mean().item()
        print(json.dumps({"ttft": "smollm_135m", "B": B, "prefix": P, "new": T,
                          "reuse_ms": round(best["reuse"] * 1e3, 3), "full_prefill_ms": round(best["full"] * 1e3, 3),
                          "speedup": round(best["full"] / best["reuse"], 2),
                          "reuse_faster": bool(best["reuse"] < best["full"]), "argmax_agreement": round(agree, 4),
                          "logit_max_abs_diff": round((out["reuse"].float() - out["full"].float()).abs().max().item(), 4),
                          "reuse_ms_all": [round(t * 1e3, 3) for t in times["reuse"]],
                          "full_ms_all": [round(t * 1e3, 3) for t in times["full"]]}), flush=True)


def bench_kernel(dev, reps):
    import torch
    import torch.nn.functional as F
    from databricks_distributed_deep_learning_amd import ops
    D, C, n = 64, 1024, 896
    table = ops.rope_table(2048, 10000.0, D, dev)
    for H, Hkv in ((9, 3), (32, 32)):
        G = H // Hkv
        for B in (1, 16):
            per_layer = 2 * B * Hkv * C * D * 2
            L = min(256, -(-ROTATE_BYTES // per_layer))
            data = torch.randn(L, 2, B, Hkv, C, D, device=dev).bfloat16()
            wide = data.repeat_interleave(G, 3) if G > 1 else data.clone()     # the cache expanded to H heads
            lens = torch.full((B,), n, dtype=torch.int32, device=dev)
            for T in (16, 64, 128):
                qkv = torch.randn(B, T, (H + 2 * Hkv) * D, device=dev).bfloat16()
                rows = table[n:n + T].contiguous()
                q = ops.rope_qkv(qkv, rows, H, Hkv).view(B, T, 3, H, D)[:, :, 0].transpose(1, 2)
                j, i = torch.arange(n + T, device=dev), torch.arange(T, device=dev)
                mask = j[None, :] <= n + i[:, None]

                def ours(k):
                    ops.attention_extend_gqa(qkv, table, data[k % L, 0], data[k % L, 1], lens, H, Hkv, n)

                def composed(k):
                    ops.attention_extend(ops.rope_qkv(qkv, rows, H, Hkv), wide[k % L, 0], wide[k % L, 1], lens, H, n)

                def sdpa(k):
                    F.scaled_dot_product_attention(q, wide[k % L, 0, :, :, :n + T], wide[k % L, 1, :, :, :n + T],
                                                   attn_mask=mask)

                iters = 200
                arms = (("ours", ours), ("composed", composed), ("sdpa", sdpa))
                for _, fn in arms:
                    fn(0)
                    _events(fn, 50)
                t = {name: [] for name, _ in arms}
                for _ in range(reps):
                    for name, fn in arms:
                        t[name].append(_events(fn, iters))
                t = {name: min(v) for name, v in t.items()}
                flops = 4.0 * B * H * D * T * (n + (T + 1) / 2)
                print(json.dumps({"kernel": "attention_extend_gqa", "B": B, "H": H, "Hkv": Hkv, "n": n, "T": T,
                                  "copies": L, "us": round(t["ours"], 2),
                                  "rope_plus_extend_expanded_us": round(t["composed"], 2),
                                  "sdpa_masked_us": round(t["sdpa"], 2), "TFLOPs": round(flops / t["ours"] / 1e6, 2),
                                  "no_slower_than_composition": bool(t["ours"] <= t["composed"]),
                                  "faster_than_sdpa": bool(t["ours"] < t["sdpa"])}), flush=True)
            del data, wide


def bench_chunked(model, dev, reps):
    import torch
    from databricks_distributed_deep_learning_amd.models import LlamaKVCache
    B, S, chunk = 16, 1024, 128
    ids = torch.randint(0, model.config.vocab_size, (B, S), device=dev)
    cnt = torch.full((B,), S, dtype=torch.int32, device=dev)
    cache = LlamaKVCache.allocate(model, B, S)
    out, peak = {}, {}

    def arm(name, pc):
        def fn():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out[name] = model.prefill(ids, cnt, cache, chunk=pc)
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - base
        return fn

    best, times = _alternate([("chunked", arm("chunked", chunk)), ("whole", arm("whole", None))], reps)
    agree = (out["chunked"].argmax(-1) == out["whole"].argmax(-1)).float().mean().item()
    print(json.dumps({"chunked_prefill": "smollm_135m", "B": B, "S": S, "chunk": chunk,
                      "chunked_ms": round(best["chunked"] * 1e3, 3), "whole_ms": round(best["whole"] * 1e3, 3),
                      "chunked_over_whole": round(best["chunked"] / best["whole"], 3),
                      "chunked_faster": bool(best["chunked"] < best["whole"]),
                      "chunked_peak_MB": round(peak["chunked"] / 2 ** 20, 1), "whole_peak_MB": round(peak["whole"] / 2 ** 20, 1),
                      "argmax_agreement": round(agree, 4),
                      "chunked_ms_all": [round(t * 1e3, 3) for t in times["chunked"]],
                      "whole_ms_all": [round(t * 1e3, 3) for t in times["whole"]]}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-ttft", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-chunked", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("llama_extend_bench needs a GPU: times are not measured without one")
    dev = torch.device("cuda", 0)
    model = None if args.skip_ttft and args.skip_chunked else _model(dev)
    with torch.no_grad():
        if not args.skip_ttft:
            bench_ttft(model, dev, args.reps)
        if not args.skip_kernel:
            bench_kernel(dev, args.reps)
        if not args.skip_chunked:
            bench_chunked(model, dev, args.reps)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
