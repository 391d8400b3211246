#!/usr/bin/env python3
"""Extending a grouped-query KV cache by a chunk of tokens, on one GPU: prefix reuse, the grouped-query
chunk-attention kernel, chunked prefill.  SmolLM-135M (9 heads over 3 KV heads), bf16, random weights; the
best of ``--reps`` runs after one warm-up run of each arm, the arms alternating in one process.

    python benchmarks/llama_extend_bench.py [--reps 3] [--skip-ttft] [--skip-kernel] [--skip-chunked]
                                            [--head-dim 128 | --fp8-kv | --split-sweep]

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

``--head-dim 128`` runs the head-dimension-128 study instead (csrc/kernels/attn_extend_d128.hip):
(d) ``ops.attention_extend_gqa`` at D = 128 for (H, Hkv) in {(32, 8), (32, 32)}, B in {1, 16}, T in {16, 64, 128,
    512} over n in {896, 8191} cached keys, timed as in (b) against ``ops.attention_extend_gqa_reference`` on the
    same tensors (what every D = 128 extend ran before) and the masked SDPA of (b).  Each line carries the bytes
    the kernel must read (n cached K and V rows of Hkv heads, the chunk, its table rows) and the MFMA FLOPs,
    both from the shapes; ``floor_bound`` marks a call time within 1.5x of the ~20 us enqueue floor, which bounds
    the kernel from above and does not measure it.  A fourth arm runs the same call with ``key_splits=1`` (the
    one launch, all there was before the key split): ``one_launch_us``, next to the ``key_splits`` the plan chose.
    ``--split-sweep`` runs only this comparison, without the reference and SDPA arms: the default, ``key_splits=1``
    and, at T <= 128, forced ``key_splits`` in {2, 4, 8, 16, 32}, alternating; each line carries the spread of
    the ``key_splits=1`` arm between its repeats, which is the margin the plan's constants were chosen against.
(e) (a) for ``llama3_8b(num_hidden_layers=4)``.

``--fp8-kv`` runs the FP8-cache study instead (csrc/kernels/attn_extend_d128_fp8.hip):
(f) the shapes of (d); three arms alternating in one process, timed as in (b): ``ops.attention_extend_gqa_fp8`` on
    an FP8 cache (e4m3 bytes and fp32 row scales), ``ops.attention_extend_gqa`` on a bf16 cache of the same shape,
    and ``attention_extend_gqa_fp8_reference`` (the dequantise / bf16 kernel / requantise composition every FP8
    extend ran before) on the FP8 cache; each arm rotates through its own >= 512 MB of cache copies.  Each line
    carries the two ratios, the bytes the fp8 kernel must read and the peak memory each fp8 arm allocates above
    its inputs in one call.
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


def _model(dev, name="smollm_135m", **kw):
    import torch
    from databricks_distributed_deep_learning_amd import models
    from databricks_distributed_deep_learning_amd.models import cast_params
    torch.manual_seed(0)
    model = getattr(models, name)(**kw).to(dev).eval()
    cast_params(model, torch.bfloat16)
    return model


def bench_ttft(model, dev, reps, name="smollm_135m"):
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
        print(json.dumps({"ttft": name, "B": B, "prefix": P, "new": T,
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


ENQUEUE_FLOOR_US = 20.0


def bench_kernel_d128(dev, reps):
    import torch
    import torch.nn.functional as F
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.ops import _native_attn_cache as N
    from databricks_distributed_deep_learning_amd.ops.attention import attention_extend_gqa_reference as ref_fn
    D, TS = 128, (16, 64, 128, 512)
    table = ops.rope_table(8192 + 512, 500000.0, D, dev)
    for H, Hkv in ((32, 8), (32, 32)):
        G = H // Hkv
        for B in (1, 16):
            for n in (896, 8191):
                C = n + max(TS)
                per_layer = 2 * B * Hkv * C * D * 2
                L = min(64, -(-ROTATE_BYTES // per_layer))
                data = torch.randn(L, 2, B, Hkv, C, D, device=dev).bfloat16()
                wide = data.repeat_interleave(G, 3) if G > 1 else data      # the cache expanded to H heads
                lens = torch.full((B,), n, dtype=torch.int32, device=dev)
                for T in TS:
                    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, device=dev).bfloat16()
                    q = ops.rope_qkv(qkv, table[n:n + T].contiguous(), H, Hkv).view(B, T, 3, H, D)[:, :, 0].transpose(1, 2)
                    j, i = torch.arange(n + T, device=dev), torch.arange(T, device=dev)
                    mask = j[None, :] <= n + i[:, None]

                    def ours(k):
                        ops.attention_extend_gqa(qkv, table, data[k % L, 0], data[k % L, 1], lens, H, Hkv, n)

                    def one(k):
                        ops.attention_extend_gqa(qkv, table, data[k % L, 0], data[k % L, 1], lens, H, Hkv, n,
                                                 key_splits=1)

                    def reference(k):
                        ref_fn(qkv, table, data[k % L, 0], data[k % L, 1], lens, H, Hkv, n)

                    def sdpa(k):
                        F.scaled_dot_product_attention(q, wide[k % L, 0, :, :, :n + T], wide[k % L, 1, :, :, :n + T],
                                                       attn_mask=mask)

                    arms = (("ours", ours), ("one", one), ("reference", reference), ("sdpa", sdpa))
                    iters = {}
                    for name, fn in arms:       # warm-up; then as many calls as fit ~50 ms, 3 .. 200
                        fn(0)
                        iters[name] = int(min(200, max(3, 5e4 / _events(fn, 3))))
                    t = {name: [] for name, _ in arms}
                    for _ in range(reps):
                        for name, fn in arms:
                            t[name].append(_events(fn, iters[name]))
                    t = {name: min(v) for name, v in t.items()}
                    flops = 4.0 * B * H * D * T * (n + (T + 1) / 2)
                    read = 2 * B * Hkv * n * D * 2 + B * T * (H + 2 * Hkv) * D * 2 + T * D * 4
                    print(json.dumps({"kernel": "attention_extend_gqa_d128", "B": B, "H": H, "Hkv": Hkv, "n": n, "T": T,
                                      "copies": L, "us": round(t["ours"], 2),
                                      "key_splits": N.plan_extend(B, T, H, Hkv, n), "one_launch_us": round(t["one"], 2),
                                      "reference_us": round(t["reference"], 2),
                                      "sdpa_masked_us": round(t["sdpa"], 2), "min_read_MB": round(read / 1e6, 2),
                                      "mfma_GFLOP": round(flops / 1e9, 3), "TFLOPs": round(flops / t["ours"] / 1e6, 2),
                                      "GBps": round(read / t["ours"] / 1e3, 1),
                                      "floor_bound": bool(t["ours"] < 1.5 * ENQUEUE_FLOOR_US),
                                      "faster_than_reference": bool(t["ours"] < t["reference"]),
                                      "faster_than_sdpa": bool(t["ours"] < t["sdpa"])}), flush=True)
                del data, wide


def bench_split_sweep(dev, reps):
    import torch
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.ops import _native_attn_cache as N
    D, TS = 128, (16, 64, 128, 512)
    table = ops.rope_table(8192 + 512, 500000.0, D, dev)
    for H, Hkv in ((32, 8), (32, 32)):
        for B in (1, 16):
            for n in (896, 8191):
                C = n + max(TS)
                L = min(64, -(-ROTATE_BYTES // (2 * B * Hkv * C * D * 2)))
                data = torch.randn(L, 2, B, Hkv, C, D, device=dev).bfloat16()
                lens = torch.full((B,), n, dtype=torch.int32, device=dev)
                for T in TS:
                    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, device=dev).bfloat16()

                    def arm(ks):
                        return lambda k: ops.attention_extend_gqa(qkv, table, data[k % L, 0], data[k % L, 1], lens, H,
                                                                  Hkv, n, key_splits=ks)

                    arms = [("default", arm(None)), ("1", arm(1))]
                    arms += [(str(ks), arm(ks)) for ks in (2, 4, 8, 16, 32)] if T <= 128 else []
                    iters = {}
                    for name, fn in arms:
                        fn(0)
                        iters[name] = int(min(200, max(3, 5e4 / _events(fn, 3))))
                    t = {name: [] for name, _ in arms}
                    for r in range(reps):       # odd rounds backwards: no arm always follows the same neighbour
                        for name, fn in (arms[::-1] if r % 2 else arms):
                            t[name].append(_events(fn, iters[name]))
                    best = {name: round(min(v), 2) for name, v in t.items()}
                    spread = max(t["1"]) - min(t["1"])
                    forced = {k: v for k, v in best.items() if k != "default"}
                    print(json.dumps({"split_sweep": "attention_extend_gqa_d128", "B": B, "H": H, "Hkv": Hkv, "n": n,
                                      "T": T, "copies": L, "plan": N.plan_extend(B, T, H, Hkv, n), "us": best,
                                      "one_launch_spread_us": round(spread, 2),
                                      "default_over_one_launch": round(best["default"] / best["1"], 3),
                                      "default_minus_best_forced_us": round(best["default"] - min(forced.values()), 2),
                                      "no_slower_than_one_launch": bool(best["default"] <= best["1"] + spread),
                                      "floor_bound": bool(best["default"] < 1.5 * ENQUEUE_FLOOR_US)}), flush=True)
                del data


def bench_kernel_fp8kv(dev, reps):
    import torch
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.ops.attention import attention_extend_gqa_fp8_reference as ref_fn
    D, TS = 128, (16, 64, 128, 512)
    table = ops.rope_table(8192 + 512, 500000.0, D, dev)
    for H, Hkv in ((32, 8), (32, 32)):
        for B in (1, 16):
            for n in (896, 8191):
                C = n + max(TS)
                per_layer = 2 * B * Hkv * C * D
                L8, L16 = min(64, -(-ROTATE_BYTES // per_layer)), min(64, -(-ROTATE_BYTES // (2 * per_layer)))
                # any finite e4m3 code (sign | 0 .. 0x77) and scales around 1 / 448: rows of amax about 1
                c8 = (torch.randint(0, 0x78, (L8, 2, B, Hkv, C, D), device=dev, dtype=torch.uint8)
                      | (torch.randint(0, 2, (L8, 2, B, Hkv, C, D), device=dev, dtype=torch.uint8) << 7))
                sc = (torch.rand(L8, 2, B, Hkv, C, device=dev) + 0.5) / 448
                c16 = torch.randn(L16, 2, B, Hkv, C, D, device=dev).bfloat16()
                lens = torch.full((B,), n, dtype=torch.int32, device=dev)
                for T in TS:
                    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, device=dev).bfloat16()

                    def fp8(k):
                        j = k % L8
                        ops.attention_extend_gqa_fp8(qkv, table, c8[j, 0], c8[j, 1], sc[j, 0], sc[j, 1], lens, H, Hkv, n)

                    def bf16(k):
                        ops.attention_extend_gqa(qkv, table, c16[k % L16, 0], c16[k % L16, 1], lens, H, Hkv, n)

                    def reference(k):
                        j = k % L8
                        ref_fn(qkv, table, c8[j, 0], c8[j, 1], sc[j, 0], sc[j, 1], lens, H, Hkv, n)

                    arms = (("fp8", fp8), ("bf16", bf16), ("reference", reference))
                    iters, peak = {}, {}
                    for name, fn in arms:       # warm-up (and the call's own allocations); then ~50 ms of calls
                        torch.cuda.synchronize()
                        base = torch.cuda.memory_allocated()
                        torch.cuda.reset_peak_memory_stats()
                        fn(0)
                        torch.cuda.synchronize()
                        peak[name] = torch.cuda.max_memory_allocated() - base
                        iters[name] = int(min(200, max(3, 5e4 / _events(fn, 3))))
                    t = {name: [] for name, _ in arms}
                    for _ in range(reps):
                        for name, fn in arms:
                            t[name].append(_events(fn, iters[name]))
                    t = {name: min(v) for name, v in t.items()}
                    read = 2 * B * Hkv * n * (D + 4) + B * T * (H + 2 * Hkv) * D * 2 + T * D * 4
                    print(json.dumps({"kernel": "attention_extend_gqa_d128_fp8", "B": B, "H": H, "Hkv": Hkv, "n": n, "T": T,
                                      "copies": [L8, L16], "fp8_us": round(t["fp8"], 2), "bf16_us": round(t["bf16"], 2),
                                      "fp8_reference_us": round(t["reference"], 2),
                                      "fp8_over_bf16": round(t["fp8"] / t["bf16"], 3),
                                      "reference_over_fp8": round(t["reference"] / t["fp8"], 2),
                                      "min_read_MB": round(read / 1e6, 2), "GBps": round(read / t["fp8"] / 1e3, 1),
                                      "call_peak_MB": round(peak["fp8"] / 2 ** 20, 2),
                                      "reference_call_peak_MB": round(peak["reference"] / 2 ** 20, 2),
                                      "floor_bound": bool(t["fp8"] < 1.5 * ENQUEUE_FLOOR_US),
                                      "faster_than_reference": bool(t["fp8"] < t["reference"]),
                                      "faster_than_bf16": bool(t["fp8"] < t["bf16"])}), flush=True)
                del c8, sc, c16


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
    ap.add_argument("--head-dim", type=int, default=64, choices=(64, 128))
    ap.add_argument("--fp8-kv", action="store_true")
    ap.add_argument("--split-sweep", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("llama_extend_bench needs a GPU: times are not measured without one")
    dev = torch.device("cuda", 0)
    if args.fp8_kv:
        with torch.no_grad():
            bench_kernel_fp8kv(dev, args.reps)
        return 0
    if args.split_sweep:
        with torch.no_grad():
            bench_split_sweep(dev, args.reps)
        return 0
    if args.head_dim == 128:
        with torch.no_grad():
            if not args.skip_kernel:
                bench_kernel_d128(dev, args.reps)
            if not args.skip_ttft:
                bench_ttft(_model(dev, "llama3_8b", num_hidden_layers=4), dev, args.reps, "llama3_8b(num_hidden_layers=4)")
        return 0
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
