#!/usr/bin/env python3
"""Llama-family generation on one GPU: the grouped-query KV-cache decode against decoding by full re-forward,
and the decode attention against what the library could compose before it.

    python benchmarks/llama_generate_bench.py [--model smollm_135m] [--prompt 128] [--new 128]
                                              [--batches 1,8,16] [--reps 3] [--skip-e2e] [--skip-recompute]
                                              [--skip-kernels] [--skip-d128] [--fp8] [--fp8-kv]

End to end (bf16, random weights, greedy, no eos): ``generate`` (prefill + cached decode steps), the same with
``use_graph=True`` (the decode step captured once and replayed; the capture is timed once, apart) and the
recompute arm (a full ``forward`` over the whole prefix per token, argmax of its last row), timed by a host
clock around work that ends in a device synchronise; the best of ``--reps`` runs after one warm-up run of each
arm, the arms alternating in one process.

Per call at B = 16 and 1023 cached keys, for (H, Hkv) = (9, 3) and (32, 32), timed by device events around
ITERS back-to-back calls (launch overhead included), every call on another copy of its cache (copies
totalling >= 512 MB, more than the 256 MB last-level cache, so the rows come from HBM):
  * ``ops.attention_decode_gqa`` on the ``[B, Hkv, C, 64]`` cache;
  * the composition that needs no new kernel: ``ops.rope_qkv`` on the one token (with that row's table
    rows gathered beforehand) plus ``ops.attention_decode`` over a cache expanded to H heads;
  * ``F.scaled_dot_product_attention`` with a boolean key mask on the H-head cache (it neither rotates nor
    appends).
Bytes are what each algorithm must read: 2 (n + 1) 128 B per (batch, KV head) for the GQA kernel, per (batch,
query head) for the other two.

Head dim 128 (``--skip-d128`` leaves it out), same method: (H, Hkv) = (32, 8) and (32, 32), B = 1 and 16, 1023
and 8191 cached keys; ``ops.attention_decode_gqa`` against ``attention_decode_gqa_reference`` on the same tensors
(what these shapes ran before the D = 128 kernel) and masked SDPA over the H-head cache; 2 (n + 1) 256 B per
(batch, KV head).  Then one end-to-end line: ``llama3_8b(num_hidden_layers=4)`` at B = 16, ``generate`` eager
and with ``use_graph=True``.

``--fp8`` runs only the FP8 decode-weight section: ``ops.linear_small_m_fp8`` against ``ops.linear_small_m`` per
call at M = 1 and 16 on Llama-3-8B's four block shapes (device events, the two arms alternating, best of 3, every
call on another copy of its weight, copies totalling >= 512 MB per arm; bytes are the weight's: N K (+ 4 N of
scales) against 2 N K), then ``llama3_8b(num_hidden_layers=4)`` at B = 1 and 16, eager and graph-replayed, with
and without ``quantize_decode_weights()``.

``--fp8-kv`` runs only the FP8 KV-cache section.  Per call at head dim 128, (H, Hkv) = (32, 8) and (32, 32), B = 1
and 16, 1023 and 8191 cached keys: ``ops.attention_decode_gqa_fp8`` against ``ops.attention_decode_gqa`` on a bf16
cache of the same shape against ``attention_decode_gqa_fp8_reference`` (device events, the arms alternating in one
process, best of 3, every call on another copy of its cache, copies totalling >= 512 MB per arm).  Bytes: 2 (n + 1)
(128 + 4) per (batch, KV head) against 2 (n + 1) 256.  Only the two B = 16, 8191-key shapes are far above the
~20 us launch floor; the other six sit at or near it and bound the kernel from above only (``near_floor``).  Then
``llama3_8b(num_hidden_layers=4)`` at B = 1 and 16, eager and graph-replayed, bf16 against FP8 cache, with and
without ``quantize_decode_weights()``.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_TBS = 6.3
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


def _best(fn, iters, reps=3):
    fn(0)
    _events(fn, max(4, iters // 4))
    return min(_events(fn, iters) for _ in range(reps))


def bench_attention(dev):
    import torch
    import torch.nn.functional as F
    from databricks_distributed_deep_learning_amd import ops
    B, D, C, n = 16, 64, 1024, 1023
    table = ops.rope_table(C, 10000.0, D, dev)
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
    for H, Hkv in ((9, 3), (32, 32)):
        G = H // Hkv
        L = min(256, -(-ROTATE_BYTES // (2 * B * Hkv * C * D * 2)))
        Lx = min(256, -(-ROTATE_BYTES // (2 * B * H * C * D * 2)))
        small = torch.randn(L, 2, B, Hkv, C, D, device=dev).bfloat16()
        big = torch.randn(Lx, 2, B, H, C, D, device=dev).bfloat16()
        proj = torch.randn(B, (H + 2 * Hkv) * D, device=dev).bfloat16()
        tab_n = table[n:n + 1].contiguous()         # every row sits at position n here: one table row serves
        q = torch.randn(B, H, 1, D, device=dev).bfloat16()
        keep = (torch.arange(C, device=dev)[None, :] <= lens[:, None]).view(B, 1, 1, C)

        def ours(i):
            ops.attention_decode_gqa(proj, table, small[i % L, 0], small[i % L, 1], lens, H, Hkv, n + 1)

        def composed(i):
            packed = ops.rope_qkv(proj.view(B, 1, -1), tab_n, H, Hkv)
            ops.attention_decode(packed.view(B, -1), big[i % Lx, 0], big[i % Lx, 1], lens, H, n + 1)

        def sdpa(i):
            F.scaled_dot_product_attention(q, big[i % Lx, 0], big[i % Lx, 1], attn_mask=keep)

        with torch.no_grad():
            t_o, t_c, t_s = _best(ours, 400), _best(composed, 400), _best(sdpa, 400)
        nb, nbx = 2 * (n + 1) * D * 2 * B * Hkv, 2 * (n + 1) * D * 2 * B * H
        print(json.dumps({"kernel": "attention_decode_gqa", "B": B, "H": H, "Hkv": Hkv, "G": G, "n": n,
                          "copies": L, "us": round(t_o, 2), "GBps": round(nb / t_o / 1e3, 1),
                          "share_of_stream": round(nb / t_o / 1e6 / STREAM_TBS, 4),
                          "rope_plus_mha_decode_us": round(t_c, 2), "rope_plus_mha_decode_GBps": round(nbx / t_c / 1e3, 1),
                          "masked_sdpa_us": round(t_s, 2), "masked_sdpa_GBps": round(nbx / t_s / 1e3, 1),
                          "no_slower_than_composition": bool(t_o <= t_c)}), flush=True)
        del small, big


def d128_bytes(B, Hkv, n):
    """What the D = 128 decode must read: 2 (n + 1) 256 B per (batch, KV head)."""
    return 2 * (n + 1) * 256 * B * Hkv


def bench_attention_d128(dev):
    """Head dim 128 per call, same method as above: the kernel, ``attention_decode_gqa_reference`` on the same
    tensors (what these shapes ran before the kernel) and masked SDPA over a cache expanded to H heads."""
    import torch
    import torch.nn.functional as F
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.ops.attention import attention_decode_gqa_reference
    D = 128
    for n in (1023, 8191):
        C = n + 1
        table = ops.rope_table(C, 5e5, D, dev)
        for H, Hkv in ((32, 8), (32, 32)):
            for B in (1, 16):
                lens = torch.full((B,), n, dtype=torch.int32, device=dev)
                L = min(256, -(-ROTATE_BYTES // (2 * B * Hkv * C * D * 2)))
                Lx = min(256, -(-ROTATE_BYTES // (2 * B * H * C * D * 2)))
                small = torch.randn(L, 2, B, Hkv, C, D, device=dev).bfloat16()
                big = small if H == Hkv else torch.randn(Lx, 2, B, H, C, D, device=dev).bfloat16()
                proj = torch.randn(B, (H + 2 * Hkv) * D, device=dev).bfloat16()
                q = torch.randn(B, H, 1, D, device=dev).bfloat16()
                keep = (torch.arange(C, device=dev)[None, :] <= lens[:, None]).view(B, 1, 1, C)

                def ours(i):
                    ops.attention_decode_gqa(proj, table, small[i % L, 0], small[i % L, 1], lens, H, Hkv, n + 1)

                def reference(i):
                    attention_decode_gqa_reference(proj, table, small[i % L, 0], small[i % L, 1], lens, H, Hkv, n + 1)

                def sdpa(i):
                    F.scaled_dot_product_attention(q, big[i % Lx, 0], big[i % Lx, 1], attn_mask=keep)

                slow = 20 if n > 4096 else 100
                with torch.no_grad():
                    t_o, t_r, t_s = _best(ours, 400), _best(reference, slow), _best(sdpa, slow)
                nb, nbx = d128_bytes(B, Hkv, n), d128_bytes(B, H, n)
                print(json.dumps({"kernel": "attention_decode_gqa_d128", "B": B, "H": H, "Hkv": Hkv, "G": H // Hkv,
                                  "n": n, "copies": L, "us": round(t_o, 2), "GBps": round(nb / t_o / 1e3, 1),
                                  "share_of_stream": round(nb / t_o / 1e6 / STREAM_TBS, 4),
                                  "reference_us": round(t_r, 2), "reference_GBps": round(nb / t_r / 1e3, 1),
                                  "masked_sdpa_us": round(t_s, 2), "masked_sdpa_GBps": round(nbx / t_s / 1e3, 1),
                                  "faster_than_reference": bool(t_o < t_r)}), flush=True)
                del small, big


def bench_e2e_d128(dev, args):
    """``llama3_8b(num_hidden_layers=4)``: ``generate`` eager and graph-replayed, tokens/s."""
    import torch
    from databricks_distributed_deep_learning_amd.models import cast_params, llama3_8b
    torch.manual_seed(0)
    with torch.device(dev):
        model = llama3_8b(num_hidden_layers=4).eval()
    model = model.to(dev)
    cast_params(model, torch.bfloat16)
    B = 16
    ids = torch.randint(0, model.config.vocab_size, (B, args.prompt), device=dev)
    arms = {"cached": lambda: model.generate(ids, max_new_tokens=args.new),
            "graph": lambda: model.generate(ids, max_new_tokens=args.new, use_graph=True)}
    outs, times = {}, {name: [] for name in arms}
    for rep in range(args.reps + 1):        # (the first round warms up and captures)
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            outs[name] = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t)
    c, g = min(times["cached"]), min(times["graph"])
    print(json.dumps({"e2e": "llama3_8b(num_hidden_layers=4)", "B": B, "prompt": args.prompt, "new": args.new,
                      "cached_tokens_per_s": round(B * args.new / c, 1), "graph_tokens_per_s": round(B * args.new / g, 1),
                      "graph_speedup_over_cached": round(c / g, 2), "graph_captures": model.decode_session.captures,
                      "graph_token_agreement_with_cached": round((outs["cached"] == outs["graph"]).float().mean().item(), 4)}),
          flush=True)


LLAMA3_8B_LINEARS = ((6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336))     # qkv, o_proj, gate_up, down_proj


def bench_fp8_linears(dev):
    import torch
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.ops import _native_linear_decode as NL, _native_linear_decode_fp8 as NLF
    for N, K in LLAMA3_8B_LINEARS:
        L16, L8 = -(-ROTATE_BYTES // (2 * N * K)), -(-ROTATE_BYTES // (N * K))
        w16 = (torch.randn(L16, N, K, device=dev) * K ** -0.5).bfloat16()
        wq = torch.empty(L8, N, K, dtype=torch.float8_e4m3fn, device=dev)
        sc = torch.empty(L8, N, dtype=torch.float32, device=dev)
        for i in range(L8):
            wq[i], sc[i] = ops.quantize_fp8_rows(w16[i % L16])
        for M in (1, 16):
            x = torch.randn(M, K, device=dev).bfloat16()

            def bf16(i):
                ops.linear_small_m(x, w16[i % L16])

            def fp8(i):
                ops.linear_small_m_fp8(x, wq[i % L8], sc[i % L8])

            with torch.no_grad():
                _best(bf16, 200, 1), _best(fp8, 200, 1)         # warm-up of both arms
                t16 = t8 = float("inf")
                for _ in range(3):
                    t16, t8 = min(t16, _events(bf16, 400)), min(t8, _events(fp8, 400))
            nb16, nb8 = 2 * N * K, N * K + 4 * N
            print(json.dumps({"kernel": "linear_small_m_fp8", "M": M, "N": N, "K": K, "copies": [L16, L8],
                              "plan_fp8": NLF.plan(N, K), "plan_bf16": NL.plan(N, K),
                              "fp8_us": round(t8, 2), "fp8_GBps": round(nb8 / t8 / 1e3, 1),
                              "fp8_share_of_stream": round(nb8 / t8 / 1e6 / STREAM_TBS, 4),
                              "bf16_us": round(t16, 2), "bf16_GBps": round(nb16 / t16 / 1e3, 1),
                              "bf16_share_of_stream": round(nb16 / t16 / 1e6 / STREAM_TBS, 4),
                              "fp8_over_bf16": round(t8 / t16, 3), "fp8_no_slower": bool(t8 <= t16)}), flush=True)
        del w16, wq, sc


def bench_fp8_e2e(dev, args):
    """``llama3_8b(num_hidden_layers=4)``, B = 1 and 16: ``generate`` eager and graph-replayed on the bf16 weights
    and on ``quantize_decode_weights()``; each round runs all four arms (the session is captured again, untimed,
    after every switch of the weights)."""
    import torch
    from databricks_distributed_deep_learning_amd.models import cast_params, llama3_8b
    torch.manual_seed(0)
    with torch.device(dev):
        model = llama3_8b(num_hidden_layers=4).eval()
    cast_params(model, torch.bfloat16)
    for B in (1, 16):
        ids = torch.randint(0, model.config.vocab_size, (B, args.prompt), device=dev)

        def timed(**kw):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = model.generate(ids, max_new_tokens=args.new, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t, out
        times, outs = {}, {}
        for rnd in range(args.reps + 1):        # (the first round warms up)
            for fmt in ("bf16", "fp8"):
                model.quantize_decode_weights() if fmt == "fp8" else model.clear_decode_weights()
                timed(use_graph=True)           # captures the session for these weights
                for arm, kw in (("cached", {}), ("graph", {"use_graph": True})):
                    t, outs[fmt, arm] = timed(**kw)
                    if rnd:
                        times.setdefault((fmt, arm), []).append(t)
        tps = {k: B * args.new / min(v) for k, v in times.items()}
        print(json.dumps({"e2e": "llama3_8b(num_hidden_layers=4)", "B": B, "prompt": args.prompt, "new": args.new,
                          **{f"{fmt}_{arm}_tokens_per_s": round(tps[fmt, arm], 1) for fmt, arm in tps},
                          "fp8_speedup_cached": round(tps["fp8", "cached"] / tps["bf16", "cached"], 3),
                          "fp8_speedup_graph": round(tps["fp8", "graph"] / tps["bf16", "graph"], 3),
                          "fp8_graph_token_agreement_with_cached":
                              round((outs["fp8", "cached"] == outs["fp8", "graph"]).float().mean().item(), 4),
                          "fp8_token_agreement_with_bf16":
                              round((outs["fp8", "cached"] == outs["bf16", "cached"]).float().mean().item(), 4)}),
              flush=True)
    model.clear_decode_weights()


def bench_fp8_kv_attention(dev):
    import torch
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.ops.attention import attention_decode_gqa_fp8_reference
    D = 128
    for n in (1023, 8191):
        C = n + 1
        table = ops.rope_table(C, 5e5, D, dev)
        for H, Hkv in ((32, 8), (32, 32)):
            for B in (1, 16):
                lens = torch.full((B,), n, dtype=torch.int32, device=dev)
                L16 = min(256, -(-ROTATE_BYTES // (2 * B * Hkv * C * D * 2)))
                L8 = min(512, -(-ROTATE_BYTES // (2 * B * Hkv * C * (D + 4))))
                c16 = torch.randn(L16, 2, B, Hkv, C, D, device=dev).bfloat16()
                c8 = torch.empty(L8, 2, B, Hkv, C, D, dtype=torch.float8_e4m3fn, device=dev)
                sc = torch.empty(L8, 2, B, Hkv, C, dtype=torch.float32, device=dev)
                for i in range(L8):
                    q, s = ops.quantize_fp8_rows(c16[i % L16].view(-1, D))
                    c8[i], sc[i] = q.view(2, B, Hkv, C, D), s.view(2, B, Hkv, C)
                proj = torch.randn(B, (H + 2 * Hkv) * D, device=dev).bfloat16()

                def bf16(i):
                    ops.attention_decode_gqa(proj, table, c16[i % L16, 0], c16[i % L16, 1], lens, H, Hkv, n + 1)

                def fp8(i):
                    j = i % L8
                    ops.attention_decode_gqa_fp8(proj, table, c8[j, 0], c8[j, 1], sc[j, 0], sc[j, 1], lens, H, Hkv, n + 1)

                def reference(i):
                    j = i % L8
                    attention_decode_gqa_fp8_reference(proj, table, c8[j, 0], c8[j, 1], sc[j, 0], sc[j, 1], lens, H, Hkv,
                                                       n + 1)

                with torch.no_grad():
                    _best(bf16, 200, 1), _best(fp8, 200, 1)         # warm-up of both arms
                    t16 = t8 = float("inf")
                    for _ in range(3):
                        t16, t8 = min(t16, _events(bf16, 400)), min(t8, _events(fp8, 400))
                    t_r = _best(reference, 10 if n > 4096 else 40, 1)
                nb16, nb8 = d128_bytes(B, Hkv, n), 2 * (n + 1) * (D + 4) * B * Hkv
                print(json.dumps({"kernel": "attention_decode_gqa_fp8", "B": B, "H": H, "Hkv": Hkv, "G": H // Hkv, "n": n,
                                  "copies": [L16, L8], "near_floor": not (B == 16 and n == 8191),
                                  "fp8_us": round(t8, 2), "fp8_GBps": round(nb8 / t8 / 1e3, 1),
                                  "fp8_share_of_stream": round(nb8 / t8 / 1e6 / STREAM_TBS, 4),
                                  "bf16_us": round(t16, 2), "bf16_GBps": round(nb16 / t16 / 1e3, 1),
                                  "bf16_share_of_stream": round(nb16 / t16 / 1e6 / STREAM_TBS, 4),
                                  "fp8_reference_us": round(t_r, 2), "fp8_over_bf16": round(t8 / t16, 3),
                                  "fp8_faster": bool(t8 < t16)}), flush=True)
                del c16, c8, sc


def bench_fp8_kv_e2e(dev, args):
    """``llama3_8b(num_hidden_layers=4)``, B = 1 and 16: ``generate`` eager and graph-replayed on a bf16 and on an
    FP8 cache, with the bf16 weights and with ``quantize_decode_weights()``; each round runs all eight arms (a
    switch of weights or cache rebuilds the session: one untimed graph call first)."""
    import torch
    from databricks_distributed_deep_learning_amd.models import cast_params, llama3_8b
    torch.manual_seed(0)
    with torch.device(dev):
        model = llama3_8b(num_hidden_layers=4).eval()
    cast_params(model, torch.bfloat16)
    for B in (1, 16):
        ids = torch.randint(0, model.config.vocab_size, (B, args.prompt), device=dev)

        def timed(**kw):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = model.generate(ids, max_new_tokens=args.new, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t, out
        times, outs = {}, {}
        for rnd in range(args.reps + 1):        # (the first round warms up)
            for w in ("w16", "w8"):
                model.quantize_decode_weights() if w == "w8" else model.clear_decode_weights()
                for kv in ("kv16", "kv8"):
                    kw = {"kv_cache_dtype": "fp8"} if kv == "kv8" else {}
                    timed(use_graph=True, **kw)         # captures the session for these weights and this cache
                    for arm, more in (("cached", {}), ("graph", {"use_graph": True})):
                        t, outs[w, kv, arm] = timed(**kw, **more)
                        if rnd:
                            times.setdefault((w, kv, arm), []).append(t)
        tps = {k: B * args.new / min(v) for k, v in times.items()}
        print(json.dumps({"e2e": "llama3_8b(num_hidden_layers=4)", "B": B, "prompt": args.prompt, "new": args.new,
                          **{"_".join(k) + "_tokens_per_s": round(v, 1) for k, v in tps.items()},
                          **{f"kv8_speedup_{w}_{arm}": round(tps[w, "kv8", arm] / tps[w, "kv16", arm], 3)
                             for w in ("w16", "w8") for arm in ("cached", "graph")},
                          "kv8_graph_token_agreement_with_cached":
                              round((outs["w16", "kv8", "cached"] == outs["w16", "kv8", "graph"]).float().mean().item(), 4),
                          "kv8_token_agreement_with_kv16":
                              round((outs["w16", "kv8", "cached"] == outs["w16", "kv16", "cached"]).float().mean().item(),
                                    4)}), flush=True)
    model.clear_decode_weights()


def bench_e2e(dev, args):
    import torch
    from databricks_distributed_deep_learning_amd import models
    from databricks_distributed_deep_learning_amd.models import cast_params
    from databricks_distributed_deep_learning_amd.models._decode_graph import round_capacity, session_for
    torch.manual_seed(0)
    model = getattr(models, args.model)().to(dev).eval()
    cast_params(model, torch.bfloat16)
    n_pos = model.config.max_position_embeddings
    for B in [int(b) for b in args.batches.split(",")]:
        ids = torch.randint(0, model.config.vocab_size, (B, args.prompt), device=dev)

        def cached():
            return model.generate(ids, max_new_tokens=args.new)

        def recompute():
            seq = ids
            with torch.no_grad():
                for _ in range(args.new):
                    seq = torch.cat([seq, model(seq)[:, -1].argmax(-1, keepdim=True)], 1)
            return seq

        def graphed():
            return model.generate(ids, max_new_tokens=args.new, use_graph=True)

        def timed(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t, out

        # the session (cache, state, warm-up and capture of the step) is built once per shape: timed apart
        t_capture, sess = timed(lambda: session_for(model, B, round_capacity(args.prompt + args.new, n_pos), True))
        _, a = timed(cached)
        _, g = timed(graphed)
        assert model.decode_session is sess and sess.captures == 1
        arms = [("cached", cached), ("graph", graphed)]
        agree = None
        if not args.skip_recompute:
            _, b = timed(recompute)
            agree = (a == b).float().mean().item()
            arms.append(("recompute", recompute))
        times = {name: [] for name, _ in arms}
        for _ in range(args.reps):
            for name, fn in arms:
                times[name].append(timed(fn)[0])
        c, gt = min(times["cached"]), min(times["graph"])
        n_tok = B * args.new
        rec = {"e2e": args.model, "B": B, "prompt": args.prompt, "new": args.new,
               "cached_tokens_per_s": round(n_tok / c, 1), "cached_ms_per_token": round(c / args.new * 1e3, 3),
               "graph_tokens_per_s": round(n_tok / gt, 1), "graph_ms_per_token": round(gt / args.new * 1e3, 3),
               "graph_speedup_over_cached": round(c / gt, 2), "graph_faster": bool(gt < c),
               "graph_capture_s": round(t_capture, 4), "graph_captures": sess.captures,
               "graph_token_agreement_with_cached": round((a == g).float().mean().item(), 4),
               "cached_s_all": [round(t, 4) for t in times["cached"]],
               "graph_s_all": [round(t, 4) for t in times["graph"]]}
        if not args.skip_recompute:
            r = min(times["recompute"])
            rec.update({"recompute_tokens_per_s": round(n_tok / r, 1),
                        "recompute_ms_per_token": round(r / args.new * 1e3, 3), "speedup": round(r / c, 2),
                        "graph_speedup_over_recompute": round(r / gt, 2),
                        "graph_fastest": bool(gt < c and gt < r),
                        "recompute_s_all": [round(t, 4) for t in times["recompute"]],
                        "token_agreement": round(agree, 4)})
        print(json.dumps(rec), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="smollm_135m")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-recompute", action="store_true", help="end to end: the cached and graph arms only")
    ap.add_argument("--skip-d128", action="store_true", help="no head-dim-128 section (per call and llama3_8b)")
    ap.add_argument("--fp8", action="store_true", help="only the FP8 decode-weight section (per call and llama3_8b)")
    ap.add_argument("--fp8-kv", action="store_true", help="only the FP8 KV-cache section (per call and llama3_8b)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("llama_generate_bench needs a GPU: times and rates are not measured without one")
    dev = torch.device("cuda", 0)
    if args.fp8:
        bench_fp8_linears(dev)
        bench_fp8_e2e(dev, args)
        return 0
    if args.fp8_kv:
        bench_fp8_kv_attention(dev)
        bench_fp8_kv_e2e(dev, args)
        return 0
    if not args.skip_e2e:
        bench_e2e(dev, args)
    if not args.skip_kernels:
        bench_attention(dev)
    if not args.skip_d128:
        bench_attention_d128(dev)
        bench_e2e_d128(dev, args)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
