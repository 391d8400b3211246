#!/usr/bin/env python3
"""Llama-family generation on one GPU: the grouped-query KV-cache decode against decoding by full re-forward,
and the decode attention against what the library could compose before it.

    python benchmarks/llama_generate_bench.py [--model smollm_135m] [--prompt 128] [--new 128]
                                              [--batches 1,8,16] [--reps 3] [--skip-e2e] [--skip-recompute]
                                              [--skip-kernels]

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
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("llama_generate_bench needs a GPU: times and rates are not measured without one")
    dev = torch.device("cuda", 0)
    if not args.skip_e2e:
        bench_e2e(dev, args)
    if not args.skip_kernels:
        bench_attention(dev)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
