#!/usr/bin/env python3
"""GPT-2 generation on one GPU: the KV-cache decode against decoding by full re-forward, and the two
decode kernels against what the library had before them.

    python benchmarks/gpt2_generate_bench.py [--model gpt2] [--prompt 128] [--new 128] [--batches 1,8,16]
                                             [--reps 3] [--skip-e2e] [--skip-recompute] [--skip-glue]
                                             [--skip-sampling] [--skip-kernels]

End to end (bf16, random weights, greedy, no eos): ``generate`` (prefill + cached decode steps), the same
with ``use_graph=True`` (the decode step captured once and replayed; the capture is timed once, apart) and
the recompute arm (a full ``forward`` over the whole prefix per token, argmax of its last row), timed by a
host clock around work that ends in a device synchronise; the best of ``--reps`` runs after one warm-up
run of each arm, the arms alternating in one process.

The step's glue (``ops.decode_embed``, ``ops.next_token``) at V = 50257 and B in {1, 16} against the ATen
sequences it replaces, as call times; ``next_token`` with top-p, min-p and a repetition penalty against the
torch composition of the same semantics (``bench_sampling``).

Per kernel, timed by device events around ITERS back-to-back calls (so launch overhead is included:
"call time"), every call on another copy of its large operand (copies totalling >= 512 MB, more than the
256 MB last-level cache, so the operand comes from HBM):
  * decode attention at n in {128, 512, 1023} cached keys against ``F.scaled_dot_product_attention`` on
    the same cache (which neither appends nor needs to: it is handed the n + 1 rows);
  * the small-M linear on GPT-2 small's five shapes at M in {1, 8, 16} against ``ops.linear``.
Bytes are what the algorithm must read: 2 (n + 1) 128 B per (batch, head) for attention, N K 2 B for a
linear; the streaming figure to hold them against is 6.3 TB/s (a float4 copy on this part; 8 TB/s spec).
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
    H, D, C = 12, 64, 1024
    for B in (1, 16):
        per_layer = 2 * B * H * C * D * 2
        L = min(256, -(-ROTATE_BYTES // per_layer))
        data = torch.randn(L, 2, B, H, C, D, device=dev).bfloat16()
        qkv = torch.randn(B, 3 * H * D, device=dev).bfloat16()
        for n in (128, 512, 1023):
            lens = torch.full((B,), n, dtype=torch.int32, device=dev)
            q = qkv.view(B, 3, H, 1, D)[:, 0]

            def ours(i):
                ops.attention_decode(qkv, data[i % L, 0], data[i % L, 1], lens, H, n + 1)

            def sdpa(i):
                F.scaled_dot_product_attention(q, data[i % L, 0, :, :, :n + 1], data[i % L, 1, :, :, :n + 1])

            t_o, t_s = _best(ours, 400), _best(sdpa, 400)
            nbytes = 2 * (n + 1) * D * 2 * B * H
            print(json.dumps({"kernel": "attention_decode", "B": B, "H": H, "n": n, "copies": L, "us": round(t_o, 2),
                              "sdpa_us": round(t_s, 2), "GBps": round(nbytes / t_o / 1e3, 1),
                              "sdpa_GBps": round(nbytes / t_s / 1e3, 1),
                              "share_of_stream": round(nbytes / t_o / 1e6 / STREAM_TBS, 4)}), flush=True)
        del data


def bench_linear(dev):
    import torch
    from databricks_distributed_deep_learning_amd import ops
    shapes = [("qkv", 2304, 768, None, False), ("attn_out", 768, 768, None, True), ("fc1", 3072, 768, "gelu", False),
              ("fc2", 768, 3072, None, True), ("head", 50257, 768, None, False)]
    for name, N, K, act, res in shapes:
        copies = min(512, -(-ROTATE_BYTES // (N * K * 2)))
        w = (torch.randn(copies, N, K, device=dev) * K ** -0.5).bfloat16()
        bias = None if name == "head" else torch.randn(N, device=dev).bfloat16()
        for M in (1, 8, 16):
            x = torch.randn(M, K, device=dev).bfloat16()
            r = torch.randn(M, N, device=dev).bfloat16() if res else None

            def ours(i):
                ops.linear_small_m(x, w[i % copies], bias, act, r)

            def base(i):
                ops.linear(x, w[i % copies], bias, act, residual=r)

            with torch.no_grad():
                t_o, t_b = _best(ours, 300), _best(base, 300)
            nbytes = N * K * 2
            print(json.dumps({"kernel": "linear_small_m", "layer": name, "M": M, "N": N, "K": K, "copies": copies,
                              "us": round(t_o, 2), "ops_linear_us": round(t_b, 2),
                              "GBps": round(nbytes / t_o / 1e3, 1), "ops_linear_GBps": round(nbytes / t_b / 1e3, 1),
                              "share_of_stream": round(nbytes / t_o / 1e6 / STREAM_TBS, 4),
                              "faster_than_ops_linear": bool(t_o < t_b)}), flush=True)
        del w


def bench_e2e(dev, args):
    import torch
    from databricks_distributed_deep_learning_amd import models
    from databricks_distributed_deep_learning_amd.models import cast_params
    from databricks_distributed_deep_learning_amd.models._decode_graph import round_capacity, session_for
    torch.manual_seed(0)
    model = getattr(models, args.model)(dropout=0.0).to(dev).eval()
    cast_params(model, torch.bfloat16)
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
        t_capture, sess = timed(lambda: session_for(model, B, round_capacity(args.prompt + args.new,
                                                                             model.config.n_positions), True))
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
                        "recompute_s_all": [round(t, 4) for t in times["recompute"]],
                        "token_agreement": round(agree, 4)})
        print(json.dumps(rec), flush=True)


def bench_glue(dev):
    """``decode_embed`` and ``next_token`` at GPT-2 small's sizes against the ATen sequences they replace
    (call times: device events around back-to-back calls, launch overhead included)."""
    import torch
    from databricks_distributed_deep_learning_amd import ops
    V, E, P = 50257, 768, 1024
    wte, wpe = torch.randn(V, E, device=dev).bfloat16(), torch.randn(P, E, device=dev).bfloat16()
    for B in (1, 16):
        tok = torch.randint(0, V, (B,), device=dev)
        lens = torch.randint(0, P - 1, (B,), device=dev).int()
        logits = (torch.randn(B, V, device=dev) * 2).bfloat16()
        u = torch.rand(1, B, device=dev)
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        step = torch.zeros(B, dtype=torch.int32, device=dev)
        tokens_out = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        out = torch.zeros(B, dtype=torch.int64, device=dev)
        lens2 = lens.clone()
        greedy = ops.next_token_params(eos_token_id=0, sample=False, device=dev)
        sampled = ops.next_token_params(1.0 / 0.8, 50, eos_token_id=0, device=dev)

        def embed(i):
            ops.decode_embed(tok, lens, wte, wpe)

        def embed_aten(i):
            ops.embedding(tok, wte) + ops.embedding(lens.long(), wpe)

        def pick(params):
            def f(i):
                ops.next_token(logits, u=u, params=params, step=step, done=done, out=out, tokens_out=tokens_out,
                               lens=lens2)
            return f

        def greedy_aten(i):
            t = logits.argmax(-1)
            t = torch.where(done, torch.full_like(t, 0), t)
            d = done | (t == 0)     # noqa: F841
            lens2.add_(1)

        def sampled_aten(i):
            z = logits.float() / 0.8
            kth = z.topk(50, -1).values[:, -1:]
            z = torch.where(z < kth, torch.full_like(z, float("-inf")), z)
            t = torch.multinomial(torch.softmax(z, -1), 1).squeeze(1)
            t = torch.where(done, torch.full_like(t, 0), t)
            d = done | (t == 0)     # noqa: F841
            lens2.add_(1)

        with torch.no_grad():
            rows = [("decode_embed", _best(embed, 400), _best(embed_aten, 400)),
                    ("next_token greedy", _best(pick(greedy), 400), _best(greedy_aten, 400)),
                    ("next_token top-50 T=0.8", _best(pick(sampled), 400), _best(sampled_aten, 400))]
        for name, t_o, t_a in rows:
            print(json.dumps({"kernel": name, "B": B, "V": V, "E": E, "us": round(t_o, 2), "aten_us": round(t_a, 2),
                              "faster_than_aten": bool(t_o < t_a)}), flush=True)


def bench_sampling(dev):
    """``next_token`` with top-p / min-p / a repetition penalty at V = 50257 against the torch composition of the
    same semantics (``ops.decode``'s ``penalise_logits`` and ``sampling_kept``, then ``torch.multinomial``); the
    arms alternate, best of 3.  ``plain top-50`` is the unchanged entry point: what top-p's 16 passes add."""
    import torch
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.ops.decode import penalise_logits, sampling_kept
    V, Lh = 50257, 128
    for B in (1, 16):
        logits = (torch.randn(B, V, device=dev) * 2).bfloat16()
        u = torch.rand(1, B, device=dev)
        out = torch.zeros(B, dtype=torch.int64, device=dev)
        history = torch.randint(0, V, (B, Lh), device=dev)
        history_lens = torch.full((B,), Lh, dtype=torch.int32, device=dev)
        inv_t = 1.0 / 0.8
        cases = [("plain top-50", dict(top_k=50), False), ("top_p=0.9", dict(top_p=0.9), False),
                 ("top-50 + top_p=0.9", dict(top_k=50, top_p=0.9), False), ("min_p=0.05", dict(min_p=0.05), False),
                 ("repetition_penalty=1.2, 128 ids", dict(repetition_penalty=1.2), True)]
        for name, kw, hist in cases:
            params = ops.next_token_params(inv_t, kw.get("top_k"), device=dev,
                                           **{k: v for k, v in kw.items() if k != "top_k"})
            h = dict(history=history, history_lens=history_lens) if hist else {}

            def ours(i):
                ops.next_token(logits, u=u, params=params, out=out, **h)

            def composed(i):
                x = penalise_logits(logits, kw["repetition_penalty"], history, history_lens, None, None) if hist \
                    else logits
                x = x.float()
                kept = sampling_kept(x, inv_t, kw.get("top_k"), kw.get("top_p", 1.0), kw.get("min_p", 0.0))
                z = torch.where(kept, x * inv_t, torch.full_like(x, float("-inf")))
                torch.multinomial(torch.softmax(z, -1), 1)

            with torch.no_grad():
                t_o = t_a = float("inf")
                for _ in range(3):
                    t_o = min(t_o, _best(ours, 400, 1))
                    t_a = min(t_a, _best(composed, 100, 1))
            print(json.dumps({"kernel": "next_token " + name, "B": B, "V": V, "us": round(t_o, 2),
                              "torch_us": round(t_a, 2), "torch_over_ours": round(t_a / t_o, 2)}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-recompute", action="store_true", help="end to end: the cached and graph arms only")
    ap.add_argument("--skip-glue", action="store_true")
    ap.add_argument("--skip-sampling", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpt2_generate_bench needs a GPU: times and rates are not measured without one")
    dev = torch.device("cuda", 0)
    if not args.skip_e2e:
        bench_e2e(dev, args)
    if not args.skip_glue:
        bench_glue(dev)
    if not args.skip_sampling:
        bench_sampling(dev)
    if not args.skip_kernels:
        bench_attention(dev)
        bench_linear(dev)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
