"""Head-dim-128 chunk (extend) attention over an FP8 KV cache with the chunk's rotation and its quantising append
(GPU only; csrc/kernels/attn_extend_d128_fp8.hip), and a head-dim-128 model through prefill, extend and a decode
step on an FP8 cache.  Inputs, `reference` and `check` (M = 2, unchanged) are tests/test_attention_extend_gqa_gpu.py's
at D = 128 (the fixture of tests/test_attention_extend_d128_gpu.py), its bf16 caches quantised by the CPU
``quantize_fp8_rows``; the reference sees the cache DEQUANTISED in its own dtype and the rotated chunk as bf16.

Edges, from the kernel's constants: cached keys come in byte tiles of 64 (scored as two halves of 32, the second
only if n reaches into it), chunk keys in bf16 tiles of 32; the instances switch at T = 16 | 17 and 32 | 33.

Measured on an MI355X, ulp term subtracted: kernel (346 comparisons) at most 1.286 (max form; routing, (4, 2),
n = (129, 64), T = 33, round 5) and 0.145 (rms; random, n = (191, 127), T = 32), plain kernel / emulation error at
most 2.33 (max; that routing case, round 1) and 1.74 (rms; routing, (8, 1), n = (1, 127), T = 17); model (4) 0.874
(max) and 0.902 (rms; both row 0, decode step), plain ratios 1.16 and 1.11.  So M = 2 holds as it stands.
"""
import copy
import math

import pytest
import torch

import test_attention_extend_gqa_gpu as X
from conftest import gpu_device
from test_attention_decode_fp8kv_gpu import quant
from test_attention_edges_gpu import check
from test_attention_extend_d128_gpu import A, N, _helpers_at_d128, _raise  # noqa: F401
from test_attention_extend_gqa_gpu import B, C, MAIN, OTHERS, _bits, _garbage, _i32
from test_llama_generate_gpu import LENS, _tokens

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.models import LlamaKVCache, cast_params, llama_tiny

pytestmark = pytest.mark.gpu
D, TC, TK, F8, U8 = 128, 64, 32, torch.float8_e4m3fn, torch.uint8
NS = [0, 1] + [e + d for e in range(TC, 257, TC) for d in (-1, 0, 1)]
PAIRS = list(zip(NS, reversed(NS)))


def run8(hh, qkv, table, cache, ns, max_len, ts=None):
    """cache = (K bytes, K scales, V bytes, V scales), copied -> out and the four tensors as the kernel left them."""
    kq, ks, vq, vs = after = [t.clone() for t in cache]
    dev = qkv.device
    out = ops.attention_extend_gqa_fp8(qkv, table, kq, vq, ks, vs, _i32(ns, dev), hh[0], hh[1], max_len,
                                       None if ts is None else _i32(ts, dev))
    torch.cuda.synchronize()
    return out, after


def check8(fails, label, hh, qkv, table, cache, ns, ts, max_len, ragged):
    """-> out, the fp64 weights and the four tensors after the call."""
    packed = X.rotate(hh, qkv, table, ns)

    def deq(dt):
        return [c.view(F8).float().to(dt) * s[..., None].to(dt) for c, s in (cache[:2], cache[2:])]

    r64, ps = X.reference(hh, packed, *deq(torch.float64), ns, ts, torch.float64)
    em = X.reference(hh, packed, *deq(torch.float32), ns, ts, torch.float32, round_p=True)[0].bfloat16()
    out, after = run8(hh, qkv, table, cache, ns, max_len, ts if ragged else None)
    assert torch.isfinite(out.float()).all(), label
    for b, t in enumerate(ts):
        assert (_bits(out[b, t:]) == 0).all(), label
    check(fails, label, out, r64, em)
    return out, ps, after


@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
@pytest.mark.parametrize("T", [1, 16, 17, 32, 33, 64, 65, 129])
def test_parity_edges(T, tight, monkeypatch):
    monkeypatch.setattr(A, "attention_extend_gqa_fp8_reference", _raise)
    dev, fails = gpu_device(), []
    for i, ns in enumerate(p for p in PAIRS if max(p) + T <= C):
        qkv, ck, cv, _ = X.make_random(MAIN, ns, T, dev, 100 * T + i)
        check8(fails, f"random n={ns} T={T}", MAIN, qkv, X.real_table(dev), quant(ck) + quant(cv), ns, (T, T),
               max(ns) if tight else C - T, False)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("hh", OTHERS, ids=str)
@pytest.mark.parametrize("T", [1, 17, 33, 49])
def test_parity_other_groups_and_ragged(hh, T, monkeypatch):
    monkeypatch.setattr(A, "attention_extend_gqa_fp8_reference", _raise)
    dev, fails = gpu_device(), []
    for i, ns in enumerate([(0, 257), (33, 160), (255, 31)]):
        qkv, ck, cv, _ = X.make_random(hh, ns, T, dev, 100 * T + i + hh[0])
        cache = quant(ck) + quant(cv)
        check8(fails, f"random {hh} n={ns} T={T}", hh, qkv, X.real_table(dev), cache, ns, (T, T),
               max(ns) if i % 2 else C - T, False)
        if T >= 2:
            ts = (T - 1, (T + 1) // 2)
            for b, t in enumerate(ts):
                qkv[b, t:] = _garbage((T - t, qkv.shape[2]), dev, T + b)
            check8(fails, f"ragged {hh} n={ns} T={T} t={ts}", hh, qkv, X.real_table(dev), cache, ns, ts,
                   C - T if i % 2 else max(ns), True)
    assert not fails, "\n".join(fails)


def candidates(n, i):
    """Targets of query i: cache keys 0 and n-1, chunk key 0, its own, both sides of every cache-tile edge (64), of
    every half tile (32) and of every chunk-tile edge (32)."""
    c = [n, n + i] + ([0, n - 1] if n else [])
    c += [e - d for e in range(TK, n, TK) for d in (1, 0)] + [n + e - d for e in range(TK, i + 1, TK) for d in (1, 0)]
    return sorted(set(c))


@pytest.mark.parametrize("hh,ns,T", [(MAIN, (129, 64), 33), (MAIN, (65, 0), 65), ((3, 1), (63, 96), 17),
                                     ((8, 1), (1, 127), 17), ((1, 1), (0, 64), 16)], ids=str)
def test_routing_scales_and_dead_rows(hh, ns, T, monkeypatch):
    """Identity table, +-1 codes, odd cache positions' keys 1.5 x their code (a target's key scale differs from its
    neighbours'; every value row has its own): every head puts >= 0.999 on its target.  The second batch row is two
    tokens short: NaN codes and NaN scales in dead cache rows and NaN bits in dead chunk rows change no bit."""
    monkeypatch.setattr(X, "candidates", candidates)
    dev, H, fails = gpu_device(), hh[0], []
    table, ts = X.identity_table(dev), (T, max(T - 2, 1))
    for rnd in range(max(len(candidates(n, T - 1)) for n in ns)):
        qkv, ck, cv, targets = X.make_routing(hh, ns, T, rnd, dev, 31 * rnd + sum(ns) + T, "zeros")
        ck[:, :, 1::2] *= 1.5
        for b, t in enumerate(ts):
            qkv[b, t:] = 0.0
        kq, ks, vq, vs = cache = quant(ck) + quant(cv)
        out, ps, _ = check8(fails, f"routing {hh} n={ns} T={T} round={rnd}", hh, qkv, table, cache, ns, ts, C - T, True)
        for b, t in enumerate(ts):
            ar = torch.arange(t, device=dev)
            for h in range(H):
                assert ps[b][h, ar, torch.tensor(targets[b][h][:t], device=dev)].min().item() >= 0.999, (rnd, b, h)
            n = ns[b]
            kq[b, :, n::2], kq[b, :, n + 1::2], vq[b, :, n:] = 0x7F, 0xFF, 0xFF
            ks[b, :, n:], vs[b, :, n:] = math.nan, math.nan
            qkv[b, t:] = math.nan
        assert torch.equal(_bits(out), _bits(run8(hh, qkv, table, cache, ns, C - T, ts)[0]))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("ns,T,ts", [((257, 0), 33, None), ((257, 0), 1, None), ((5, 300), 33, (17, 33)),
                                     ((5, 300), 1, None), ((64, 63), 33, None), ((64, 63), 1, None)], ids=str)
def test_append(ns, T, ts):
    """Rows n .. n + t - 1: V = quantize_fp8_rows(v) bit for bit; K = that of the swapped key (swap table) or, with
    the real table, within tests/test_attention_decode_fp8kv_gpu.py::test_append's bound of the fp64 rotation.
    Every other byte and scale of the four tensors is unchanged."""
    dev = gpu_device()
    H, Hkv = MAIN
    qkv, ck, cv, _ = X.make_random(MAIN, ns, T, dev, 17)
    x = qkv.view(B, T, H + 2 * Hkv, D)
    k, v = x[:, :, H:H + Hkv].permute(0, 2, 1, 3), x[:, :, H + Hkv:].permute(0, 2, 1, 3)      # [B, Hkv, T, D]
    before = quant(ck) + quant(cv)
    swap = torch.cat([torch.zeros(C, 64), torch.ones(C, 64)], 1).to(dev)
    for table in (swap, X.real_table(dev)):
        after = run8(MAIN, qkv, table, before, ns, max(ns), ts)[1]
        for b, (n, t) in enumerate(zip(ns, ts or (T, T))):
            sl, kb = slice(n, n + t), k[b, :, :t]
            gk, gks, gv, gvs = (a[b, :, sl] for a in after)
            wq, ws = quant(v[b, :, :t])
            assert torch.equal(gv, wq) and torch.equal(gvs, ws)
            if table is swap:
                wq, ws = quant(torch.cat([-kb[..., 64:], kb[..., :64]], -1))
                assert torch.equal(gk, wq) and torch.equal(gks, ws)
            else:
                row, k1, k2 = table[sl].double(), kb[..., :64].double(), kb[..., 64:].double()
                w = torch.cat([k1 * row[:, :64] - k2 * row[:, 64:], k2 * row[:, :64] + k1 * row[:, 64:]], -1)
                sc = gks.double().unsqueeze(-1)
                ulp = torch.ldexp(torch.ones_like(w), torch.frexp(w).exponent - 8)
                bound = ulp + torch.maximum((w.abs() + ulp) / 16, sc / 1024) * (1 + 17 * 2.0 ** -24)
                assert ((gk.view(F8).float().double() * sc - w).abs() <= bound).all()
        for got, old in zip(after, before):
            want = old.clone()
            for b, (n, t) in enumerate(zip(ns, ts or (T, T))):
                want[b, :, n:n + t] = got[b, :, n:n + t]
            assert torch.equal(got.view(U8), want.view(U8))      # (bytes: NaN scales of dead rows compare equal)


def test_every_code_through_the_append():
    """A chunk whose V rows carry every e4m3 code at scale 1 (amax 448), and their negatives, comes back as them."""
    dev = gpu_device()
    codes = torch.arange(127, dtype=U8).view(F8).float()
    pos = torch.cat([codes, codes[-1:]])
    x = torch.randn(B, 2, 3, D)
    x[:, 0, 2], x[:, 1, 2] = pos, -pos
    cache = [torch.zeros(B, 1, 4, D, dtype=U8, device=dev), torch.zeros(B, 1, 4, device=dev),
             torch.zeros(B, 1, 4, D, dtype=U8, device=dev), torch.zeros(B, 1, 4, device=dev)]
    after = run8((1, 1), x.view(B, 2, -1).bfloat16().to(dev), X.identity_table(dev), cache, (0, 1), 1)[1]
    want = torch.cat([torch.arange(127), torch.tensor([126])]).to(U8).to(dev)
    for b, n in enumerate((0, 1)):
        assert torch.equal(after[2][b, 0, n], want) and torch.equal(after[2][b, 0, n + 1, 1:], want[1:] | 0x80)
        assert after[3][b, 0, n:n + 2].tolist() == [1.0, 1.0]


def test_dispatch(monkeypatch):
    """D = 128 and the five group sizes run the kernel; an unaligned cache view and G = 5 run the reference."""
    dev = gpu_device()
    assert N.supported_extend_fp8(4, 2, 128) and not N.supported_extend_fp8(5, 1, 128)
    assert not N.supported_extend_fp8(4, 2, 64)

    def go(hh, shift=0):
        qkv, ck, cv, _ = X.make_random(hh, (3, 70), 5, dev, 3)
        cache = list(quant(ck) + quant(cv))
        for i in (0, 2):    # the same bytes at an address that is shift past a 16-byte boundary
            flat = torch.empty(cache[i].numel() + 16, dtype=U8, device=dev)
            off = (shift - flat.data_ptr()) % 16
            cache[i] = flat[off:off + cache[i].numel()].view(cache[i].shape).copy_(cache[i])
        kq, ks, vq, vs = cache
        return ops.attention_extend_gqa_fp8(qkv, X.real_table(dev), kq, vq, ks, vs, _i32((3, 70), dev), *hh, 70)

    with monkeypatch.context() as m:
        m.setattr(A, "attention_extend_gqa_fp8_reference", _raise)
        for hh in [MAIN] + OTHERS:
            assert torch.isfinite(go(hh).float()).all()
    monkeypatch.setattr(N, "attention_extend_gqa_fp8", _raise)
    assert torch.isfinite(go(MAIN, 8).float()).all() and torch.isfinite(go((5, 1)).float()).all()


def test_model_fp8_extend(monkeypatch):
    """`prefill` of a prefix, `extend` with ragged `new_lens`, a `decode_step`, all on an FP8 cache: the logits against
    an fp64 copy on the reference fp8 ops (over the dequantised cache; emulation: the bf16 copy on those ops).  Then
    `generate(prefix=..., kv_cache_dtype="fp8")` under a graph equals the eager call token for token."""
    dev, fails = gpu_device(), []
    torch.manual_seed(0)
    model = llama_tiny(hidden_size=256).eval().to(dev)
    cast_params(model, torch.bfloat16)
    prompts, forced = _tokens()
    S, first = max(LENS), [3, 40]
    head, tail = torch.zeros(len(LENS), first[1], dtype=torch.long), torch.zeros(len(LENS), S - first[1], dtype=torch.long)
    for b, r in enumerate(prompts):
        head[b, :first[b]], tail[b, :len(r) - first[b]] = r[:first[b]], r[first[b]:]

    def roll(m, d):
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=d)  # noqa: E731
        cache = LlamaKVCache.allocate(m, len(LENS), S + 1, fp8=True)
        m.prefill(head.to(d), i32(first), cache)
        out = [m.extend(tail.to(d), cache, i32([n - f for n, f in zip(LENS, first)]))]
        out.append(m.decode_step(forced[:, 0].to(d), cache))
        assert cache.lens.tolist() == [n + 1 for n in LENS]
        return torch.stack(out).double().cpu()

    with torch.no_grad():
        ref, em = roll(copy.deepcopy(model).cpu().double(), "cpu"), roll(copy.deepcopy(model).cpu(), "cpu")
        monkeypatch.setattr(A, "attention_extend_gqa_fp8_reference", _raise)
        got = roll(model, dev)
    for t, name in enumerate(("extend", "decode step")):
        for b in range(len(LENS)):
            check(fails, f"row {b} {name}", got[t, b], ref[t, b], em[t, b])
    assert not fails, "\n".join(fails)
    prefix = LlamaKVCache.allocate(model, len(LENS), first[1], fp8=True)
    model.prefill(head.to(dev), torch.tensor(first, dtype=torch.int32, device=dev), prefix)
    ids = tail.to(dev)
    mask = (torch.arange(tail.shape[1])[None] < (torch.tensor(LENS) - torch.tensor(first))[:, None]).long()
    runs = [model.generate(ids, attention_mask=mask.to(dev), max_new_tokens=4, prefix=prefix, kv_cache_dtype="fp8",
                           use_graph=g) for g in (False, True)]
    assert torch.equal(*runs)
