"""Chunk attention over a KV cache with the append (GPU only; csrc/kernels/attn_extend.hip).

Every case has two batch rows of DIFFERENT cached lengths n (B = 2, H = 2, C = 384).

Boundaries the kernel has.  Keys come in tiles of 64, the cache part first (tiles at 64 k, the last one cut
by n), then the chunk part (tiles at 64 k of the chunk, the last one cut by the diagonal).  A workgroup is
1 / 2 / 4 waves of 16 queries for T <= 16 / <= 32 / more, so the query tile is 16, 32 or 64 and T = 16 | 17 and
32 | 33 switch the instance; 64 | 65 and 128 | 129 add a query tile (and a chunk key tile).  Inside a tile a lane
owns keys 4 g .. 4 g + 3 of each 16-key block.  Cached lengths: the issue's {0, 1, 63, 64, 65, 127, 128, 129, 255,
256, 257} plus 191, 192, 193 (the third tile edge); chunk lengths: the issue's {1, 7, 16, 17, 63, 64, 65, 127}
plus 15, 31, 32, 33, 128, 129.  Every pair with max n + T <= C runs, each -- the ragged `new_lens` cases too --
with max_len = max n (tight) and max_len = C - T; (257, T = 127) is n + T = C, the last slot.

Tolerance: the form of tests/test_attention_edges_gpu.py (`check`, M = 2): reference fp64 from the bf16
inputs; the emulation has fp32 scores and softmax, P rounded to bf16 and a bf16 output.  Every case prints
its ratios.

Measured on an MI355X: 773 comparisons in this file.  With the ulp term subtracted the largest ratios are 0.76
(max form; random inputs, n = (193, 64), T = 1) and 0.115 (rms form; random, n = (127, 191), T = 17); as plain
kernel error / emulation error the largest are 1.64 (max) and 1.17 (rms), both in that T = 1 case (256 output
values).  So M = 2 holds as it stands.
"""
import math

import pytest
import torch

from conftest import gpu_device
from test_attention_edges_gpu import D, M, _split, check  # noqa: F401

from databricks_distributed_deep_learning_amd import ops

pytestmark = pytest.mark.gpu

B, H, C = 2, 2, 384
NS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257]
TS = [1, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]
PAIRS = list(zip(NS, reversed(NS)))
SCALE = 1.0 / math.sqrt(D)


def _garbage(shape, dev, seed):
    """Arbitrary bf16 bit patterns, NaN and Inf among them."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-32768, 32767, shape, generator=g, dtype=torch.int16).to(dev).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16)


def _i32(v, dev):
    return torch.tensor(list(v), dtype=torch.int32, device=dev)


def make_random(ns, T, dev, seed):
    """qkv_new [B, T, 3 H D], caches [B, H, C, D] (live rows randn, the rest arbitrary bits), lens int32."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).bfloat16().to(dev)
    ck, cv = _garbage((B, H, C, D), dev, seed + 1), _garbage((B, H, C, D), dev, seed + 2)
    for b, n in enumerate(ns):
        ck[b, :, :n] = torch.randn(H, n, D, generator=g).bfloat16().to(dev)
        cv[b, :, :n] = torch.randn(H, n, D, generator=g).bfloat16().to(dev)
    return qkv, ck, cv, _i32(ns, dev)


def reference(qkv, ck, cv, ns, ts, dt, round_p=False):
    """out [B, T, H D] (rows >= t zeros) in dtype dt and, per batch row, the weights [H, t, n + t] over the keys
    cache 0 .. n-1, chunk 0 .. t-1.  round_p: P rounded to bf16 before P V (the kernel's precision)."""
    T = qkv.shape[1]
    q, k, v = _split(qkv.to(dt), H)
    out = torch.zeros(B, T, H * D, dtype=dt, device=qkv.device)
    ps = []
    for b, (n, t) in enumerate(zip(ns, ts)):
        kk = torch.cat([ck[b, :, :n].to(dt), k[b, :, :t]], 1)
        vv = torch.cat([cv[b, :, :n].to(dt), v[b, :, :t]], 1)
        s = (q[b, :, :t] @ kk.transpose(-1, -2)) * SCALE
        i, j = torch.arange(t, device=qkv.device), torch.arange(n + t, device=qkv.device)
        p = torch.softmax(s.masked_fill(j[None, :] > n + i[:, None], -math.inf), -1)
        ps.append(p)
        if round_p:
            p = p.bfloat16().to(dt)
        out[b, :t] = (p @ vv).permute(1, 0, 2).reshape(t, H * D)
    return out, ps


def run(qkv, ck, cv, lens, max_len, new_lens=None):
    out = ops.attention_extend(qkv, ck, cv, lens, H, max_len, new_lens)
    torch.cuda.synchronize()
    return out


def _check_case(fails, label, qkv, ck, cv, ns, ts, max_len, ragged):
    dev = qkv.device
    r64, _ = reference(qkv, ck, cv, ns, ts, torch.float64)
    em = reference(qkv, ck, cv, ns, ts, torch.float32, round_p=True)[0].bfloat16()
    out = run(qkv, ck.clone(), cv.clone(), _i32(ns, dev), max_len, _i32(ts, dev) if ragged else None)
    assert torch.isfinite(out.float()).all(), label
    for b, t in enumerate(ts):
        assert (_bits(out[b, t:]) == 0).all(), label
    check(fails, label, out, r64, em)


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
@pytest.mark.parametrize("T", TS)
def test_parity_random(T, tight):
    dev = gpu_device()
    fails = []
    for i, ns in enumerate(PAIRS):
        if max(ns) + T > C:
            continue
        qkv, ck, cv, _ = make_random(ns, T, dev, 100 * T + i)
        _check_case(fails, f"random n={ns} T={T}", qkv, ck, cv, ns, (T, T), max(ns) if tight else C - T, False)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
@pytest.mark.parametrize("T", [t for t in TS if t >= 2])
def test_parity_ragged_new_lens(T, tight):
    dev = gpu_device()
    fails = []
    for i, ns in enumerate([(257, 0), (64, 129), (1, 255), (192, 63)]):
        if max(ns) + T > C:
            continue
        for ts in ((1, T), (T - 1, 2), (T, (T + 1) // 2)):
            qkv, ck, cv, _ = make_random(ns, T, dev, 7 * T + i)
            for b, t in enumerate(ts):      # padded columns: arbitrary bits
                qkv[b, t:] = _garbage((T - t, 3 * H * D), dev, T + b)
            _check_case(fails, f"ragged n={ns} T={T} t={ts}", qkv, ck, cv, ns, ts, max(ns) if tight else C - T, True)
    assert not fails, "\n".join(fails)


def test_last_slot():
    """n + T = C exactly, in both rows, tight bound = C - T."""
    dev = gpu_device()
    fails = []
    for T in (1, 17, 127):
        ns = (C - T, C - T)
        qkv, ck, cv, _ = make_random(ns, T, dev, T)
        _check_case(fails, f"last slot T={T}", qkv, ck, cv, ns, (T, T), C - T, False)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ routing
def candidates(n, i):
    """Key indices (cache 0 .. n-1, then chunk 0 .. i at n ..) query i is steered to: cache key 0, cache key
    n-1, chunk key 0, its own key, and the first and last key of every key tile of both parts."""
    c = [n, n + i]
    if n:
        c += [0, n - 1]
    for e in range(64, n, 64):
        c += [e - 1, e]
    for e in range(64, i + 1, 64):
        c += [n + e - 1, n + e]
    return sorted(set(c))


def make_routing(ns, T, rnd, dev, seed, dead=None):
    """K = +-1 codes, q_i = 4 code[target_i], V = randn: query i's whole weight sits on one key.  Returns the
    targets [B][H][T] too.  dead: None (arbitrary bits) | 'zeros' | 'decoys' (K = 2 x a target's code, V = 8)
    | 'nan'."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.empty(B, T, 3, H, D)
    ck, cv = _garbage((B, H, C, D), "cpu", seed + 1), _garbage((B, H, C, D), "cpu", seed + 2)
    targets = [[None] * H for _ in range(B)]
    for b, n in enumerate(ns):
        for h in range(H):
            code = torch.randint(0, 2, (n + T, D), generator=g).float() * 2 - 1
            val = torch.randn(n + T, D, generator=g)
            tg = []
            for i in range(T):
                cand = candidates(n, i)
                tg.append(cand[(i + rnd + h) % len(cand)])
            targets[b][h] = tg
            ck[b, h, :n], cv[b, h, :n] = code[:n].bfloat16(), val[:n].bfloat16()
            qkv[b, :, 0, h], qkv[b, :, 1, h], qkv[b, :, 2, h] = 4.0 * code[tg], code[n:], val[n:]
            if dead == "zeros":
                ck[b, h, n:], cv[b, h, n:] = 0.0, 0.0
            elif dead == "decoys":
                ck[b, h, n:], cv[b, h, n:] = (2.0 * code[tg[-1]]).bfloat16(), 8.0
            elif dead == "nan":
                ck[b, h, n:], cv[b, h, n:] = math.nan, math.nan
    return qkv.reshape(B, T, 3 * H * D).bfloat16().to(dev), ck.to(dev), cv.to(dev), targets


@pytest.mark.parametrize("ns,T", [((129, 64), 65), ((257, 0), 127), ((1, 65), 17), ((63, 128), 16), ((192, 5), 129)],
                         ids=str)
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
def test_routing(ns, T, tight):
    dev = gpu_device()
    fails = []
    rounds = max(len(candidates(n, T - 1)) for n in ns)
    for rnd in range(rounds):
        qkv, ck, cv, targets = make_routing(ns, T, rnd, dev, 31 * rnd + sum(ns) + T)
        r64, ps = reference(qkv, ck, cv, ns, (T, T), torch.float64)
        em = reference(qkv, ck, cv, ns, (T, T), torch.float32, round_p=True)[0].bfloat16()
        out = run(qkv, ck.clone(), cv.clone(), _i32(ns, dev), max(ns) if tight else C - T)
        _, _, v = _split(qkv, H)
        for b, n in enumerate(ns):
            vv = torch.cat([cv[b, :, :n], v[b]], 1).float()         # [H, n + T, D]
            for h in range(H):
                tg = torch.tensor(targets[b][h], device=dev)
                w = ps[b][h, torch.arange(T, device=dev), tg]
                assert w.min().item() >= 0.999, (ns, T, rnd, b, h, w.min().item())
                got = out[b, :, h * D:(h + 1) * D].float()
                torch.testing.assert_close(got, vv[h, tg], rtol=2.0 ** -7, atol=0.03)
        check(fails, f"routing n={ns} T={T} round={rnd}", out, r64, em)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ leaks
@pytest.mark.parametrize("ns,T", [((255, 63), 65), ((128, 7), 16), ((0, 193), 127)], ids=str)
def test_dead_tail_cannot_reach_the_output(ns, T):
    dev = gpu_device()
    outs = []
    for dead in ("zeros", "decoys", "nan"):
        qkv, ck, cv, _ = make_routing(ns, T, 1, dev, 5, dead)
        outs.append(run(qkv, ck, cv, _i32(ns, dev), C - T))
        assert torch.isfinite(outs[-1].float()).all()
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))


@pytest.mark.parametrize("ns,T", [((129, 0), 66), ((64, 5), 17), ((1, 200), 130)], ids=str)
def test_next_chunk_key_cannot_move_a_query(ns, T):
    """A decoy at chunk key i + 1 (K = 2 x query i's target code: it would win; V = 8) leaves rows 0 .. i bitwise
    as they were; query i's reference weight on its target is >= 0.999, so a leak would move it by O(1)."""
    dev = gpu_device()
    qkv, ck, cv, targets = make_routing(ns, T, 0, dev, 11)
    _, ps = reference(qkv, ck, cv, ns, (T, T), torch.float64)
    base = run(qkv, ck.clone(), cv.clone(), _i32(ns, dev), max(ns))
    for i in sorted({0, 14, 15, 16, 30, 31, 32, 62, 63, 64, 126, 127, 128, T - 2} & set(range(T - 1))):
        x = qkv.clone().view(B, T, 3, H, D)
        for b in range(B):
            for h in range(H):
                assert ps[b][h, i, targets[b][h][i]].item() >= 0.999
                x[b, i + 1, 1, h] = 0.5 * x[b, i, 0, h]        # q_i = 4 code[target]: 2 x the code
                x[b, i + 1, 2, h] = 8.0
        out = run(x.view(B, T, 3 * H * D), ck.clone(), cv.clone(), _i32(ns, dev), max(ns))
        assert torch.equal(_bits(out[:, :i + 1]), _bits(base[:, :i + 1])), i


@pytest.mark.parametrize("ns,T,ts", [((129, 0), 66, (64, 1)), ((64, 5), 17, (16, 15)), ((1, 200), 130, (65, 129))], ids=str)
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
def test_padded_columns_cannot_move_a_valid_query(ns, T, ts, tight):
    """Chunk rows i >= t as zeros, as decoys (K = 2 x the last valid query's target code, V = 8, q = the same) and
    as NaN: the outputs and the caches are bitwise equal."""
    dev = gpu_device()
    res = []
    for mode in ("zeros", "decoys", "nan"):
        qkv, ck, cv, targets = make_routing(ns, T, 2, dev, 13)
        x = qkv.view(B, T, 3, H, D)
        for b, t in enumerate(ts):
            if mode == "zeros":
                x[b, t:] = 0.0
            elif mode == "nan":
                x[b, t:] = math.nan
            else:
                x[b, t:, 0], x[b, t:, 1], x[b, t:, 2] = x[b, t - 1, 0], 0.5 * x[b, t - 1, 0], 8.0
        out = run(qkv, ck, cv, _i32(ns, dev), max(ns) if tight else C - T, _i32(ts, dev))
        assert torch.isfinite(out.float()).all()
        res.append((out, ck, cv))
    for other in res[1:]:
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(res[0], other))


# ------------------------------------------------------------------ append, repeatability
@pytest.mark.parametrize("ns,T,ts", [((257, 0), 127, None), ((64, 63), 65, (1, 65)), ((5, 128), 16, (15, 2)),
                                     ((383, 320), 1, None), ((0, 191), 129, (128, 129))], ids=str)
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
def test_append(ns, T, ts, tight):
    """cache[b, h, n_b + i] becomes chunk row i's K / V for i < t_b; nothing else changes (n + T = C, the last
    slot, included); lens and new_lens are not written."""
    dev = gpu_device()
    qkv, ck, cv, lt = make_random(ns, T, dev, 17)
    wk, wv = ck.clone(), cv.clone()
    _, k, v = _split(qkv, H)
    tt = ts or (T, T)
    for b, (n, t) in enumerate(zip(ns, tt)):
        wk[b, :, n:n + t], wv[b, :, n:n + t] = k[b, :, :t], v[b, :, :t]
    nl = None if ts is None else _i32(ts, dev)
    run(qkv, ck, cv, lt, max(ns) if tight else C - T, nl)
    assert torch.equal(_bits(ck), _bits(wk)) and torch.equal(_bits(cv), _bits(wv))
    assert lt.tolist() == list(ns) and (nl is None or nl.tolist() == list(ts))


def test_repeatable():
    dev = gpu_device()
    for ns, T in (((250, 3), 129), ((100, 64), 16)):
        qkv, ck, cv, lt = make_random(ns, T, dev, 23)
        runs = []
        for _ in range(3):
            k, v = ck.clone(), cv.clone()
            runs.append((run(qkv, k, v, lt, C - T), k, v))
        for other in runs[1:]:
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(runs[0], other))


# ------------------------------------------------------------------ prefill + extend + decode chain
def _causal(qkv, dt, round_p=False):
    q, k, v = _split(qkv.to(dt), H)
    S = qkv.shape[1]
    s = (q @ k.transpose(-1, -2)) * SCALE
    ar = torch.arange(S, device=qkv.device)
    p = torch.softmax(s.masked_fill(ar[None, :] > ar[:, None], -math.inf), -1)
    if round_p:
        p = p.bfloat16().to(dt)
    return (p @ v).permute(0, 2, 1, 3).reshape(qkv.shape[0], S, H * D)


def test_prefill_extend_decode_chain():
    """Native causal prefill of 65 tokens + fill, extends of T = 1, 16 and 65, one decode step: each result is its
    row range of one causal attention over all 148 tokens."""
    from databricks_distributed_deep_learning_amd.ops import _native_attention as NA
    dev = gpu_device()
    S0, chunks = 65, (1, 16, 65)
    S = S0 + sum(chunks) + 1
    qkv = torch.randn(B, S, 3 * H * D, device=dev).bfloat16()
    r64, em = _causal(qkv, torch.float64), _causal(qkv, torch.float32, True).bfloat16()
    ck, cv = _garbage((B, H, C, D), dev, 1), _garbage((B, H, C, D), dev, 2)
    pre = qkv[:, :S0].contiguous()
    fails = []
    check(fails, "chain prefill", NA.attention(pre, H, None, 0.0, causal=True), r64[:, :S0], em[:, :S0])
    ops.kv_cache_fill(pre, ck, cv, H)
    lens, at = torch.full((B,), S0, dtype=torch.int32, device=dev), S0
    for T in chunks:
        out = run(qkv[:, at:at + T].contiguous(), ck, cv, lens, at)
        check(fails, f"chain extend T={T}", out, r64[:, at:at + T], em[:, at:at + T])
        lens += T
        at += T
    out = ops.attention_decode(qkv[:, at].contiguous(), ck, cv, lens, H, at + 1)
    check(fails, "chain decode", out, r64[:, at], em[:, at])
    _, k, v = _split(qkv, H)
    assert torch.equal(_bits(ck[:, :, :S]), _bits(k)) and torch.equal(_bits(cv[:, :, :S]), _bits(v))
    assert not fails, "\n".join(fails)


def test_capacity_guard_is_on_the_host():
    dev = gpu_device()
    qkv, ck, cv, lt = make_random((3, 4), 5, dev, 1)
    with pytest.raises(ValueError, match="capacity"):
        ops.attention_extend(qkv, ck, cv, lt, H, C - 4)
    with pytest.raises(RuntimeError, match="autograd"):
        ops.attention_extend(qkv.clone().requires_grad_(True), ck, cv, lt, H, 4)
