"""Head-dim-128 rotary grouped-query chunk attention with the chunk's rotation and the append (GPU only;
csrc/kernels/attn_extend_d128.hip), and a head-dim-128 model through chunked prefill, extend and a decode step.

Inputs, references and the tolerance (`check`, M = 2, unchanged) are tests/test_attention_extend_gqa_gpu.py's, whose
helpers read the head dimension from that module's ``D``: the fixture below points them (and ``_split``'s ``D``) at
128 and their key-tile edges at this kernel's.  B = 2 rows of DIFFERENT cached lengths, C = 384.  At D = 128
``rotate`` goes through ``rope_qkv``'s reference, so appended keys are compared with an fp64 rotation to one bf16
ulp (the kernel may contract ``a c - b s`` into an FMA), not bit for bit.

Edges, from the kernel's constants.  Keys come in tiles of 32: cached lengths 0, 1 and +-1 around 32, 64, ... 256
(a cache tile cut by n; with n = 0 no DMA'd K tile at all).  A workgroup is G x NS waves, NS = 1 / 2 / 4 for
T <= 16 / <= 32 / more, capped at 4 (G <= 2), 2 (G = 3, 4), 1 (G = 8).  For (4, 2): T = 16 | 17 and 32 | 33 switch the
instance (16 | 17 also leaves the 128-thread one), 64 | 65 and 128 | 129 add a 64-query tile, and 31 | 32 | 33 and
63 | 64 | 65 are chunk key-tile edges as well; T = 1 is the decode-sized chunk.  From T = 33 the query tile is wider
than the key tile, so some sub-tiles sit a chunk tile out.  (1, 1) has the 64-thread instance that rotates on
arrival; (3, 1) the uneven split of DMA instructions and rotation pairs over 3 or 6 waves (32 | 33, 64 | 65, 96 | 97
add a tile); (8, 1) the half-pair instance, a query tile every 16 (48 | 49); (4, 1) the 256-thread one and, from
T = 17, half pairs.  Every (n pair, T) with n + T <= C runs at the tight max_len and at max_len = C - T;
(257, T = 127) is n + T = C, the last slot.

Measured on an MI355X, ulp term subtracted: kernel (1125 comparisons) at most 0.458 (max form; random, (4, 2),
n = (96, 161), T = 1) and 0.079 (rms; n = (127, 159), T = 1), plain kernel / emulation error at most 1.33 (max;
(3, 1), n = (255, 31), T = 1) and 1.10 (rms; (1, 1), n = (33, 160), T = 1); model (6) 0.464 (max; row 0, chunked
prefill) and 0.448 (rms; row 0, decode step), plain / forward error at most 1.07.  So M = 2 holds as it stands.
"""
import importlib
import math

import pytest
import torch

import test_attention_edges_gpu as E
import test_attention_extend_gqa_gpu as X
from conftest import gpu_device
from test_attention_edges_gpu import check
from test_attention_extend_gqa_gpu import B, C, MAIN, OTHERS, _bits, _garbage, _i32
from test_llama_generate_gpu import LENS, _tokens, forward64

from databricks_distributed_deep_learning_amd.models import LlamaKVCache, cast_params, llama_tiny
from databricks_distributed_deep_learning_amd.ops import _native_attn_cache as N

A = importlib.import_module("databricks_distributed_deep_learning_amd.ops.attention")    # the module, not the op
pytestmark = pytest.mark.gpu

D, TK = 128, 32
NS = [0, 1] + [e + d for e in range(TK, 257, TK) for d in (-1, 0, 1)]
PAIRS = list(zip(NS, reversed(NS)))
TS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]
TS_RED = [1, 16, 17, 32, 33, 49, 64, 65, 97]
PAIRS_RED = [(0, 257), (33, 160), (96, 1), (255, 31)]


def candidates(n, i):
    """Targets of query i: cache keys 0 and n-1, chunk key 0, its own (the diagonal), both sides of every tile edge."""
    c = [n, n + i] + ([0, n - 1] if n else [])
    c += [e - d for e in range(TK, n, TK) for d in (1, 0)] + [n + e - d for e in range(TK, i + 1, TK) for d in (1, 0)]
    return sorted(set(c))


@pytest.fixture(autouse=True)
def _helpers_at_d128(monkeypatch):
    for mod, name, v in ((X, "D", D), (E, "D", D), (X, "SCALE", 1.0 / math.sqrt(D)), (X, "_TABLES", {}),
                         (X, "candidates", candidates)):
        monkeypatch.setattr(mod, name, v)


def _raise(*a, **k):
    raise AssertionError("the reference path was taken")


def _ragged(fails, hh, ns, T, ts, max_len, dev, seed):
    qkv, ck, cv, _ = X.make_random(hh, ns, T, dev, seed)
    for b, t in enumerate(ts):
        qkv[b, t:] = _garbage((T - t, qkv.shape[2]), dev, T + b)
    X._check_case(fails, f"ragged {hh} n={ns} T={T} t={ts}", hh, qkv, X.real_table(dev), ck, cv, ns, ts, max_len, True)


@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
@pytest.mark.parametrize("T", TS)
def test_parity_edges(T, tight):
    dev, fails = gpu_device(), []
    for i, ns in enumerate(p for p in PAIRS if max(p) + T <= C):
        qkv, ck, cv, _ = X.make_random(MAIN, ns, T, dev, 100 * T + i)
        X._check_case(fails, f"random n={ns} T={T}", MAIN, qkv, X.real_table(dev), ck, cv, ns, (T, T),
                      max(ns) if tight else C - T, False)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("hh", OTHERS, ids=str)
@pytest.mark.parametrize("T", TS_RED)
def test_parity_other_groups(hh, T):
    dev, fails = gpu_device(), []
    for i, ns in enumerate(p for p in PAIRS_RED if max(p) + T <= C):
        qkv, ck, cv, _ = X.make_random(hh, ns, T, dev, 100 * T + i + hh[0])
        X._check_case(fails, f"random {hh} n={ns} T={T}", hh, qkv, X.real_table(dev), ck, cv, ns, (T, T),
                      max(ns) if i % 2 else C - T, False)
        if T >= 2:
            _ragged(fails, hh, ns, T, (T - 1, (T + 1) // 2), C - T if i % 2 else max(ns), dev, 100 * T + i)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("T", [t for t in TS if t >= 2])
def test_parity_ragged_new_lens(T):
    dev, fails = gpu_device(), []
    for i, ns in enumerate(p for p in [(257, 0), (32, 129), (1, 255), (160, 31)] if max(p) + T <= C):
        for ts in ((1, T), (T - 1, 2), (T, (T + 1) // 2)):
            _ragged(fails, MAIN, ns, T, ts, max(ns) if i % 2 else C - T, dev, 7 * T + i)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("hh,ns,T", [(MAIN, (65, 32), 33), (MAIN, (129, 0), 65), ((3, 1), (33, 96), 33),
                                     ((8, 1), (31, 1), 17), ((1, 1), (0, 64), 16), ((4, 1), (95, 2), 49)], ids=str)
def test_routing_and_dead_cache_rows(hh, ns, T):
    """Identity table, +-1 codes: each query head of a group aims at its own key, KV heads hold different codes.  The
    targets walk both sides of every tile edge and the diagonal.  NaN dead cache rows give the zero rows' bits."""
    dev, H, fails = gpu_device(), hh[0], []
    table, ar = X.identity_table(dev), torch.arange(T, device=dev)
    for rnd in range(max(len(candidates(n, T - 1)) for n in ns)):
        seed = 31 * rnd + sum(ns) + T
        qkv, ck, cv, targets = X.make_routing(hh, ns, T, rnd, dev, seed, "zeros")
        packed = X.rotate(hh, qkv, table, ns)
        r64, ps = X.reference(hh, packed, ck, cv, ns, (T, T), torch.float64)
        em = X.reference(hh, packed, ck, cv, ns, (T, T), torch.float32, round_p=True)[0].bfloat16()
        out = X.run(hh, qkv, table, ck.clone(), cv.clone(), _i32(ns, dev), C - T)
        for b, n in enumerate(ns):
            vv = X._values(hh, qkv, cv, b, n)
            for h in range(H):
                tg = torch.tensor(targets[b][h], device=dev)
                assert ps[b][h, ar, tg].min().item() >= 0.999, (rnd, b, h)
                torch.testing.assert_close(out[b, :, h * D:(h + 1) * D].float(), vv[h, tg], rtol=2.0 ** -7, atol=0.03)
        check(fails, f"routing {hh} n={ns} T={T} round={rnd}", out, r64, em)
        qn, kn, vn, _ = X.make_routing(hh, ns, T, rnd, dev, seed, "nan")
        assert torch.equal(_bits(out), _bits(X.run(hh, qn, table, kn, vn, _i32(ns, dev), C - T)))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("ns,T,ts", [((33, 0), 66, (64, 1)), ((64, 5), 17, (16, 15)), ((1, 200), 34, (33, 32))], ids=str)
def test_padded_rows_and_the_next_key_cannot_move_a_query(ns, T, ts):
    """Chunk rows i >= t as zeros and as NaN: the outputs and the caches are bitwise equal.  A decoy at chunk key
    i + 1 (K = 2 x the target code of query i: it would win; V = 8) leaves output rows 0 .. i bitwise as they were."""
    dev = gpu_device()
    H, Hkv = MAIN
    G, table = H // Hkv, X.identity_table(dev)
    res = []
    for fill in (0.0, math.nan):
        qkv, ck, cv, targets = X.make_routing(MAIN, ns, T, 2, dev, 13)
        for b, t in enumerate(ts):
            qkv[b, t:] = fill
        res.append((X.run(MAIN, qkv, table, ck, cv, _i32(ns, dev), C - T, _i32(ts, dev)), ck, cv))
    assert torch.isfinite(res[1][0].float()).all()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*res))
    qkv, ck, cv, targets = X.make_routing(MAIN, ns, T, 0, dev, 11)
    base = X.run(MAIN, qkv, table, ck.clone(), cv.clone(), _i32(ns, dev), max(ns))
    for i in sorted({0, 14, 15, 16, 30, 31, 32, 62, 63, 64, T - 2} & set(range(T - 1))):
        x = qkv.clone().view(B, T, H + 2 * Hkv, D)
        for j in range(Hkv):
            x[:, i + 1, H + j] = 0.5 * x[:, i, j * G]          # q_i = 4 code[target]: 2 x the code
            x[:, i + 1, H + Hkv + j] = 8.0
        out = X.run(MAIN, x.view(B, T, -1), table, ck.clone(), cv.clone(), _i32(ns, dev), max(ns))
        assert torch.equal(_bits(out[:, :i + 1]), _bits(base[:, :i + 1])), i


@pytest.mark.parametrize("hh,ns,T,ts", [(MAIN, (257, 0), 127, None), (MAIN, (31, 64), 33, (1, 33)),
                                        ((3, 1), (100, 7), 17, (17, 9)), ((8, 1), (1, 64), 49, (48, 49)),
                                        ((1, 1), (63, 0), 16, (15, 16))], ids=str)
def test_rotation_and_append(hh, ns, T, ts):
    """cache[b, :, n_b + i] becomes chunk row i's rotated key (swap table: exactly [-k[64:], k[:64]]; real: within one
    bf16 ulp of an fp64 rotation) and its value's bits for i < t_b, the last slot too; nothing else changes."""
    dev = gpu_device()
    H, Hkv = hh
    qkv, ck0, cv0, lt = X.make_random(hh, ns, T, dev, 17)
    x = qkv.view(B, T, H + 2 * Hkv, D)
    k, v = x[:, :, H:H + Hkv].permute(0, 2, 1, 3), x[:, :, H + Hkv:].permute(0, 2, 1, 3)      # [B, Hkv, T, D]
    swap = torch.cat([torch.zeros(C, 64), torch.ones(C, 64)], 1).to(dev)
    for table in (swap, X.real_table(dev)):
        ck, cv, wk, wv = ck0.clone(), cv0.clone(), ck0.clone(), cv0.clone()
        X.run(hh, qkv, table, ck, cv, lt, C - T, None if ts is None else _i32(ts, dev))
        for b, (n, t) in enumerate(zip(ns, ts or (T, T))):
            got, kb = ck[b, :, n:n + t], k[b, :, :t]
            if table is swap:
                assert torch.equal(_bits(got), _bits(torch.cat([-kb[..., 64:], kb[..., :64]], -1)))
            else:
                row, k1, k2 = table[n:n + t].double(), kb[..., :64].double(), kb[..., 64:].double()
                cos, sin = row[:, :64], row[:, 64:]
                w = torch.cat([k1 * cos - k2 * sin, k2 * cos + k1 * sin], -1).bfloat16().double()
                assert ((got.double() - w).abs() <= torch.ldexp(torch.ones_like(w), torch.frexp(w).exponent - 8)).all()
            wk[b, :, n:n + t], wv[b, :, n:n + t] = got, v[b, :, :t]
        assert torch.equal(_bits(ck), _bits(wk)) and torch.equal(_bits(cv), _bits(wv)) and lt.tolist() == list(ns)


def test_routes_to_the_kernel(monkeypatch):
    dev = gpu_device()
    assert N.supported_extend(4, 2, 128) and N.supported_extend(4, 2) and not N.supported(4, 2, 128)
    assert all(N.supported_extend(*hh, 128) for hh in OTHERS) and not N.supported_extend(5, 1, 128)
    assert [N.tile(T, 4, 2, 128) for T in (16, 17, 32, 33)] == [16, 32, 32, 64]
    assert [N.tile(T, 3, 1, 128) for T in (16, 17, 33)] == [16, 32, 32] and N.tile(129, 8, 1, 128) == 16
    monkeypatch.setattr(A, "attention_extend_gqa_reference", _raise)
    qkv, ck, cv, lt = X.make_random(MAIN, (250, 3), 129, dev, 23)
    runs = []
    for _ in range(2):
        kc, vc = ck.clone(), cv.clone()
        runs.append((X.run(MAIN, qkv, X.real_table(dev), kc, vc, lt, C - 129), kc, vc))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs))


def test_model_d128_extend(monkeypatch):
    """`prefill(chunk=24)` (24, 24, a ragged 17), and `extend` on a native prefill then a `decode_step`: `forward64`."""
    dev, fails = gpu_device(), []
    monkeypatch.setattr(A, "attention_extend_gqa_reference", _raise)
    torch.manual_seed(0)
    model = llama_tiny(hidden_size=256).eval().to(dev)
    cast_params(model, torch.bfloat16)
    prompts, forced = _tokens()
    S, first = max(LENS), [3, 40]
    comp, tail = torch.zeros(len(LENS), S, dtype=torch.long), torch.zeros(len(LENS), S - first[1], dtype=torch.long)
    for b, r in enumerate(prompts):
        comp[b, :len(r)], tail[b, :len(r) - first[b]] = r, r[first[b]:]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    cache = LlamaKVCache.allocate(model, len(LENS), S + 1)
    got = {"chunked prefill": (model.prefill(comp.to(dev), i32(LENS), cache, chunk=24), -2)}
    cache = LlamaKVCache.allocate(model, len(LENS), S + 1)
    model.prefill(comp[:, :first[1]].to(dev), i32(first), cache)
    got["extend"] = (model.extend(tail.to(dev), cache, i32([n - f for n, f in zip(LENS, first)])), -2)
    got["decode step"] = (model.decode_step(forced[:, 0].to(dev), cache), -1)
    assert cache.data.shape[-1] == D and cache.lens.tolist() == [n + 1 for n in LENS]
    with torch.no_grad():
        for b, r in enumerate(prompts):
            full = torch.cat([r, forced[b, :1]])
            ref, fwd = forward64(model, full), model(full[None].to(dev))[0].float().cpu()
            for name, (logits, row) in got.items():
                check(fails, f"row {b} {name}", logits[b].float().cpu(), ref[row], fwd[row])
    assert not fails, "\n".join(fails)
