"""Grouped-query chunk attention over a rotated KV cache with the chunk's rotation and the append (GPU only;
the rotary instances of csrc/kernels/attn_extend.hip), in the form of tests/test_attention_extend_gpu.py.

Every case has two batch rows of DIFFERENT cached lengths n (B = 2, C = 384).  (H, Hkv) = (4, 2) runs the full
lists; (1, 1), (3, 1), (4, 1) and (8, 1) -- the other group sizes with an instance -- run reduced ones.

Boundaries the kernel has.  Keys come in tiles of 64, the cache part first (tiles at 64 k, the last one cut by
n), then the chunk part (tiles at 64 k of the chunk, the last one cut by the diagonal); cache tiles arrive by
LDS-DMA, chunk K tiles through registers (rotated on the way), so a case with n = 0 has no DMA'd K tile and a
case with n > 0 has both kinds in turn.  A workgroup is G x NS waves, NS = 1 / 2 / 4 sixteen-query sub-tiles
for T <= 16 / <= 32 / more, capped at 4 (G <= 2), 2 (G = 3, 4), 1 (G = 8): the query tile is 16, 32 or 64 for
G <= 2 (T = 16 | 17 and 32 | 33 switch the instance, 64 | 65 and 128 | 129 add a query tile), 16 or 32 for G = 3, 4
(32 | 33, 64 | 65, 96 | 97 and 128 | 129 add a tile) and 16 for G = 8 (every 16: 48 | 49 is in the reduced list).  With
G = 3 a workgroup has 3 or 6 waves: the 8 DMA instructions of a tile and the 256 rotation pairs of a chunk K
tile do not divide evenly (the short last round).  Cached lengths {0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193,
255, 256, 257}; chunk lengths {1, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129}.  Every pair with max n + T <=
C runs, each with max_len = max n (tight) and max_len = C - T; (257, T = 127) is n + T = C, the last slot.

Reference: the chunk is rotated ONCE by the native ``ops.rope_qkv`` with table rows n .. n + T - 1 (the bits a
full forward sees); fp64 attention from those bf16 operands over the cache expanded to H heads.  The emulation
has fp32 scores and softmax, P rounded to bf16 and a bf16 output.  Tolerance: `check` of
tests/test_attention_edges_gpu.py with the project's M = 2, unchanged.  Every case prints its ratios.  Random
parity runs on the real rotary table; the routing and leak cases build their +-1 codes on the rotated side and
run with the identity table (cos = 1, sin = 0), under which the rotation returns its input bits.

Measured on an MI355X: 1195 comparisons in this file.  With the ulp term subtracted the largest ratios are 0.333
(max form; random, (4, 2), n = (128, 129), T = 31) and 0.088 (rms form; ragged, (3, 1), n = (65, 192), T = 65,
t = (64, 33)); as plain kernel error / emulation error the largest are 1.27 (max; that T = 31 case) and 1.05
(rms; last slot, (1, 1), T = 1).  So M = 2 holds as it stands.  The appended keys equal the native
``ops.rope_qkv``'s bits in every case (the compiler contracts the two kernels' rotation alike): no one-ulp
fallback is used.
"""
import math

import pytest
import torch

from conftest import gpu_device
from test_attention_edges_gpu import D, M, _split, check  # noqa: F401

from databricks_distributed_deep_learning_amd import ops

pytestmark = pytest.mark.gpu

B, C = 2, 384
NS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257]
TS = [1, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]
PAIRS = list(zip(NS, reversed(NS)))
TS_RED = [1, 15, 16, 17, 32, 33, 49, 64, 65, 97, 128, 129]
PAIRS_RED = [(0, 257), (65, 192), (128, 1), (255, 63)]
MAIN = (4, 2)
OTHERS = [(1, 1), (3, 1), (4, 1), (8, 1)]
SCALE = 1.0 / math.sqrt(D)


def _garbage(shape, dev, seed):
    """Arbitrary bf16 bit patterns, NaN and Inf among them."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-32768, 32767, shape, generator=g, dtype=torch.int16).to(dev).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16)


def _i32(v, dev):
    return torch.tensor(list(v), dtype=torch.int32, device=dev)


_TABLES = {}


def real_table(dev):
    if "real" not in _TABLES:
        _TABLES["real"] = ops.rope_table(C, 10000.0, D, dev)
    return _TABLES["real"]


def identity_table(dev):
    if "id" not in _TABLES:
        _TABLES["id"] = torch.cat([torch.ones(C, D // 2), torch.zeros(C, D // 2)], 1).to(dev)
    return _TABLES["id"]


def make_random(hh, ns, T, dev, seed):
    """qkv_new [B, T, (H + 2 Hkv) D], caches [B, Hkv, C, D] (live rows randn, the rest arbitrary bits), lens."""
    H, Hkv = hh
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, generator=g).bfloat16().to(dev)
    ck, cv = _garbage((B, Hkv, C, D), dev, seed + 1), _garbage((B, Hkv, C, D), dev, seed + 2)
    for b, n in enumerate(ns):
        ck[b, :, :n] = torch.randn(Hkv, n, D, generator=g).bfloat16().to(dev)
        cv[b, :, :n] = torch.randn(Hkv, n, D, generator=g).bfloat16().to(dev)
    return qkv, ck, cv, _i32(ns, dev)


def rotate(hh, qkv, table, ns):
    """The chunk rotated once by the native rope_qkv, row b with table rows n_b ..: packed [B, T, 3 H D]."""
    H, Hkv = hh
    T = qkv.shape[1]
    return torch.cat([ops.rope_qkv(qkv[b:b + 1].contiguous(), table[n:n + T].contiguous(), H, Hkv)
                      for b, n in enumerate(ns)])


def reference(hh, packed, ck, cv, ns, ts, dt, round_p=False):
    """out [B, T, H D] (rows >= t zeros) in dtype dt from the rotated packed chunk and, per batch row, the
    weights [H, t, n + t] over the keys cache 0 .. n-1, chunk 0 .. t-1.  round_p: P rounded to bf16 before P V."""
    H, Hkv = hh
    G = H // Hkv
    T = packed.shape[1]
    q, k, v = _split(packed.to(dt), H)
    out = torch.zeros(B, T, H * D, dtype=dt, device=packed.device)
    ps = []
    for b, (n, t) in enumerate(zip(ns, ts)):
        kk = torch.cat([ck[b, :, :n].to(dt).repeat_interleave(G, 0), k[b, :, :t]], 1)
        vv = torch.cat([cv[b, :, :n].to(dt).repeat_interleave(G, 0), v[b, :, :t]], 1)
        s = (q[b, :, :t] @ kk.transpose(-1, -2)) * SCALE
        i, j = torch.arange(t, device=packed.device), torch.arange(n + t, device=packed.device)
        p = torch.softmax(s.masked_fill(j[None, :] > n + i[:, None], -math.inf), -1)
        ps.append(p)
        if round_p:
            p = p.bfloat16().to(dt)
        out[b, :t] = (p @ vv).permute(1, 0, 2).reshape(t, H * D)
    return out, ps


def run(hh, qkv, table, ck, cv, lens, max_len, new_lens=None):
    out = ops.attention_extend_gqa(qkv, table, ck, cv, lens, hh[0], hh[1], max_len, new_lens)
    torch.cuda.synchronize()
    return out


def _check_case(fails, label, hh, qkv, table, ck, cv, ns, ts, max_len, ragged):
    dev = qkv.device
    packed = rotate(hh, qkv, table, ns)
    r64, _ = reference(hh, packed, ck, cv, ns, ts, torch.float64)
    em = reference(hh, packed, ck, cv, ns, ts, torch.float32, round_p=True)[0].bfloat16()
    out = run(hh, qkv, table, ck.clone(), cv.clone(), _i32(ns, dev), max_len, _i32(ts, dev) if ragged else None)
    assert torch.isfinite(out.float()).all(), label
    for b, t in enumerate(ts):
        assert (_bits(out[b, t:]) == 0).all(), label
    check(fails, label, out, r64, em)


def test_routes_to_the_kernel():
    from databricks_distributed_deep_learning_amd.ops import _native_attn_cache as N
    assert all(N.supported(*hh) for hh in [MAIN] + OTHERS) and not N.supported(5, 1) and not N.supported(6, 4)
    assert [N.tile(T, 4, 2) for T in (16, 17, 32, 33)] == [16, 32, 32, 64]
    assert [N.tile(T, 3, 1) for T in (16, 17, 33)] == [16, 32, 32] and N.tile(129, 8, 1) == 16


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
@pytest.mark.parametrize("T", TS)
def test_parity_random(T, tight):
    dev = gpu_device()
    fails = []
    for i, ns in enumerate(PAIRS):
        if max(ns) + T > C:
            continue
        qkv, ck, cv, _ = make_random(MAIN, ns, T, dev, 100 * T + i)
        _check_case(fails, f"random n={ns} T={T}", MAIN, qkv, real_table(dev), ck, cv, ns, (T, T),
                    max(ns) if tight else C - T, False)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("hh", OTHERS, ids=str)
@pytest.mark.parametrize("T", TS_RED)
def test_parity_random_other_groups(hh, T):
    dev = gpu_device()
    fails = []
    for i, ns in enumerate(PAIRS_RED):
        if max(ns) + T > C:
            continue
        qkv, ck, cv, _ = make_random(hh, ns, T, dev, 100 * T + i + hh[0])
        _check_case(fails, f"random {hh} n={ns} T={T}", hh, qkv, real_table(dev), ck, cv, ns, (T, T),
                    max(ns) if i % 2 else C - T, False)
        if T >= 2:
            ts = (T - 1, (T + 1) // 2)
            for b, t in enumerate(ts):
                qkv[b, t:] = _garbage((T - t, qkv.shape[2]), dev, T + b)
            _check_case(fails, f"ragged {hh} n={ns} T={T} t={ts}", hh, qkv, real_table(dev), ck, cv, ns, ts,
                        C - T if i % 2 else max(ns), True)
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
            qkv, ck, cv, _ = make_random(MAIN, ns, T, dev, 7 * T + i)
            for b, t in enumerate(ts):      # padded columns: arbitrary bits
                qkv[b, t:] = _garbage((T - t, qkv.shape[2]), dev, T + b)
            _check_case(fails, f"ragged n={ns} T={T} t={ts}", MAIN, qkv, real_table(dev), ck, cv, ns, ts,
                        max(ns) if tight else C - T, True)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("hh", [MAIN] + OTHERS, ids=str)
def test_last_slot(hh):
    """n + T = C exactly, in both rows, tight bound = C - T: the last cache row and the last table row."""
    dev = gpu_device()
    fails = []
    for T in (1, 17, 127):
        ns = (C - T, C - T)
        qkv, ck, cv, _ = make_random(hh, ns, T, dev, T)
        _check_case(fails, f"last slot {hh} T={T}", hh, qkv, real_table(dev), ck, cv, ns, (T, T), C - T, False)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ routing (identity table)
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


def make_routing(hh, ns, T, rnd, dev, seed, dead=None):
    """K = +-1 codes per KV head, q_i = 4 code[target_i] (each query head of a group has its own targets),
    V = randn: query i's whole weight sits on one key.  Returns the targets [B][H][T] too.  dead: None
    (arbitrary bits) | 'zeros' | 'decoys' (K = 2 x a target's code, V = 8) | 'nan'."""
    H, Hkv = hh
    G = H // Hkv
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.empty(B, T, H + 2 * Hkv, D)
    ck, cv = _garbage((B, Hkv, C, D), "cpu", seed + 1), _garbage((B, Hkv, C, D), "cpu", seed + 2)
    targets = [[None] * H for _ in range(B)]
    for b, n in enumerate(ns):
        for j in range(Hkv):
            code = torch.randint(0, 2, (n + T, D), generator=g).float() * 2 - 1
            val = torch.randn(n + T, D, generator=g)
            ck[b, j, :n], cv[b, j, :n] = code[:n].bfloat16(), val[:n].bfloat16()
            x[b, :, H + j], x[b, :, H + Hkv + j] = code[n:], val[n:]
            for h in range(j * G, (j + 1) * G):
                tg = []
                for i in range(T):
                    cand = candidates(n, i)
                    tg.append(cand[(i + rnd + h) % len(cand)])
                targets[b][h] = tg
                x[b, :, h] = 4.0 * code[tg]
            if dead == "zeros":
                ck[b, j, n:], cv[b, j, n:] = 0.0, 0.0
            elif dead == "decoys":
                ck[b, j, n:], cv[b, j, n:] = (2.0 * code[tg[-1]]).bfloat16(), 8.0
            elif dead == "nan":
                ck[b, j, n:], cv[b, j, n:] = math.nan, math.nan
    return x.reshape(B, T, (H + 2 * Hkv) * D).bfloat16().to(dev), ck.to(dev), cv.to(dev), targets


def _values(hh, qkv, cv, b, n):
    """[H, n + T, D]: the values behind the key indices of batch row b."""
    H, Hkv = hh
    T = qkv.shape[1]
    v = qkv.view(B, T, H + 2 * Hkv, D)[b, :, H + Hkv:].permute(1, 0, 2)        # [Hkv, T, D]
    return torch.cat([cv[b, :, :n], v], 1).float().repeat_interleave(H // Hkv, 0)


@pytest.mark.parametrize("hh,ns,T", [(MAIN, (129, 64), 65), (MAIN, (257, 0), 127), (MAIN, (1, 65), 17),
                                     (MAIN, (63, 128), 16), (MAIN, (192, 5), 129), ((3, 1), (65, 128), 33),
                                     ((8, 1), (64, 1), 65), ((1, 1), (0, 129), 64), ((4, 1), (127, 2), 97)], ids=str)
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
def test_routing(hh, ns, T, tight):
    dev = gpu_device()
    H = hh[0]
    fails = []
    table = identity_table(dev)
    rounds = max(len(candidates(n, T - 1)) for n in ns)
    for rnd in range(rounds):
        qkv, ck, cv, targets = make_routing(hh, ns, T, rnd, dev, 31 * rnd + sum(ns) + T)
        packed = rotate(hh, qkv, table, ns)
        if rnd == 0:        # the identity table returns the input bits
            x = qkv.view(B, T, -1, D)
            assert torch.equal(_bits(_split(packed, H)[0]), _bits(x[:, :, :H].permute(0, 2, 1, 3)))
        r64, ps = reference(hh, packed, ck, cv, ns, (T, T), torch.float64)
        em = reference(hh, packed, ck, cv, ns, (T, T), torch.float32, round_p=True)[0].bfloat16()
        out = run(hh, qkv, table, ck.clone(), cv.clone(), _i32(ns, dev), max(ns) if tight else C - T)
        for b, n in enumerate(ns):
            vv = _values(hh, qkv, cv, b, n)
            for h in range(H):
                tg = torch.tensor(targets[b][h], device=dev)
                w = ps[b][h, torch.arange(T, device=dev), tg]
                assert w.min().item() >= 0.999, (ns, T, rnd, b, h, w.min().item())
                got = out[b, :, h * D:(h + 1) * D].float()
                torch.testing.assert_close(got, vv[h, tg], rtol=2.0 ** -7, atol=0.03)
        check(fails, f"routing {hh} n={ns} T={T} round={rnd}", out, r64, em)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ leaks
@pytest.mark.parametrize("hh,ns,T", [(MAIN, (255, 63), 65), (MAIN, (128, 7), 16), ((3, 1), (0, 193), 127)], ids=str)
def test_dead_tail_cannot_reach_the_output(hh, ns, T):
    dev = gpu_device()
    outs = []
    for dead in ("zeros", "decoys", "nan"):
        qkv, ck, cv, _ = make_routing(hh, ns, T, 1, dev, 5, dead)
        outs.append(run(hh, qkv, identity_table(dev), ck, cv, _i32(ns, dev), C - T))
        assert torch.isfinite(outs[-1].float()).all()
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))


@pytest.mark.parametrize("hh,ns,T", [(MAIN, (129, 0), 66), (MAIN, (64, 5), 17), ((8, 1), (1, 200), 130)], ids=str)
def test_next_chunk_key_cannot_move_a_query(hh, ns, T):
    """A decoy at chunk key i + 1 (K = 2 x the target code of query i of the group's first head: it would win;
    V = 8) leaves rows 0 .. i bitwise as they were; the reference weight on the target is >= 0.999."""
    dev = gpu_device()
    H, Hkv = hh
    G = H // Hkv
    table = identity_table(dev)
    qkv, ck, cv, targets = make_routing(hh, ns, T, 0, dev, 11)
    _, ps = reference(hh, rotate(hh, qkv, table, ns), ck, cv, ns, (T, T), torch.float64)
    base = run(hh, qkv, table, ck.clone(), cv.clone(), _i32(ns, dev), max(ns))
    for i in sorted({0, 14, 15, 16, 30, 31, 32, 62, 63, 64, 126, 127, 128, T - 2} & set(range(T - 1))):
        x = qkv.clone().view(B, T, H + 2 * Hkv, D)
        for b in range(B):
            for j in range(Hkv):
                assert ps[b][j * G, i, targets[b][j * G][i]].item() >= 0.999
                x[b, i + 1, H + j] = 0.5 * x[b, i, j * G]          # q_i = 4 code[target]: 2 x the code
                x[b, i + 1, H + Hkv + j] = 8.0
        out = run(hh, x.view(B, T, -1), table, ck.clone(), cv.clone(), _i32(ns, dev), max(ns))
        assert torch.equal(_bits(out[:, :i + 1]), _bits(base[:, :i + 1])), i


@pytest.mark.parametrize("ns,T,ts", [((129, 0), 66, (64, 1)), ((64, 5), 17, (16, 15)), ((1, 200), 130, (65, 129))], ids=str)
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
def test_padded_columns_cannot_move_a_valid_query(ns, T, ts, tight):
    """Chunk rows i >= t as zeros, as decoys (K = 2 x the last valid query's target code, V = 8, q = the same) and
    as NaN: the outputs and the caches are bitwise equal."""
    dev = gpu_device()
    H, Hkv = MAIN
    G = H // Hkv
    res = []
    for mode in ("zeros", "decoys", "nan"):
        qkv, ck, cv, _ = make_routing(MAIN, ns, T, 2, dev, 13)
        x = qkv.view(B, T, H + 2 * Hkv, D)
        for b, t in enumerate(ts):
            if mode == "zeros":
                x[b, t:] = 0.0
            elif mode == "nan":
                x[b, t:] = math.nan
            else:
                x[b, t:, :H] = x[b, t - 1, :H]
                x[b, t:, H:H + Hkv] = 0.5 * x[b, t - 1, 0:H:G]
                x[b, t:, H + Hkv:] = 8.0
        out = run(MAIN, qkv, identity_table(dev), ck, cv, _i32(ns, dev), max(ns) if tight else C - T, _i32(ts, dev))
        assert torch.isfinite(out.float()).all()
        res.append((out, ck, cv))
    for other in res[1:]:
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(res[0], other))


@pytest.mark.parametrize("ns,T", [((129, 64), 65), ((0, 200), 17), ((255, 3), 129)], ids=str)
def test_other_kv_heads_cannot_reach_a_group(ns, T):
    """(H, Hkv) = (4, 2): with KV head j' != j -- its cache rows, chunk keys and chunk values -- as zeros, as
    decoys (K = 2 x the target code of a query of group j, V = 8) and as NaN, the outputs of group j's query
    heads are bitwise equal, and they are the routed values."""
    dev = gpu_device()
    H, Hkv = MAIN
    G = H // Hkv
    table = identity_table(dev)
    for j in range(Hkv):
        o = 1 - j
        outs = []
        for mode in ("zeros", "decoys", "nan"):
            qkv, ck, cv, targets = make_routing(MAIN, ns, T, 3, dev, 19)
            x = qkv.view(B, T, H + 2 * Hkv, D)
            for b, n in enumerate(ns):
                if mode == "zeros":
                    ck[b, o], cv[b, o], x[b, :, H + o], x[b, :, H + Hkv + o] = 0.0, 0.0, 0.0, 0.0
                elif mode == "nan":
                    ck[b, o], cv[b, o], x[b, :, H + o], x[b, :, H + Hkv + o] = math.nan, math.nan, math.nan, math.nan
                else:       # every key of the other head is the code the group's queries look for, doubled
                    ck[b, o, :n] = 0.5 * x[b, 0, j * G]
                    x[b, :, H + o] = 0.5 * x[b, :, j * G]
                    cv[b, o], x[b, :, H + Hkv + o] = 8.0, 8.0
            out = run(MAIN, qkv, table, ck, cv, _i32(ns, dev), C - T)
            mine = out.view(B, T, H, D)[:, :, j * G:(j + 1) * G]
            assert torch.isfinite(mine.float()).all()
            outs.append(mine.clone())
        assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))
        for b, n in enumerate(ns):
            vv = _values(MAIN, qkv, cv, b, n)
            for h in range(j * G, (j + 1) * G):
                tg = torch.tensor(targets[b][h], device=dev)
                torch.testing.assert_close(outs[0][b, :, h - j * G].float(), vv[h, tg], rtol=2.0 ** -7, atol=0.03)


# ------------------------------------------------------------------ append, repeatability
@pytest.mark.parametrize("hh,ns,T,ts", [(MAIN, (257, 0), 127, None), (MAIN, (64, 63), 65, (1, 65)),
                                        (MAIN, (5, 128), 16, (15, 2)), (MAIN, (383, 320), 1, None),
                                        (MAIN, (0, 191), 129, (128, 129)), ((3, 1), (100, 7), 33, (33, 17)),
                                        ((8, 1), (1, 64), 49, None), ((1, 1), (63, 0), 65, (64, 65))], ids=str)
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
def test_append(hh, ns, T, ts, tight):
    """cache[b, j, n_b + i] becomes chunk row i's rotated K -- the bits of the native ``ops.rope_qkv`` at table
    row n_b + i -- and its V (a bit copy) for i < t_b; nothing else changes (n + T = C, the last slot, included);
    lens and new_lens are not written."""
    dev = gpu_device()
    H, Hkv = hh
    G = H // Hkv
    qkv, ck, cv, lt = make_random(hh, ns, T, dev, 17)
    wk, wv = ck.clone(), cv.clone()
    _, k, v = _split(rotate(hh, qkv, real_table(dev), ns), H)
    tt = ts or (T, T)
    for b, (n, t) in enumerate(zip(ns, tt)):
        wk[b, :, n:n + t], wv[b, :, n:n + t] = k[b, ::G, :t], v[b, ::G, :t]
    assert torch.equal(_bits(v[:, ::G]), _bits(qkv.view(B, T, -1, D)[:, :, H + Hkv:].permute(0, 2, 1, 3)))
    nl = None if ts is None else _i32(ts, dev)
    run(hh, qkv, real_table(dev), ck, cv, lt, max(ns) if tight else C - T, nl)
    assert torch.equal(_bits(ck), _bits(wk)) and torch.equal(_bits(cv), _bits(wv))
    assert lt.tolist() == list(ns) and (nl is None or nl.tolist() == list(ts))


def test_repeatable():
    dev = gpu_device()
    for hh, ns, T in ((MAIN, (250, 3), 129), (MAIN, (100, 64), 16), ((3, 1), (70, 200), 65)):
        qkv, ck, cv, lt = make_random(hh, ns, T, dev, 23)
        runs = []
        for _ in range(3):
            k, v = ck.clone(), cv.clone()
            runs.append((run(hh, qkv, real_table(dev), k, v, lt, C - T), k, v))
        for other in runs[1:]:
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(runs[0], other))


# ------------------------------------------------------------------ prefill + extend + decode chain
def _causal(packed, H, dt, round_p=False):
    q, k, v = _split(packed.to(dt), H)
    S = packed.shape[1]
    s = (q @ k.transpose(-1, -2)) * SCALE
    ar = torch.arange(S, device=packed.device)
    p = torch.softmax(s.masked_fill(ar[None, :] > ar[:, None], -math.inf), -1)
    if round_p:
        p = p.bfloat16().to(dt)
    return (p @ v).permute(0, 2, 1, 3).reshape(packed.shape[0], S, H * D)


@pytest.mark.parametrize("hh", [MAIN, (3, 1)], ids=str)
def test_prefill_extend_decode_chain(hh):
    """Native rope_qkv + causal attention + kv_cache_fill_gqa on 65 tokens, extends of T = 1, 16 and 65, one
    attention_decode_gqa: each result is its row range of one causal attention over all 148 tokens, and the
    cache equals the rotated K / V of the whole sequence bitwise."""
    from databricks_distributed_deep_learning_amd.ops import _native_attention as NA
    dev = gpu_device()
    H, Hkv = hh
    G = H // Hkv
    table = real_table(dev)
    S0, chunks = 65, (1, 16, 65)
    S = S0 + sum(chunks) + 1
    proj = torch.randn(B, S, (H + 2 * Hkv) * D, device=dev).bfloat16()
    packed = ops.rope_qkv(proj, table, H, Hkv)
    r64, em = _causal(packed, H, torch.float64), _causal(packed, H, torch.float32, True).bfloat16()
    ck, cv = _garbage((B, Hkv, C, D), dev, 1), _garbage((B, Hkv, C, D), dev, 2)
    pre = ops.rope_qkv(proj[:, :S0].contiguous(), table, H, Hkv)
    fails = []
    check(fails, "chain prefill", NA.attention(pre, H, None, 0.0, causal=True), r64[:, :S0], em[:, :S0])
    ops.kv_cache_fill_gqa(pre, ck, cv, H, Hkv)
    lens, at = torch.full((B,), S0, dtype=torch.int32, device=dev), S0
    for T in chunks:
        out = run(hh, proj[:, at:at + T].contiguous(), table, ck, cv, lens, at)
        check(fails, f"chain extend T={T}", out, r64[:, at:at + T], em[:, at:at + T])
        lens += T
        at += T
    out = ops.attention_decode_gqa(proj[:, at].contiguous(), table, ck, cv, lens, H, Hkv, at + 1)
    check(fails, "chain decode", out, r64[:, at], em[:, at])
    _, k, v = _split(packed, H)
    assert torch.equal(_bits(ck[:, :, :S]), _bits(k[:, ::G])) and torch.equal(_bits(cv[:, :, :S]), _bits(v[:, ::G]))
    assert not fails, "\n".join(fails)


def test_guards_are_on_the_host():
    dev = gpu_device()
    qkv, ck, cv, lt = make_random(MAIN, (3, 4), 5, dev, 1)
    with pytest.raises(ValueError, match="capacity"):
        ops.attention_extend_gqa(qkv, real_table(dev), ck, cv, lt, 4, 2, C - 4)
    with pytest.raises(ValueError, match="rotary table"):
        ops.attention_extend_gqa(qkv, real_table(dev)[:8], ck, cv, lt, 4, 2, 4)
    with pytest.raises(RuntimeError, match="autograd"):
        ops.attention_extend_gqa(qkv.clone().requires_grad_(True), real_table(dev), ck, cv, lt, 4, 2, 4)
