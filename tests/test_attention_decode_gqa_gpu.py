"""Grouped-query single-query attention over a rotated KV cache, with the new token's rotation and the append,
and its cache fill (GPU only; the rotary instances of csrc/kernels/attn_decode.hip).

Every case has two batch rows of DIFFERENT lengths (B = 2, H = 4, Hkv = 2, C = 1024 unless said otherwise).
Live cache rows are randn, the rest arbitrary bf16 bit patterns, NaN / Inf among them.

Boundaries the kernel has.  A workgroup is 32 key groups of 8 lanes and takes 4 keys per group per round (2
at G = 8): key j of a split sits in unroll slot (j / 32) % 4, so 32 is the slot edge and 128 (64) the round
edge.  Splits: nsplit = min(32, ceil(CUs / (B Hkv)), ceil(max_len / 64)) and chunk = ceil(max_len / nsplit)
rounded up to 32; at B Hkv = 4 (and 2, the G = 8 case) on 256 CUs that is chunk = 64 for every max_len <= 1024
(nsplit = 1 for max_len <= 64, 16 at max_len = 1024), so the split edges are the multiples of 64 up to 960.
Lengths: the issue's {0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1022, 1023} plus +-1
around every split edge 64 k, k = 1 .. 15; each length runs with max_len = the tight bound (max n + 1) and with
max_len = C (trailing splits empty).  Two more geometries cover what B Hkv = 4 cannot: B Hkv = 128 (nsplit = 2,
chunk = 512: four rounds per split) and B Hkv = 256 (nsplit = 1, chunk = max_len: the direct-output path with
eight rounds).

Tolerance: `check` of tests/test_attention_edges_gpu.py at its M = 2, the emulation being fp32 throughout
with a bf16 output; reference fp64 from the bf16 operands.  The rotated bf16 q / k of both come from a
plain-torch fp32 rotation rounded once.  Every case prints its ratios.

Measured on an MI355X: 202 comparisons in this file.  Of the 200 that run the decode kernel, with the ulp
term subtracted the largest ratios are -0.000 (max form; random inputs, n = (7, 961)) and -0.239 (rms form;
n = (831, 65)): the kernel never exceeds the fp32 emulation's error by more than half a bf16 ulp.  As plain
kernel error / emulation error the largest is 1.00 (max and rms; random, routing and the three chain steps
alike).  The chain's other two comparisons run the existing causal kernel (1.01 max, 1.18 rms as plain ratios).
So M = 2 holds as it stands.  The appended key rows equal native ``ops.rope_qkv``'s bitwise: the fallback to a
one-ulp comparison against an fp64 rotation was not needed.
"""
import math

import pytest
import torch

from conftest import gpu_device
from test_attention_edges_gpu import D, M, check  # noqa: F401

from databricks_distributed_deep_learning_amd import ops

pytestmark = pytest.mark.gpu

B, H, HKV, C = 2, 4, 2, 1024
EDGES = [64 * k for k in range(1, 16)]
LENGTHS = sorted({0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1022, 1023}
                 | {e + d for e in EDGES for d in (-1, 0, 1)})
PAIRS = list(zip(LENGTHS, reversed(LENGTHS)))       # (an odd count: the middle length pairs with itself ...)
PAIRS[len(LENGTHS) // 2] = (LENGTHS[len(LENGTHS) // 2], 5)      # ... so it gets another partner)
SCALE = 1.0 / math.sqrt(D)
_TABLES = {}


def table(dev, kind="real"):
    """fp32 [C, 64]: the real rotary table, the identity (cos 1, sin 0) or the swap (cos 0, sin 1)."""
    if (kind, dev) not in _TABLES:
        if kind == "real":
            t = ops.rope_table(C, 10000.0, D, dev)
        else:
            one, zero = torch.ones(C, D // 2, device=dev), torch.zeros(C, D // 2, device=dev)
            t = torch.cat([one, zero] if kind == "identity" else [zero, one], 1).contiguous()
        _TABLES[(kind, dev)] = t
    return _TABLES[(kind, dev)]


def _garbage(shape, dev, seed):
    """Arbitrary bf16 bit patterns, NaN and Inf among them."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-32768, 32767, shape, generator=g, dtype=torch.int16).to(dev).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16)


def make_random(lens, dev, seed, b=B, h=H, hkv=HKV, c=C):
    """qkv_new [b, (h + 2 hkv) D], caches [b, hkv, c, D] (live rows randn, the rest arbitrary bits), lens."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(b, (h + 2 * hkv) * D, generator=g).bfloat16().to(dev)
    ck, cv = _garbage((b, hkv, c, D), dev, seed + 1), _garbage((b, hkv, c, D), dev, seed + 2)
    for i, n in enumerate(lens):
        ck[i, :, :n] = torch.randn(hkv, n, D, generator=g).bfloat16().to(dev)
        cv[i, :, :n] = torch.randn(hkv, n, D, generator=g).bfloat16().to(dev)
    return qkv, ck, cv, torch.tensor(lens, dtype=torch.int32, device=dev)


def rotate_once(qkv, tab, lens, h, hkv):
    """The bf16 operands: q [b, h, D] and k [b, hkv, D] rotated by table row lens[b] in fp32 and rounded once;
    v [b, hkv, D] as it is."""
    b = qkv.shape[0]
    x = qkv.float().view(b, h + 2 * hkv, D)
    row = tab[lens.long()].float()
    cos, sin = row[:, None, :D // 2], row[:, None, D // 2:]
    x1, x2 = x[:, :h + hkv, :D // 2], x[:, :h + hkv, D // 2:]
    r = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], -1).bfloat16()
    return r[:, :h], r[:, h:], qkv.view(b, h + 2 * hkv, D)[:, h + hkv:]


def reference(qkv, tab, ck, cv, lens, h, hkv, dt):
    """out [b, h D] in dtype dt and the attention weights [b, h, L]: keys 0 .. n-1 from the cache, key n the
    new one."""
    b, G = qkv.shape[0], h // hkv
    L = int(lens.max()) + 1
    q, k, v = (t.to(dt) for t in rotate_once(qkv, tab, lens, h, hkv))
    kk, vv = ck[:, :, :L].to(dt).clone(), cv[:, :, :L].to(dt).clone()
    bi, n = torch.arange(b, device=qkv.device), lens.long()
    kk[bi, :, n], vv[bi, :, n] = k, v
    live = torch.arange(L, device=qkv.device).view(1, 1, 1, L) <= n.view(b, 1, 1, 1)
    s = (q.view(b, hkv, G, D) @ kk.transpose(-1, -2)) * SCALE                      # [b, hkv, G, L]
    p = torch.softmax(torch.where(live, s, torch.full_like(s, -math.inf)), -1)
    vv = torch.where(live.view(b, 1, L, 1), vv, torch.zeros_like(vv))
    return (p @ vv).reshape(b, h * D), p.reshape(b, h, L)


def run(qkv, tab, ck, cv, lens, max_len, h=H, hkv=HKV):
    out = ops.attention_decode_gqa(qkv, tab, ck, cv, lens, h, hkv, max_len)
    torch.cuda.synchronize()
    return out


def _check_case(fails, label, qkv, tab, ck, cv, lens, max_len, h=H, hkv=HKV):
    r64, _ = reference(qkv, tab, ck, cv, lens, h, hkv, torch.float64)
    em = reference(qkv, tab, ck, cv, lens, h, hkv, torch.float32)[0].bfloat16()
    out = run(qkv, tab, ck.clone(), cv.clone(), lens, max_len, h, hkv)
    assert torch.isfinite(out.float()).all(), label
    check(fails, label, out, r64, em)


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
def test_parity_random(tight):
    dev = gpu_device()
    fails = []
    for i, lens in enumerate(PAIRS):
        qkv, ck, cv, lt = make_random(lens, dev, 100 + i)
        _check_case(fails, f"random n={lens}", qkv, table(dev), ck, cv, lt, max(lens) + 1 if tight else C)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("G,hkv", [(1, 2), (3, 2), (4, 2), (8, 1)], ids=["G1", "G3", "G4", "G8"])
def test_parity_group_sizes(G, hkv):
    dev = gpu_device()
    fails = []
    qkv, ck, cv, lt = make_random((1023, 65), dev, 40 + G, B, G * hkv, hkv)
    _check_case(fails, f"random G={G} Hkv={hkv}", qkv, table(dev), ck, cv, lt, C, G * hkv, hkv)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("b,hkv,want", [(8, 16, 2), (16, 16, 1)], ids=["bhkv128-2splits", "bhkv256-1split"])
def test_parity_other_geometries(b, hkv, want):
    """Long splits (several rounds each) and the direct-output path at a long length."""
    from databricks_distributed_deep_learning_amd.ops import _native_attn_cache as ND
    dev = gpu_device()
    h = 2 * hkv
    lens = [(LENGTHS[(3 * i + 1) % len(LENGTHS)]) for i in range(b)]
    lens[0], lens[-1] = 1023, 0
    nsplit, chunk = ND.plan_gqa(b, hkv, C)
    print(f"plan B Hkv = {b * hkv}: nsplit {nsplit} chunk {chunk}")
    assert nsplit == want
    fails = []
    qkv, ck, cv, lt = make_random(lens, dev, 7, b, h, hkv)
    _check_case(fails, f"random B={b} H={h} Hkv={hkv}", qkv, table(dev), ck, cv, lt, C, h, hkv)
    assert not fails, "\n".join(fails)


def test_plan_is_what_the_docstring_says():
    from databricks_distributed_deep_learning_amd.ops import _native_attn_cache as ND
    gpu_device()
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        return      # the listed split edges are those of a 256-CU part
    assert ND.plan_gqa(B, HKV, 1024) == (16, 64) and ND.plan_gqa(B, HKV, 64) == (1, 64) and ND.plan_gqa(B, HKV, 65) == (2, 64)
    assert ND.plan_gqa(B, HKV, 514) == (9, 64) and ND.plan_gqa(B, 1, 1024) == (16, 64)
    assert ND.plan_gqa(8, 16, 1024) == (2, 512) and ND.plan_gqa(16, 16, 1024) == (1, 1024)
    assert ND.plan_gqa(1, 3, 2048) == (32, 64) and ND.plan_gqa(16, 3, 1024) == (6, 192)
    for g in (1, 2, 3, 4, 8):
        assert ND.supported(8 * g, 8)
    assert not ND.supported(5, 1) and not ND.supported(12, 2) and not ND.supported(4, 3)


def test_single_key_is_the_value_row_bitwise():
    """n = 0: a softmax over one key is exactly 1."""
    dev = gpu_device()
    for max_len in (6, C):
        qkv, ck, cv, lt = make_random([0, 5], dev, 3)
        out = run(qkv, table(dev), ck, cv, lt, max_len)
        v = qkv.view(B, H + 2 * HKV, D)[0, H + HKV:]
        assert torch.equal(_bits(out[0].view(HKV, H // HKV, D)), _bits(v[:, None].expand(HKV, H // HKV, D)))


def test_unsupported_group_takes_the_reference():
    """G = 5 has no kernel instance: the op computes it in plain torch, to the same bound."""
    dev = gpu_device()
    fails = []
    qkv, ck, cv, lt = make_random((200, 33), dev, 9, B, 5, 1)
    _check_case(fails, "random G=5", qkv, table(dev), ck, cv, lt, 201, 5, 1)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ routing
def make_routing(lens, targets, dev, seed, dead=None, h=H, hkv=HKV):
    """Per KV head K = +-1 codes (its own), V = randn; query head j of the group aims at key targets[b][j]:
    q = 4 code[target], so the whole weight sits on one key, a different one per query head.
    dead: None (tail = arbitrary bits) | 'zeros' | 'decoys' (K = 2 x a target's code, V = 8) | 'nan'."""
    G = h // hkv
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.empty(B, h + 2 * hkv, D)
    ck, cv = _garbage((B, hkv, C, D), "cpu", seed + 1), _garbage((B, hkv, C, D), "cpu", seed + 2)
    for b, n in enumerate(lens):
        for j in range(hkv):
            code = torch.randint(0, 2, (n + 1, D), generator=g).float() * 2 - 1
            val = torch.randn(n + 1, D, generator=g)
            ck[b, j, :n], cv[b, j, :n] = code[:n].bfloat16(), val[:n].bfloat16()
            for i in range(G):
                qkv[b, j * G + i] = 4.0 * code[targets[b][j * G + i]]
            qkv[b, h + j], qkv[b, h + hkv + j] = code[n], val[n]
            t = targets[b][j * G]
            if dead == "zeros":
                ck[b, j, n:], cv[b, j, n:] = 0.0, 0.0
            elif dead == "decoys":
                ck[b, j, n:], cv[b, j, n:] = (2.0 * code[t]).bfloat16(), 8.0
            elif dead == "nan":
                ck[b, j, n:], cv[b, j, n:] = math.nan, math.nan
    return (qkv.reshape(B, (h + 2 * hkv) * D).bfloat16().to(dev), ck.to(dev), cv.to(dev),
            torch.tensor(lens, dtype=torch.int32, device=dev))


def target_cycle(n):
    """Position 0, the last cached key, the new key, and the first and last key of every 32-key slot
    (which includes every split and round edge)."""
    t = [0, max(n - 1, 0), n]
    for e in range(32, n + 1, 32):
        t += [e - 1, e]
    return t


@pytest.mark.parametrize("lens", [(1023, 257), (129, 64), (65, 1), (960, 513), (0, 33)], ids=str)
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
def test_routing(lens, tight):
    """Identity table (the rotation is exact).  The query heads of one group aim at different keys and the KV
    heads hold different codes: a wrong h / G mapping or a softmax state shared within a group fails."""
    dev = gpu_device()
    tab = table(dev, "identity")
    cyc = [target_cycle(n) for n in lens]
    fails = []
    for i in range(-(-max(len(c) for c in cyc) // H)):
        targets = [[cyc[b][(i * H + h) % len(cyc[b])] for h in range(H)] for b in range(B)]
        qkv, ck, cv, lt = make_routing(lens, targets, dev, 31 * i + sum(lens))
        r64, p = reference(qkv, tab, ck, cv, lt, H, HKV, torch.float64)
        for b in range(B):
            for h in range(H):
                assert p[b, h, targets[b][h]].item() >= 0.999
        em = reference(qkv, tab, ck, cv, lt, H, HKV, torch.float32)[0].bfloat16()
        out = run(qkv, tab, ck, cv, lt, max(lens) + 1 if tight else C)
        check(fails, f"routing n={lens} targets={targets}", out, r64, em)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("lens", [(1022, 63), (128, 7), (0, 960)], ids=str)
def test_dead_tail_cannot_reach_the_output(lens):
    dev = gpu_device()
    targets = [[0, n, max(n - 1, 0), n] for n in lens]
    outs = []
    for dead in ("zeros", "decoys", "nan"):
        qkv, ck, cv, lt = make_routing(lens, targets, dev, 5, dead)
        outs.append(run(qkv, table(dev, "identity"), ck, cv, lt, C))
        assert torch.isfinite(outs[-1].float()).all()
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))


# ------------------------------------------------------------------ rotation
def test_swap_table_appends_the_swapped_key():
    """cos = 0, sin = 1: the rotated key is [-k[32:], k[:32]], exactly."""
    dev = gpu_device()
    qkv, ck, cv, lt = make_random((5, 700), dev, 51)
    run(qkv, table(dev, "swap"), ck, cv, lt, C)
    k = qkv.view(B, H + 2 * HKV, D)[:, H:H + HKV]
    want = torch.cat([-k[..., 32:], k[..., :32]], -1)
    for b, n in enumerate((5, 700)):
        assert torch.equal(_bits(ck[b, :, n]), _bits(want[b]))


def test_appended_key_is_rope_qkv_bitwise():
    """Real table: the appended key rows are the k slot native ``ops.rope_qkv`` writes for the same projection
    row at the same position; the value row is a bit copy."""
    dev = gpu_device()
    tab = table(dev)
    lens = (5, 700)
    qkv, ck, cv, lt = make_random(lens, dev, 52)
    run(qkv, tab, ck, cv, lt, C)
    k = native_rotated_k(qkv, tab, lens)
    for b, n in enumerate(lens):
        assert torch.equal(_bits(ck[b, :, n]), _bits(k[b]))
        assert torch.equal(_bits(cv[b, :, n]), _bits(qkv.view(B, H + 2 * HKV, D)[b, H + HKV:]))


def test_rows_with_equal_projections_rotate_by_their_own_lens():
    dev = gpu_device()
    qkv, ck, cv, lt = make_random((300, 300), dev, 53)
    qkv[1], ck[1], cv[1] = qkv[0], ck[0], cv[0]
    same = run(qkv, table(dev), ck.clone(), cv.clone(), lt, C)
    assert torch.equal(_bits(same[0]), _bits(same[1]))
    lt2 = torch.tensor([300, 299], dtype=torch.int32, device=dev)
    ck[1, :, 299], cv[1, :, 299] = ck[0, :, 300], cv[0, :, 300]     # (row 1's slot 299 gets overwritten)
    out = run(qkv, table(dev), ck, cv, lt2, C)
    assert not torch.equal(_bits(out[0]), _bits(out[1]))
    assert not torch.equal(_bits(ck[0, :, 300]), _bits(ck[1, :, 299]))
    assert torch.equal(_bits(cv[0, :, 300]), _bits(cv[1, :, 299]))


# ------------------------------------------------------------------ append, repeatability
def native_rotated_k(qkv, tab, lens, h=H, hkv=HKV):
    """[b, hkv, D]: the k slots native ``ops.rope_qkv`` writes for each row at position lens[b]."""
    rows = []
    for b, n in enumerate(lens):
        packed = ops.rope_qkv(qkv[b].view(1, 1, -1).contiguous(), tab[n:n + 1].contiguous(), h, hkv).view(3, h, D)
        rows.append(packed[1, ::h // hkv])
    return torch.stack(rows)


@pytest.mark.parametrize("lens", [(1023, 0), (64, 63), (511, 1022), (5, 128)], ids=str)
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
def test_append(lens, tight):
    """cache[b, :, n_b] becomes the rotated key (rope_qkv's bits) / the value row; nothing else changes
    (n = C - 1, the last slot, included); lens is unchanged."""
    dev = gpu_device()
    qkv, ck, cv, lt = make_random(lens, dev, 17)
    wk, wv = ck.clone(), cv.clone()
    k = native_rotated_k(qkv, table(dev), lens)
    v = qkv.view(B, H + 2 * HKV, D)[:, H + HKV:]
    for b, n in enumerate(lens):
        wk[b, :, n], wv[b, :, n] = k[b], v[b]
    run(qkv, table(dev), ck, cv, lt, max(lens) + 1 if tight else C)
    assert torch.equal(_bits(ck), _bits(wk)) and torch.equal(_bits(cv), _bits(wv))
    assert lt.tolist() == list(lens)


def test_repeatable():
    from databricks_distributed_deep_learning_amd.ops import _native_attn_cache as ND
    dev = gpu_device()
    assert ND.plan_gqa(B, HKV, C)[0] > 1
    qkv, ck, cv, lt = make_random([1000, 700], dev, 23)
    a = run(qkv, table(dev), ck.clone(), cv.clone(), lt, C)
    b = run(qkv, table(dev), ck.clone(), cv.clone(), lt, C)
    assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ cache fill
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 129])
def test_kv_cache_fill_gqa(S, G):
    dev = gpu_device()
    cap, h = 160, HKV * G
    packed = torch.randn(B, S, 3 * h * D, device=dev).bfloat16()
    ck, cv = _garbage((B, HKV, cap, D), dev, 1), _garbage((B, HKV, cap, D), dev, 2)
    wk, wv = ck.clone(), cv.clone()
    p5 = packed.view(B, S, 3, h, D)
    for j in range(HKV):
        wk[:, j, :S], wv[:, j, :S] = p5[:, :, 1, j * G], p5[:, :, 2, j * G]
    ops.kv_cache_fill_gqa(packed, ck, cv, h, HKV)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ck), _bits(wk)) and torch.equal(_bits(cv), _bits(wv))


# ------------------------------------------------------------------ prefill + decode chain
def _causal(packed, h, dt):
    b, S, _ = packed.shape
    q, k, v = packed.to(dt).view(b, S, 3, h, D).permute(2, 0, 3, 1, 4).unbind(0)
    s = (q @ k.transpose(-1, -2)) * SCALE
    ar = torch.arange(S, device=packed.device)
    s = s.masked_fill(ar[None, :] > ar[:, None], -math.inf)
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(b, S, h * D)


def test_prefill_then_decode_chain():
    """Native rope_qkv + causal attention over all 68 tokens, and a prefill of 65 + fill + 3 decode steps
    (step i is row 65 + i of the same attention): both against the fp64 causal reference."""
    from databricks_distributed_deep_learning_amd.ops import _native_attention as NA
    dev = gpu_device()
    tab = table(dev)
    S0, steps = 65, 3
    proj = torch.randn(B, S0 + steps, (H + 2 * HKV) * D, device=dev).bfloat16()
    packed = ops.rope_qkv(proj, tab, H, HKV)
    r64, em = _causal(packed, H, torch.float64), _causal(packed, H, torch.float32).bfloat16()
    ck, cv = _garbage((B, HKV, C, D), dev, 1), _garbage((B, HKV, C, D), dev, 2)
    fails = []
    check(fails, "chain full", NA.attention(packed, H, None, 0.0, causal=True), r64, em)
    pre = ops.rope_qkv(proj[:, :S0].contiguous(), tab, H, HKV)
    check(fails, "chain prefill", NA.attention(pre, H, None, 0.0, causal=True), r64[:, :S0], em[:, :S0])
    ops.kv_cache_fill_gqa(pre, ck, cv, H, HKV)
    lens = torch.full((B,), S0, dtype=torch.int32, device=dev)
    for i in range(steps):
        t = S0 + i
        out = run(proj[:, t].contiguous(), tab, ck, cv, lens, t + 1)
        check(fails, f"chain step {i}", out, r64[:, t], em[:, t])
        lens += 1
    assert not fails, "\n".join(fails)


def test_guards_are_on_the_host():
    dev = gpu_device()
    qkv, ck, cv, lt = make_random([3, 4], dev, 1, c=8)
    tab = table(dev)
    with pytest.raises(ValueError, match="capacity"):
        ops.attention_decode_gqa(qkv, tab, ck, cv, lt, H, HKV, 9)
    with pytest.raises(ValueError, match="at least 1"):
        ops.attention_decode_gqa(qkv, tab, ck, cv, lt, H, HKV, 0)
    with pytest.raises(ValueError, match="rotary table"):
        ops.attention_decode_gqa(qkv, tab[:4], ck, cv, lt, H, HKV, 8)
    with pytest.raises(ValueError, match="multiple of num_kv_heads"):
        ops.attention_decode_gqa(qkv, tab, ck, cv, lt, 5, 3, 8)
    with pytest.raises(ValueError, match="cache must be"):
        ops.attention_decode_gqa(qkv, tab, ck[:, :1], cv[:, :1], lt, H, HKV, 8)
    with pytest.raises(ValueError, match="lens"):
        ops.attention_decode_gqa(qkv, tab, ck, cv, lt.long(), H, HKV, 8)
    with pytest.raises(ValueError, match="capacity"):
        ops.kv_cache_fill_gqa(torch.zeros(B, 9, 3 * H * D, device=dev).bfloat16(), ck, cv, H, HKV)
