"""Single-query attention over a KV cache and the cache fill (GPU only; csrc/kernels/attn_decode.hip).

Every case has two batch rows of DIFFERENT lengths (B = 2, H = 2, C = 1024 unless said otherwise).

Boundaries the kernel has.  A workgroup is 32 key groups of 8 lanes and takes 4 keys per group per
round: key j of a split sits in unroll slot (j / 32) % 4, so 32 is the slot edge and 128 the round
edge.  Splits: nsplit = min(16, ceil(CUs / (B H)), ceil(max_len / 64)) and chunk = ceil(max_len / nsplit)
rounded up to 32; at B H = 4 on 256 CUs that is chunk = 64 for every max_len <= 1024 (nsplit = 1 for
max_len <= 64, 16 at max_len = 1024).  Lengths: the issue's {0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255,
256, 257, 1022, 1023} plus +-1 around slot edges (31, 32, 33), further split edges (191, 192, 193, 511,
512, 513) and the last split's edge (959, 960, 961); each length runs with max_len = the tight bound
(max n + 1) and with max_len = C (trailing splits empty).  Two more geometries cover what B H = 4 cannot:
B H = 128 (nsplit = 2, chunk = 512: four rounds per split) and B H = 256 (nsplit = 1, chunk = max_len: the
direct-output path with eight rounds).

Tolerance: the form of tests/test_attention_edges_gpu.py (`check`, M = 2), the emulation being fp32
throughout with a bf16 output; reference fp64 from the bf16 inputs.  Every case prints its ratios.

Measured on an MI355X: 218 comparisons in this file.  With the ulp term subtracted the largest
ratios are -0.003 (max form; random inputs, n = (64, 256)) and -0.188 (rms form; n = (191, 129)): the kernel
never exceeds the fp32 emulation's error by more than half a bf16 ulp.  As plain kernel error / emulation
error the largest are 1.00 (max and rms; random, routing and the three chain steps alike).  So M = 2 holds
as it stands.
"""
import math

import pytest
import torch

from conftest import gpu_device
from test_attention_edges_gpu import D, M, _half_ulp_bf16, _split, check  # noqa: F401

from databricks_distributed_deep_learning_amd import ops

pytestmark = pytest.mark.gpu

B, H, C = 2, 2, 1024
LENGTHS = [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 959,
           960, 961, 1022, 1023]
PAIRS = list(zip(LENGTHS, reversed(LENGTHS)))
SCALE = 1.0 / math.sqrt(D)


def _garbage(shape, dev, seed):
    """Arbitrary bf16 bit patterns, NaN and Inf among them."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-32768, 32767, shape, generator=g, dtype=torch.int16).to(dev).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16)


def make_random(lens, dev, seed, b=B, h=H, c=C):
    """qkv_new [b, 3 h D], caches [b, h, c, D] (live rows randn, the rest arbitrary bits), lens int32."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(b, 3 * h * D, generator=g).bfloat16().to(dev)
    ck, cv = _garbage((b, h, c, D), dev, seed + 1), _garbage((b, h, c, D), dev, seed + 2)
    for i, n in enumerate(lens):
        ck[i, :, :n] = torch.randn(h, n, D, generator=g).bfloat16().to(dev)
        cv[i, :, :n] = torch.randn(h, n, D, generator=g).bfloat16().to(dev)
    return qkv, ck, cv, torch.tensor(lens, dtype=torch.int32, device=dev)


def reference(qkv, ck, cv, lens, h, dt):
    """out [b, h D] in dtype dt, and the attention weights [b, h, L]: keys 0 .. n-1 from the cache, key n
    the new one."""
    b = qkv.shape[0]
    L = int(lens.max()) + 1
    q, k, v = qkv.to(dt).view(b, 3, h, D).unbind(1)
    kk, vv = ck[:, :, :L].to(dt).clone(), cv[:, :, :L].to(dt).clone()
    bi, n = torch.arange(b, device=qkv.device), lens.long()
    kk[bi, :, n], vv[bi, :, n] = k, v
    live = torch.arange(L, device=qkv.device).view(1, 1, L) <= n.view(b, 1, 1)
    s = (kk @ q.unsqueeze(-1)).squeeze(-1) * SCALE
    p = torch.softmax(torch.where(live, s, torch.full_like(s, -math.inf)), -1)
    vv = torch.where(live.unsqueeze(-1), vv, torch.zeros_like(vv))
    return (p.unsqueeze(2) @ vv).squeeze(2).reshape(b, h * D), p


def run(qkv, ck, cv, lens, max_len, h=H):
    out = ops.attention_decode(qkv, ck, cv, lens, h, max_len)
    torch.cuda.synchronize()
    return out


def _check_case(fails, label, qkv, ck, cv, lens, max_len, h=H):
    r64, _ = reference(qkv, ck, cv, lens, h, torch.float64)
    em = reference(qkv, ck, cv, lens, h, torch.float32)[0].bfloat16()
    out = run(qkv, ck.clone(), cv.clone(), lens, max_len, h)
    assert torch.isfinite(out.float()).all(), label
    check(fails, label, out, r64, em)


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
def test_parity_random(tight):
    dev = gpu_device()
    fails = []
    for i, lens in enumerate(PAIRS):
        qkv, ck, cv, lt = make_random(lens, dev, 100 + i)
        _check_case(fails, f"random n={lens}", qkv, ck, cv, lt, max(lens) + 1 if tight else C)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("b,h", [(8, 16), (16, 16)], ids=["bh128-2splits", "bh256-1split"])
def test_parity_other_geometries(b, h):
    """Long splits (several rounds each) and the direct-output path at a long length."""
    from databricks_distributed_deep_learning_amd.ops import _native_attn_cache as ND
    dev = gpu_device()
    lens = [(LENGTHS[(3 * i + 1) % len(LENGTHS)]) for i in range(b)]
    lens[0], lens[-1] = 1023, 0
    nsplit, chunk = ND.plan(b, h, C)
    print(f"plan B H = {b * h}: nsplit {nsplit} chunk {chunk}")
    fails = []
    qkv, ck, cv, lt = make_random(lens, dev, 7, b, h)
    _check_case(fails, f"random B={b} H={h}", qkv, ck, cv, lt, C, h)
    assert not fails, "\n".join(fails)


def test_plan_is_what_the_docstring_says():
    from databricks_distributed_deep_learning_amd.ops import _native_attn_cache as ND
    gpu_device()
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        return      # the listed split edges are those of a 256-CU part
    assert ND.plan(B, H, 1024) == (16, 64) and ND.plan(B, H, 64) == (1, 64) and ND.plan(B, H, 65) == (2, 64)
    assert ND.plan(B, H, 514) == (9, 64) and ND.plan(8, 16, 1024) == (2, 512) and ND.plan(16, 16, 1024) == (1, 1024)


def test_single_key_is_the_value_row_bitwise():
    """n = 0: a softmax over one key is exactly 1."""
    dev = gpu_device()
    for max_len in (6, C):
        qkv, ck, cv, lt = make_random([0, 5], dev, 3)
        out = run(qkv, ck, cv, lt, max_len)
        assert torch.equal(_bits(out[0]), _bits(qkv.view(B, 3, H * D)[0, 2]))


# ------------------------------------------------------------------ routing
def make_routing(lens, targets, dev, seed, dead=None):
    """K = +-1 codes, q = 4 code[target], V = randn: the whole weight sits on one key.  targets [B][H].
    dead: None (tail = arbitrary bits) | 'zeros' | 'decoys' (K = 2 x the target's code, V = 8) | 'nan'."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.empty(B, 3, H, D)
    ck, cv = _garbage((B, H, C, D), "cpu", seed + 1), _garbage((B, H, C, D), "cpu", seed + 2)
    for b, n in enumerate(lens):
        for h in range(H):
            code = torch.randint(0, 2, (n + 1, D), generator=g).float() * 2 - 1
            val = torch.randn(n + 1, D, generator=g)
            t = targets[b][h]
            ck[b, h, :n], cv[b, h, :n] = code[:n].bfloat16(), val[:n].bfloat16()
            qkv[b, 0, h], qkv[b, 1, h], qkv[b, 2, h] = 4.0 * code[t], code[n], val[n]
            if dead == "zeros":
                ck[b, h, n:], cv[b, h, n:] = 0.0, 0.0
            elif dead == "decoys":
                ck[b, h, n:], cv[b, h, n:] = (2.0 * code[t]).bfloat16(), 8.0
            elif dead == "nan":
                ck[b, h, n:], cv[b, h, n:] = math.nan, math.nan
    return (qkv.reshape(B, 3 * H * D).bfloat16().to(dev), ck.to(dev), cv.to(dev),
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
    dev = gpu_device()
    cyc = [target_cycle(n) for n in lens]
    fails = []
    for i in range(-(-max(len(c) for c in cyc) // H)):
        targets = [[cyc[b][(i * H + h) % len(cyc[b])] for h in range(H)] for b in range(B)]
        qkv, ck, cv, lt = make_routing(lens, targets, dev, 31 * i + sum(lens))
        r64, p = reference(qkv, ck, cv, lt, H, torch.float64)
        for b in range(B):
            for h in range(H):
                assert p[b, h, targets[b][h]].item() >= 0.999
        em = reference(qkv, ck, cv, lt, H, torch.float32)[0].bfloat16()
        out = run(qkv, ck, cv, lt, max(lens) + 1 if tight else C)
        check(fails, f"routing n={lens} targets={targets}", out, r64, em)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("lens", [(1022, 63), (128, 7), (0, 960)], ids=str)
def test_dead_tail_cannot_reach_the_output(lens):
    dev = gpu_device()
    targets = [[0, n] for n in lens]
    outs = []
    for dead in ("zeros", "decoys", "nan"):
        qkv, ck, cv, lt = make_routing(lens, targets, dev, 5, dead)
        outs.append(run(qkv, ck, cv, lt, C))
        assert torch.isfinite(outs[-1].float()).all()
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))


# ------------------------------------------------------------------ append, repeatability
@pytest.mark.parametrize("lens", [(1023, 0), (64, 63), (511, 1022), (5, 128)], ids=str)
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
def test_append(lens, tight):
    """cache[b, h, n_b] becomes the new K / V row; nothing else changes (n = C - 1, the last slot, included)."""
    dev = gpu_device()
    qkv, ck, cv, lt = make_random(lens, dev, 17)
    wk, wv = ck.clone(), cv.clone()
    _, k, v = qkv.view(B, 3, H, D).unbind(1)
    for b, n in enumerate(lens):
        wk[b, :, n], wv[b, :, n] = k[b], v[b]
    run(qkv, ck, cv, lt, max(lens) + 1 if tight else C)
    assert torch.equal(_bits(ck), _bits(wk)) and torch.equal(_bits(cv), _bits(wv))
    assert lt.tolist() == list(lens)


def test_repeatable():
    from databricks_distributed_deep_learning_amd.ops import _native_attn_cache as ND
    dev = gpu_device()
    assert ND.plan(B, H, C)[0] > 1
    qkv, ck, cv, lt = make_random([1000, 700], dev, 23)
    a = run(qkv, ck.clone(), cv.clone(), lt, C)
    b = run(qkv, ck.clone(), cv.clone(), lt, C)
    assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ cache fill
@pytest.mark.parametrize("S", [1, 63, 64, 65, 129])
def test_kv_cache_fill(S):
    dev = gpu_device()
    cap = 160
    qkv = torch.randn(B, S, 3 * H * D, device=dev).bfloat16()
    ck, cv = _garbage((B, H, cap, D), dev, 1), _garbage((B, H, cap, D), dev, 2)
    wk, wv = ck.clone(), cv.clone()
    _, k, v = _split(qkv, H)
    wk[:, :, :S], wv[:, :, :S] = k, v
    ops.kv_cache_fill(qkv, ck, cv, H)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ck), _bits(wk)) and torch.equal(_bits(cv), _bits(wv))


# ------------------------------------------------------------------ prefill + decode chain
def _causal(qkv, dt):
    q, k, v = _split(qkv.to(dt), H)
    S = qkv.shape[1]
    s = (q @ k.transpose(-1, -2)) * SCALE
    ar = torch.arange(S, device=qkv.device)
    s = s.masked_fill(ar[None, :] > ar[:, None], -math.inf)
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(qkv.shape[0], S, H * D)


def test_prefill_then_decode_chain():
    """Causal prefill of 65 tokens + fill, then 3 decode steps: step i is row 65 + i of a causal attention
    over all 68 tokens."""
    from databricks_distributed_deep_learning_amd.ops import _native_attention as NA
    dev = gpu_device()
    S0, steps = 65, 3
    qkv = torch.randn(B, S0 + steps, 3 * H * D, device=dev).bfloat16()
    r64, em = _causal(qkv, torch.float64), _causal(qkv, torch.float32).bfloat16()
    ck, cv = _garbage((B, H, C, D), dev, 1), _garbage((B, H, C, D), dev, 2)
    pre = qkv[:, :S0].contiguous()
    fails = []
    check(fails, "chain prefill", NA.attention(pre, H, None, 0.0, causal=True), r64[:, :S0], em[:, :S0])
    ops.kv_cache_fill(pre, ck, cv, H)
    lens = torch.full((B,), S0, dtype=torch.int32, device=dev)
    for i in range(steps):
        t = S0 + i
        out = run(qkv[:, t].contiguous(), ck, cv, lens, t + 1)
        check(fails, f"chain step {i}", out, r64[:, t], em[:, t])
        lens += 1
    assert not fails, "\n".join(fails)


def test_capacity_guard_is_on_the_host():
    dev = gpu_device()
    qkv, ck, cv, lt = make_random([3, 4], dev, 1, c=8)
    with pytest.raises(ValueError, match="capacity"):
        ops.attention_decode(qkv, ck, cv, lt, H, 9)
