"""Head-dim-128 rotary grouped-query decode attention and its cache fill (GPU only;
csrc/kernels/attn_decode_d128.hip), and a head-dim-128 model through prefill, decode steps and the graph session.

Inputs, references and the tolerance (`check`, M = 2) are tests/test_attention_decode_gqa_gpu.py's, whose helpers
are generic in the head dimension they read from that module's ``D``: the fixture below points them at 128 for
this file's tests.  B = 2 rows of DIFFERENT lengths, H = 4, Hkv = 2, C = 1024 unless said otherwise.  The model's
logits use the full ``forward``'s error as the yardstick, as tests/test_llama_generate_gpu.py does.

Edges, from the kernel's constants: 16 lanes own a key, so a workgroup is 16 key groups (edge 16); a group takes
U = 4 keys per round (2 at G = 8), key j of a split sitting in slot (j / 16) % U: 32 and 48 are slot edges and
16 U = 64 (32) the round edge.  Splits are the D = 64 plan's: at B Hkv = 4 on 256 CUs chunk = 64 for every max_len
<= 1024, so the split edges are the multiples of 64; 64, 128, 512 and 960 are taken.  Lengths: 0, 1, C - 1 and +-1
around all of those, a long one paired with a short one, at the tight max_len and at max_len = C.  B Hkv = 128
gives nsplit = 2, chunk = 512 (eight rounds per split) and B Hkv = 256 the single-split direct-output path.

Measured on an MI355X, ulp term subtracted: kernel (78 comparisons) at most -0.000 (max form; B Hkv = 256) and
-0.069 (rms; n = (961, 15)), plain kernel / emulation error at most 1.00; model (8) 0.842 (max; row 1, step 2)
and 0.433 (rms; row 0, prefill), plain decode / forward error 1.72 and 1.06.  So M = 2 holds as it stands.
"""
import importlib
import math

import pytest
import torch

import test_attention_decode_gqa_gpu as T
from conftest import gpu_device
from test_attention_decode_gqa_gpu import B, C, H, HKV, _bits, _garbage
from test_attention_edges_gpu import check
from test_llama_generate_gpu import LENS, _eager_loop, _padded, _tokens, forward64

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.models import LlamaKVCache, cast_params, llama_tiny
from databricks_distributed_deep_learning_amd.models._decode_graph import round_capacity
from databricks_distributed_deep_learning_amd.ops import _native_attn_cache as ND

A = importlib.import_module("databricks_distributed_deep_learning_amd.ops.attention")    # the module, not the op
pytestmark = pytest.mark.gpu

D = 128
EDGES = [16, 32, 48, 64, 128, 512, 960]
LENGTHS = sorted({0, 1, C - 2, C - 1} | {e + d for e in EDGES for d in (-1, 0, 1)})
PAIRS = list(zip(LENGTHS, reversed(LENGTHS)))


@pytest.fixture(autouse=True)
def _helpers_at_d128(monkeypatch):
    monkeypatch.setattr(T, "D", D)
    monkeypatch.setattr(T, "SCALE", 1.0 / math.sqrt(D))
    monkeypatch.setattr(T, "_TABLES", {})


@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
def test_parity_lengths(tight):
    dev, fails = gpu_device(), []
    for i, lens in enumerate(PAIRS):
        qkv, ck, cv, lt = T.make_random(lens, dev, 100 + i)
        T._check_case(fails, f"random n={lens}", qkv, T.table(dev), ck, cv, lt, max(lens) + 1 if tight else C)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("b,h,hkv,want", [(2, 2, 2, 16), (2, 4, 2, 16), (2, 3, 1, 16), (2, 8, 2, 16), (2, 8, 1, 16),
                                          (8, 32, 16, 2), (16, 32, 16, 1)],
                         ids=["G1", "G2", "G3", "G4", "G8", "bhkv128-2splits", "bhkv256-1split"])
def test_parity_groups_and_geometries(b, h, hkv, want):
    dev, fails = gpu_device(), []
    lens = [1023, 65] + [LENGTHS[(3 * i + 1) % len(LENGTHS)] for i in range(b - 3)] + [0] * (b > 2)
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert ND.plan_gqa(b, hkv, C)[0] == want
    qkv, ck, cv, lt = T.make_random(lens, dev, 40 + h + b, b, h, hkv)
    T._check_case(fails, f"random B={b} H={h} Hkv={hkv}", qkv, T.table(dev), ck, cv, lt, C, h, hkv)
    assert not fails, "\n".join(fails)


def routing_targets(n):
    """Position 0, the last cached key, the new key, both sides of the group edge 16 and of the split edges 64 k."""
    return [t for t in [0, n - 1, n, 15, 16] + [e + d for e in range(64, n + 1, 64) for d in (-1, 0)] if 0 <= t <= n]


@pytest.mark.parametrize("lens", [(1023, 129), (65, 1), (0, 960)], ids=str)
def test_routing(lens):
    """Identity table; query heads of a group aim at different keys, KV heads hold different codes: a wrong h / G
    mapping, a shared softmax state or a dropped key fails.  A NaN dead tail gives the zero tail's bits."""
    dev = gpu_device()
    tab, fails = T.table(dev, "identity"), []
    cyc = [routing_targets(n) for n in lens]
    for i in range(-(-max(len(c) for c in cyc) // H)):
        targets = [[cyc[b][(i * H + h) % len(cyc[b])] for h in range(H)] for b in range(B)]
        qkv, ck, cv, lt = T.make_routing(lens, targets, dev, 31 * i + sum(lens), "zeros")
        r64, p = T.reference(qkv, tab, ck, cv, lt, H, HKV, torch.float64)
        assert min(p[b, h, targets[b][h]].item() for b in range(B) for h in range(H)) >= 0.999
        em = T.reference(qkv, tab, ck, cv, lt, H, HKV, torch.float32)[0].bfloat16()
        out = T.run(qkv, tab, ck, cv, lt, C)
        check(fails, f"routing n={lens} targets={targets}", out, r64, em)
        qn, kn, vn, _ = T.make_routing(lens, targets, dev, 31 * i + sum(lens), "nan")
        assert torch.isfinite(out.float()).all() and torch.equal(_bits(out), _bits(T.run(qn, tab, kn, vn, lt, C)))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("lens,tight", [((1023, 0), False), ((5, 700), True), ((64, 63), True)], ids=str)
def test_rotation_and_append(lens, tight):
    """cache[b, :, n_b] becomes the rotated key (swap table: exactly [-k[64:], k[:64]]; real: within one bf16 ulp of
    an fp64 rotation) and the value's bits, position C - 1 too; nothing else changes; n = 0 returns the value row."""
    dev = gpu_device()
    qkv, ck0, cv0, lt = T.make_random(lens, dev, 17)
    x = qkv.view(B, H + 2 * HKV, D)
    k, v, bi = x[:, H:H + HKV], x[:, H + HKV:], torch.arange(B, device=dev)
    for kind in ("swap", "real"):
        ck, cv = ck0.clone(), cv0.clone()
        out = T.run(qkv, T.table(dev, kind), ck, cv, lt, max(lens) + 1 if tight else C)
        got = ck[bi, :, lt.long()]
        if kind == "swap":
            assert torch.equal(_bits(got), _bits(torch.cat([-k[..., 64:], k[..., :64]], -1)))
        else:
            row = T.table(dev)[lt.long()].double()
            cos, sin, k1, k2 = row[:, None, :64], row[:, None, 64:], k[..., :64].double(), k[..., 64:].double()
            w = torch.cat([k1 * cos - k2 * sin, k2 * cos + k1 * sin], -1).bfloat16().double()
            assert ((got.double() - w).abs() <= torch.ldexp(torch.ones_like(w), torch.frexp(w).exponent - 8)).all()
        wk, wv = ck0.clone(), cv0.clone()
        wk[bi, :, lt.long()], wv[bi, :, lt.long()] = got, v
        assert torch.equal(_bits(ck), _bits(wk)) and torch.equal(_bits(cv), _bits(wv)) and lt.tolist() == list(lens)
        for b in (b for b, n in enumerate(lens) if n == 0):
            assert torch.equal(_bits(out[b].view(HKV, H // HKV, D)), _bits(v[b, :, None].expand(HKV, H // HKV, D)))


def _raise(*a, **k):
    raise AssertionError("the reference path was taken")


@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("S", [1, 65])
def test_kv_cache_fill_d128(S, G, monkeypatch):
    dev = gpu_device()
    monkeypatch.setattr(A, "kv_cache_fill_gqa_reference", _raise)
    cap, h = 96, HKV * G
    packed = torch.randn(B, S, 3 * h * D, device=dev).bfloat16()
    ck, cv = _garbage((B, HKV, cap, D), dev, 1), _garbage((B, HKV, cap, D), dev, 2)
    wk, wv = ck.clone(), cv.clone()
    p5 = packed.view(B, S, 3, h, D)
    for j in range(HKV):
        wk[:, j, :S], wv[:, j, :S] = p5[:, :, 1, j * G], p5[:, :, 2, j * G]
    ops.kv_cache_fill_gqa(packed, ck, cv, h, HKV)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ck), _bits(wk)) and torch.equal(_bits(cv), _bits(wv))


def test_native_path_is_taken_and_repeatable(monkeypatch):
    """D = 128 decode runs with its reference patched to raise, two runs over several splits bitwise equal; D = 128
    extend still works, through its own reference."""
    dev = gpu_device()
    assert ND.supported_decode(H, HKV, 128) and ND.supported(H, HKV) and not ND.supported(H, HKV, 128)
    qkv, ck, cv, lt = T.make_random((200, 33), dev, 9)
    tab, fails = T.table(dev), []
    ext = ops.attention_extend_gqa(qkv.view(B, 1, -1), tab, ck.clone(), cv.clone(), lt, H, HKV, 200)
    monkeypatch.setattr(A, "attention_decode_gqa_reference", _raise)
    T._check_case(fails, "patched", qkv, tab, ck, cv, lt, 201)
    check(fails, "extend T=1", ext.view(B, -1), T.reference(qkv, tab, ck, cv, lt, H, HKV, torch.float64)[0],
          T.reference(qkv, tab, ck, cv, lt, H, HKV, torch.float32)[0].bfloat16())
    assert not fails, "\n".join(fails)
    a, b = (T.run(qkv, tab, ck.clone(), cv.clone(), lt, C) for _ in range(2))
    assert ND.plan_gqa(B, HKV, C)[0] > 1 and torch.equal(_bits(a), _bits(b))


def test_model_d128(monkeypatch):
    """Prefill + 3 teacher-forced decode steps against `forward64`; then the graph session (no reference decode
    attention in it) against the eager loop at the same launch bound, bitwise."""
    dev, steps = gpu_device(), 3
    torch.manual_seed(0)
    model = llama_tiny(hidden_size=256).eval().to(dev)
    cast_params(model, torch.bfloat16)
    prompts, forced = _tokens()
    ids, mask = _padded(prompts)
    S = ids.shape[1]
    comp = torch.zeros_like(ids)
    for b, r in enumerate(prompts):
        comp[b, :len(r)] = r
    cache = LlamaKVCache.allocate(model, B, S + steps)
    got = [model.prefill(comp.to(dev), torch.tensor(LENS, dtype=torch.int32, device=dev), cache)]
    got += [model.decode_step(forced[:, t].to(dev), cache) for t in range(steps)]
    fails = []
    with torch.no_grad():
        for b, r in enumerate(prompts):
            full, rows = torch.cat([r, forced[b, :steps]]), slice(len(r) - 1, len(r) + steps)
            ref, fwd = forward64(model, full)[rows], model(full[None].to(dev))[0, rows].float().cpu()
            for t in range(steps + 1):
                check(fails, f"row {b} " + ("prefill" if t == 0 else f"decode step {t - 1}"), got[t][b].float().cpu(),
                      ref[t], fwd[t])
    assert not fails, "\n".join(fails)
    cap = round_capacity(S + steps, model.config.max_position_embeddings)
    want = _eager_loop(model, prompts, steps, dev, cap)
    monkeypatch.setattr(A, "attention_decode_gqa_reference", _raise)
    a = model.generate(ids.to(dev), attention_mask=mask.to(dev), max_new_tokens=steps, use_graph=True)
    sess = model.decode_session
    assert sess.graph is not None and sess.captures == 1 and sess.cache.data.shape[-1] == D
    assert torch.equal(a[:, S:].cpu(), want)
