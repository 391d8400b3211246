"""Head-dim-128 decode attention over an FP8 KV cache, its quantising append and fill (GPU only;
csrc/kernels/attn_decode_d128_fp8.hip), and a head-dim-128 model on an FP8 cache.  Inputs, lengths, geometries and
`check` (M = 2) are tests/test_attention_decode_d128_gpu.py's, its bf16 caches quantised by ``quantize_fp8_rows``.

Measured on an MI355X, ulp term subtracted: kernel (77 comparisons) at most 0.000 (max form; B Hkv = 256) and
-0.108 (rms; n = (961, 15)), plain kernel / emulation error at most 1.00; model (8) 0.846 (max) and 0.796 (rms; both
row 0, decode step 1), plain ratios 1.19 and 1.01.  So M = 2 holds as it stands.
"""
import copy
import math

import pytest
import torch

import test_attention_decode_gqa_gpu as T
from conftest import gpu_device
from test_attention_decode_d128_gpu import ND, PAIRS, A, _helpers_at_d128, _raise, routing_targets  # noqa: F401
from test_attention_decode_gqa_gpu import B, C, H, HKV
from test_attention_edges_gpu import check
from test_llama_generate_gpu import LENS, _padded, _tokens

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.models import LlamaKVCache, cast_params, llama_tiny
from databricks_distributed_deep_learning_amd.models._decode_graph import round_capacity

pytestmark = pytest.mark.gpu
D, F8, U8 = 128, torch.float8_e4m3fn, torch.uint8


def quant(x):
    """[..., 128] -> (uint8 bytes, fp32 scales [...]) on x's device, computed on the CPU: there ``amax / 448`` is the
    format's true division (torch's GPU division by a scalar multiplies by the rounded reciprocal)."""
    q, s = ops.quantize_fp8_rows(x.reshape(-1, D).cpu())
    return q.view(U8).view(x.shape).to(x.device), s.view(x.shape[:-1]).to(x.device)


def run(qkv, tab, cache, lens, max_len, h=H, hkv=HKV):
    """cache = (K bytes, K scales, V bytes, V scales), copied -> out and the four tensors as the kernel left them."""
    kq, ks, vq, vs = cache = [t.clone() for t in cache]
    out = ops.attention_decode_gqa_fp8(qkv, tab, kq, vq, ks, vs, lens, h, hkv, max_len)
    torch.cuda.synchronize()
    return out, cache


def reference(qkv, tab, cache, lens, h, hkv, dt):
    """T.reference, but over the dequantised cache as the kernel left it: T's puts the unquantised new key at n."""
    b, L, n = qkv.shape[0], int(lens.max()) + 1, lens.long()
    q = T.rotate_once(qkv, tab, lens, h, hkv)[0].to(dt)
    kk, vv = (c[:, :, :L].view(F8).float().to(dt) * s[:, :, :L, None].to(dt) for c, s in zip(cache[::2], cache[1::2]))
    live = torch.arange(L, device=qkv.device).view(1, 1, 1, L) <= n.view(b, 1, 1, 1)
    s = (q.view(b, hkv, h // hkv, D) @ kk.transpose(-1, -2)) * T.SCALE
    p = torch.softmax(torch.where(live, s, torch.full_like(s, -math.inf)), -1)
    vv = torch.where(live.view(b, 1, L, 1), vv, torch.zeros_like(vv))
    return (p @ vv).reshape(b, h * D), p.reshape(b, h, L)


def check_case(fails, label, qkv, tab, cache, lens, max_len, h=H, hkv=HKV):
    out, after = run(qkv, tab, cache, lens, max_len, h, hkv)
    assert torch.isfinite(out.float()).all(), label
    r64, p = reference(qkv, tab, after, lens, h, hkv, torch.float64)
    check(fails, label, out, r64, reference(qkv, tab, after, lens, h, hkv, torch.float32)[0].bfloat16())
    return out, p


GEOMS = {"G1": (2, 2, 2, 16), "G2": (2, 4, 2, 16), "G3": (2, 3, 1, 16), "G4": (2, 8, 2, 16), "G8": (2, 8, 1, 16),
         "bhkv128-2splits": (8, 32, 16, 2), "bhkv256-1split": (16, 32, 16, 1)}         # b, h, hkv, splits at C


@pytest.mark.parametrize("case", ["tight", "capacity"] + list(GEOMS))
def test_parity(case, monkeypatch):
    """Every pair of edge lengths at H = 4, Hkv = 2, at the tight max_len and at C; then the group sizes and plans."""
    monkeypatch.setattr(A, "attention_decode_gqa_fp8_reference", _raise)
    dev, fails = gpu_device(), []
    b, h, hkv, want = GEOMS.get(case, (B, H, HKV, 16))
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert ND.plan_gqa(b, hkv, C)[0] == want                # the fp8 op launches by the same plan
    mixed = [1023, 65] + [(37 * i + 1) % 1000 for i in range(b - 3)] + [0] * (b > 2)
    for i, lens in enumerate([mixed] if case in GEOMS else PAIRS):
        qkv, ck, cv, lt = T.make_random(lens, dev, 40 + h + b if case in GEOMS else 100 + i, b, h, hkv)
        check_case(fails, f"{case} n={lens}", qkv, T.table(dev), quant(ck) + quant(cv), lt,
                   max(lens) + 1 if case == "tight" else C, h, hkv)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("lens", [(1023, 129), (65, 1), (0, 960)], ids=str)
def test_routing_and_dead_rows(lens):
    """The d128 routing construction with odd positions' keys 1.5 x their code (a target's key scale differs from
    its neighbours'; every value row has its own).  NaN codes and NaN scales in dead rows change no bit."""
    dev = gpu_device()
    tab, fails = T.table(dev, "identity"), []
    cyc = [routing_targets(n) for n in lens]
    for i in range(-(-max(len(c) for c in cyc) // H)):
        targets = [[cyc[b][(i * H + h) % len(cyc[b])] for h in range(H)] for b in range(B)]
        qkv, ck, cv, lt = T.make_routing(lens, targets, dev, 31 * i + sum(lens), "zeros")
        ck[:, :, 1::2] *= 1.5
        kq, ks, vq, vs = cache = quant(ck) + quant(cv)
        out, p = check_case(fails, f"routing n={lens} targets={targets}", qkv, tab, cache, lt, C)
        assert min(p[b, h, targets[b][h]].item() for b in range(B) for h in range(H)) >= 0.999
        for b, n in enumerate(lens):
            kq[b, :, n + 1::2], kq[b, :, n + 2::2], vq[b, :, n + 1:] = 0x7F, 0xFF, 0xFF
            ks[b, :, n + 1:], vs[b, :, n + 1:] = math.nan, math.nan
        assert torch.equal(out.view(torch.int16), run(qkv, tab, cache, lt, C)[0].view(torch.int16))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("lens,tight", [((1023, 0), False), ((5, 700), True), ((64, 63), True)], ids=str)
@pytest.mark.parametrize("kind", ["swap", "real"])
def test_append(lens, tight, kind):
    """V row = quantize_fp8_rows(v); K row = that of the swapped key (swap table) or, dequantised, within one bf16 ulp
    of the fp64 rotation w plus half an e4m3 step of the rounded key x, |x| <= |w| + ulp: 2^-4 |x|, or 2^-10 scale if
    subnormal.  The code is the fp32 quotient fl(x / scale)'s, 2^-24 relative from the true one: 2^-24 |x| = 2^-20
    |x| / 16 more and 2^-24 on the half step, so x (1 + 17 * 2^-24).  Nothing else in the four tensors changes."""
    dev = gpu_device()
    qkv, ck, cv, lt = T.make_random(lens, dev, 17)
    x = qkv.view(B, H + 2 * HKV, D)
    k, v, bi, n = x[:, H:H + HKV], x[:, H + HKV:], torch.arange(B, device=dev), lt.long()
    before = quant(ck) + quant(cv)
    gk, gks, gv, gvs = after = run(qkv, T.table(dev, kind), before, lt, max(lens) + 1 if tight else C)[1]
    wq, ws = quant(v)
    assert torch.equal(gv[bi, :, n], wq) and torch.equal(gvs[bi, :, n], ws)
    if kind == "swap":
        wq, ws = quant(torch.cat([-k[..., 64:], k[..., :64]], -1))
        assert torch.equal(gk[bi, :, n], wq) and torch.equal(gks[bi, :, n], ws)
    else:
        row = T.table(dev)[n].double()
        cos, sin, k1, k2 = row[:, None, :64], row[:, None, 64:], k[..., :64].double(), k[..., 64:].double()
        w = torch.cat([k1 * cos - k2 * sin, k2 * cos + k1 * sin], -1)
        sc = gks[bi, :, n].double().unsqueeze(-1)
        ulp = torch.ldexp(torch.ones_like(w), torch.frexp(w).exponent - 8)
        bound = ulp + torch.maximum((w.abs() + ulp) / 16, sc / 1024) * (1 + 17 * 2.0 ** -24)
        assert ((gk[bi, :, n].view(F8).float().double() * sc - w).abs() <= bound).all()
    for got, old in zip(after, before):
        want = old.clone()
        want[bi, :, n] = got[bi, :, n]
        assert torch.equal(got.view(U8), want.view(U8))      # (bytes: NaN scales of dead rows compare equal)


def test_every_code_through_fill_and_append(monkeypatch):
    """Rows of amax 448 with every non-negative code, every midpoint between neighbours, their negatives; zeros;
    -0.0; subnormal bf16 values; an amax that is no power of two: bytes and scales equal quantize_fp8_rows'."""
    monkeypatch.setattr(A, "kv_cache_fill_gqa_fp8_reference", _raise)
    dev = gpu_device()
    torch.manual_seed(5)
    codes = torch.arange(127, dtype=U8).view(F8).float()
    pos, mid = torch.cat([codes, codes[-1:]]), torch.cat([(codes[:-1] + codes[1:]) / 2, codes[-1:], codes[-1:]])
    nz = torch.zeros(128)
    nz[::2], nz[1] = -0.0, 448.0
    sub = torch.arange(1, 129, dtype=torch.int16).view(torch.bfloat16).float()
    rows = torch.stack([pos, -pos, mid, -mid, torch.zeros(128), nz, sub, torch.randn(128) * 3]).bfloat16()
    wq, ws = quant(rows := rows.view(2, 4, D))                 # [b, hkv, D]
    assert torch.equal(rows[0, 2].float(), mid) and ws[0].tolist() == [1.0] * 4 and ws[1, 0] == 1.0
    # fill: H = Hkv = 4, S = 1; K third = the rows, V third = the rows in reverse order
    packed = torch.zeros(2, 1, 3, 4, D, dtype=torch.bfloat16)
    packed[:, 0, 1], packed[:, 0, 2] = rows, rows.flip(0, 1)
    kq, ks, vq, vs = cache = [torch.zeros(2, 4, 2, D, dtype=U8, device=dev), torch.zeros(2, 4, 2, device=dev),
                              torch.zeros(2, 4, 2, D, dtype=U8, device=dev), torch.zeros(2, 4, 2, device=dev)]
    ops.kv_cache_fill_gqa_fp8(packed.view(2, 1, -1).to(dev), kq, vq, ks, vs, 4, 4)
    for got, want in zip(cache, (wq, ws, wq.flip(0, 1), ws.flip(0, 1))):
        assert torch.equal(got[:, :, 0].cpu().view(U8), want.contiguous().view(U8))
    # append at position 1, identity table: V = the rows, K = the reference rotation's (exact, signed zeros apart)
    qkv = torch.cat([torch.randn(2, 4, D).bfloat16(), rows, rows], 1).view(2, -1).to(dev)
    lt, tab = torch.ones(2, dtype=torch.int32, device=dev), T.table(dev, "identity")
    kq2, ks2 = quant(T.rotate_once(qkv, tab, lt, 4, 4)[1].cpu())
    for g, want in zip(run(qkv, tab, cache, lt, 2, 4, 4)[1], (kq2, ks2, wq, ws)):
        assert torch.equal(g[:, :, 1].cpu().view(U8), want.contiguous().view(U8))


def test_model_fp8_cache(monkeypatch):
    """Prefill + 3 forced decode steps: layer 0's V bytes and scales against the bf16-cache run's; logits against an
    fp64 copy on the reference fp8 ops (emulation: the bf16 reference-op path).  Then the graph session against the
    eager greedy loop at the same launch bound: tokens, and every layer's live cache bytes and scales, bitwise."""
    dev, steps = gpu_device(), 3
    torch.manual_seed(0)
    model = llama_tiny(hidden_size=256).eval().to(dev)
    cast_params(model, torch.bfloat16)
    prompts, forced = _tokens()
    ids, mask = _padded(prompts)
    S = ids.shape[1]
    comp = torch.stack([torch.nn.functional.pad(r, (0, S - len(r))) for r in prompts])

    def roll(m, d, fp8, toks=None, cap=S + steps, **kw):
        cache = LlamaKVCache.allocate(m, B, cap, fp8=fp8)
        out = [m.prefill(comp.to(d), torch.tensor(LENS, dtype=torch.int32, device=d), cache)]
        for t in range(steps):
            out.append(m.decode_step(out[-1].argmax(-1) if toks is None else toks[:, t].to(d), cache, **kw))
        return torch.stack(out).double().cpu(), cache

    got, c8 = roll(model, dev, True, forced)
    c16 = roll(model, dev, False, forced)[1]
    for b, n in enumerate(LENS):
        wq, ws = quant(c16.v(0)[b, :, :n + steps])
        assert torch.equal(c8.v(0)[b, :, :n + steps].view(U8), wq) and torch.equal(c8.v_scale(0)[b, :, :n + steps], ws)
    ref = roll(copy.deepcopy(model).cpu().double(), "cpu", True, forced)[0]
    em = roll(copy.deepcopy(model).cpu(), "cpu", True, forced)[0]
    fails = []
    for t in range(steps + 1):
        for b in range(B):
            check(fails, f"row {b} step {t - 1}", got[t, b], ref[t, b], em[t, b])
    assert not fails, "\n".join(fails)
    cap = round_capacity(S + steps + 1, model.config.max_position_embeddings)
    eager, ce = roll(model, dev, True, None, cap, len_bound=cap)
    monkeypatch.setattr(A, "attention_decode_gqa_fp8_reference", _raise)
    a = model.generate(ids.to(dev), attention_mask=mask.to(dev), max_new_tokens=steps + 1, use_graph=True,
                       kv_cache_dtype="fp8")
    sess = model.decode_session
    assert sess.graph is not None and sess.captures == 1 and sess.capacity == cap and sess.cache.data.dtype == F8
    assert torch.equal(a[:, S:].cpu(), eager.argmax(-1).t()) and torch.equal(sess.cache.lens, ce.lens)
    for b, n in enumerate(ce.lens.tolist()):
        assert torch.equal(sess.cache.data.view(U8)[:, :, b, :, :n], ce.data.view(U8)[:, :, b, :, :n])
        assert torch.equal(sess.cache.scales[:, :, b, :, :n], ce.scales[:, :, b, :, :n])
