"""FP8 (e4m3) weight-only linears at M <= 16 rows (csrc/kernels/linear_decode_fp8.hip through
ops.linear_small_m_fp8) and the Llama decode step on quantised weights (GPU only).

Parity: M in {1, 3, 16} x SHAPES x {none, bias, bias + GELU, bias + residual} against fp64 from x, the e4m3 values
and the scales, bounded by `check` (M = 2) of tests/test_attention_edges_gpu.py against an fp32 emulation (scale
after the matmul, bf16 output).  The fp8 plan puts 2 weight tiles on a wave up to N = 1024 and 4 above; on a
256-CU part (1, 16), (7, 128), (24, 144) run 2 tiles unsplit (N below a tile, N tails, K below / not a multiple
of the 128-deep step), (257, 1024) and (1024, 4096) 2 tiles with 2 and 8 K splits, (4100, 512) 4 tiles unsplit
and (1040, 1024), added, is the smallest 4-tile shape with a split.  The other cases compare bits.

Measured on an MI355X: 84 parity comparisons; with the ulp term subtracted the largest ratios are -0.000 (max)
and 0.102 (rms; M = 3, N = 7, K = 128, bias + GELU: 21 numbers), as plain kernel / emulation error 1.00.  Model:
0.351 (max; head dim 128, row 0) and 0.435 (rms; head dim 64, row 1), plain 0.83 at most.  So M = 2 holds.
"""
import copy

import pytest
import torch

from conftest import gpu_device
from test_attention_edges_gpu import M as MARGIN, check  # noqa: F401
from test_llama_generate_gpu import _eager_loop, forward64

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.models import LlamaKVCache, cast_params, llama_tiny
from databricks_distributed_deep_learning_amd.ops import _lib, _native_linear_decode_fp8 as NLF

pytestmark = pytest.mark.gpu

MS = [1, 3, 16]
SHAPES = [(1, 16), (7, 128), (24, 144), (257, 1024), (1024, 4096), (4100, 512), (1040, 1024)]
EPIS = ["none", "bias", "bias_gelu", "bias_res"]


def _inputs(m, n, k, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(m, k, generator=g).bfloat16().to(dev)
    wq, scale = ops.quantize_fp8_rows((torch.randn(n, k, generator=g) * k ** -0.5).to(dev))
    return x, wq, scale, torch.randn(n, generator=g).bfloat16().to(dev), torch.randn(m, n, generator=g).bfloat16().to(dev)


def _ref(x, wq, scale, b, r, epi, dt):
    y = (x.to(dt) @ wq.float().to(dt).t()) * scale.to(dt)
    if epi != "none":
        y = y + b.to(dt)
    if epi == "bias_gelu":
        y = torch.nn.functional.gelu(y)
    return y + r.to(dt) if epi == "bias_res" else y


def _args(b, r, epi):
    return (None if epi == "none" else b), ("gelu" if epi == "bias_gelu" else None), (r if epi == "bias_res" else None)


@pytest.mark.parametrize("n,k", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
def test_parity(n, k):
    dev = gpu_device()
    fails = []
    print(f"N={n} K={k}: plan {NLF.plan(n, k)}")
    for m in MS:
        x, wq, scale, b, r = _inputs(m, n, k, dev, 1000 * m + n + k)
        for epi in EPIS:
            y = ops.linear_small_m_fp8(x, wq, scale, *_args(b, r, epi))
            assert y.shape == (m, n) and y.dtype == torch.bfloat16
            check(fails, f"M={m} N={n} K={k} {epi}", y, _ref(x, wq, scale, b, r, epi, torch.float64),
                  _ref(x, wq, scale, b, r, epi, torch.float32).bfloat16())
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("split", [False, True])
def test_every_byte_code_exactly(split):
    """Row n holds byte code n at one column: the hardware's decode of every code (OCP, subnormals, -0) against
    torch's, a mis-indexed row and a lost or doubled k slice all change bits."""
    dev = gpu_device()
    n = 256
    k = next(kk for kk in range(16, 1 << 14, 16) if NLF.plan(n, kk)[2] > 1) if split else 272
    _, _, ksplit, per = NLF.plan(n, k)
    assert (ksplit > 1) == split
    edges = {0, k - 1}
    for step in (128, 128 * per):       # first and last element of every k step and of every wave's k range
        for a in range(0, k, step):
            edges |= {a, min(a + step, k) - 1}
    et = torch.tensor(sorted(edges), device=dev)
    ar = torch.arange(n, device=dev)
    val = ar.to(torch.uint8).view(torch.float8_e4m3fn).float()
    ok = ~val.isnan()                   # 0x7f and 0xff, the format's NaNs, are never emitted by the quantiser
    scale = torch.pow(2.0, (ar % 5 - 2).float())
    for m in MS:
        x = torch.randn(m, k, device=dev).bfloat16()
        for rot in range(-(-len(et) // n) + 1):
            kn = et[(ar + rot * 7) % len(et)]
            wq = torch.zeros(n, k, dtype=torch.uint8, device=dev)
            wq[ar[ok], kn[ok]] = ar[ok].to(torch.uint8)
            y = ops.linear_small_m_fp8(x, wq, scale)
            # (+ 0.0: the accumulator starts at +0, so a product of -0 -- codes 0x00 and 0x80 -- sums to +0)
            want = (x.float()[:, kn] * val * scale + 0.0).bfloat16()
            bad = (y.view(torch.int16) != want.view(torch.int16))[:, ok].nonzero()
            assert not len(bad), (m, rot, bad[:4].tolist())


def test_repeatable_and_routing():
    dev = gpu_device()
    assert NLF.plan(1024, 4096)[2] > 1
    x, wq, scale, b, r = _inputs(3, 1024, 4096, dev, 5)
    a, c = ops.linear_small_m_fp8(x, wq, scale, b, None, r), ops.linear_small_m_fp8(x, wq, scale, b, None, r)
    assert torch.equal(a.view(torch.int16), c.view(torch.int16))
    for m, k in ((17, 128), (4, 24)):   # M > 16 and K % 16 != 0: the documented composition, bitwise
        x, wq, scale, b, r = _inputs(m, 64, k, dev, 9)
        for epi in EPIS:
            bias, act, res = _args(b, r, epi)
            want = ops.linear(x, (wq.float() * scale[:, None]).to(x.dtype), bias, act, residual=res)
            assert torch.equal(ops.linear_small_m_fp8(x, wq, scale, bias, act, res).view(torch.int16), want.view(torch.int16))
    x, wq, scale, b, _ = _inputs(4, 64, 32, dev, 2)
    y = ops.linear_small_m_fp8(x.view(2, 2, 32), wq.view(torch.uint8), scale, b)
    assert y.shape == (2, 2, 64) and torch.equal(y.view(4, 64), ops.linear_small_m_fp8(x, wq, scale, b))
    with pytest.raises(RuntimeError, match="autograd"):
        ops.linear_small_m_fp8(x.clone().requires_grad_(True), wq, scale, b)


LENS, STEPS = [5, 8], 3


def _tiny(dev, **kw):
    torch.manual_seed(0)
    model = llama_tiny(**kw).eval().to(dev)
    cast_params(model, torch.bfloat16)
    return model


def _step_logits(model, prompts, forced, dev):
    ids = torch.zeros(len(LENS), max(LENS), dtype=torch.long)
    for b, r in enumerate(prompts):
        ids[b, :len(r)] = r
    cache = LlamaKVCache.allocate(model, len(LENS), max(LENS) + STEPS)
    out = [model.prefill(ids.to(dev), torch.tensor(LENS, dtype=torch.int32, device=dev), cache, chunk=8)]
    out += [model.decode_step(forced[:, t].to(dev), cache) for t in range(STEPS)]
    return torch.stack(out).float().cpu()


@pytest.mark.parametrize("kw", [dict(), dict(hidden_size=256)], ids=["D64", "D128"])
def test_quantised_step_logits_against_fp64_copy(kw):
    dev = gpu_device()
    model = _tiny(dev, **kw)
    g = torch.Generator().manual_seed(77)
    prompts = [torch.randint(0, 1000, (n,), generator=g) for n in LENS]
    forced = torch.randint(0, 1000, (len(LENS), STEPS), generator=g)
    plain = _step_logits(model, prompts, forced, dev)
    model.quantize_decode_weights()
    got = _step_logits(model, prompts, forced, dev)
    mode = _lib.mode()
    _lib.set_mode("off")                # the emulation arm: the same model through the reference ops
    try:
        em = _step_logits(model, prompts, forced, dev)
    finally:
        _lib.set_mode(mode)
    copy64 = copy.deepcopy(model).cpu().double()
    with torch.no_grad():
        for blk, src in zip(copy64.layers, model.layers):
            for name, (wq, scale) in src._fp8.items():
                getattr(blk, name).weight.copy_(wq.float().double().cpu() * scale.double().cpu()[:, None])
    fails = []
    for b, r in enumerate(prompts):
        ref = forward64(copy64, torch.cat([r, forced[b]]))[len(r) - 1:]
        check(fails, f"{kw} row {b}", got[:, b], ref, em[:, b])
    assert not fails, "\n".join(fails)
    model.float().bfloat16()            # a cast drops the pairs: the unquantised model's step, bitwise
    assert all(blk._fp8 is None for blk in model.layers)
    assert torch.equal(_step_logits(model, prompts, forced, dev), plain)


def test_quantising_rebuilds_the_graph_session():
    dev = gpu_device()
    # (untied head, larger weights: greedy tokens that move under quantisation, 24 of 48 with the CPU references)
    model = _tiny(dev, tie_word_embeddings=False, initializer_range=0.1)
    g = torch.Generator().manual_seed(78)
    prompts = [torch.randint(0, 1000, (65,), generator=g) for _ in range(2)]
    ids = torch.stack(prompts).to(dev)
    new = 24
    a = model.generate(ids, max_new_tokens=new, use_graph=True)
    first = model.decode_session
    model.quantize_decode_weights()
    b = model.generate(ids, max_new_tokens=new, use_graph=True)
    sess = model.decode_session
    assert sess is not first and sess.graph is not None
    with torch.no_grad():
        want = _eager_loop(model, prompts, new, dev, sess.capacity)
    assert torch.equal(b[:, 65:].cpu(), want) and not torch.equal(a, b)     # not a replay of the stale session
    model.clear_decode_weights()
    assert torch.equal(model.generate(ids, max_new_tokens=new, use_graph=True), a) and model.decode_session is not sess
