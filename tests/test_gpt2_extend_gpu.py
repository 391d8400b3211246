"""GPT-2 ``extend`` and ``generate(prefix=..., prefill_chunk=...)`` on the GPU (gpt2_tiny, bf16, native kernels)
against an fp64 copy of the model.

B = 2 with prompt lengths {5, 65}: prefill, then ``extend`` of T = 16 columns with ``new_lens`` (16, 3), then
``extend`` of one column (B T <= 16: the weight-streaming linears), then one decode step -- teacher-forced on a
fixed token sequence.  The fp64 copy (`forward64` of tests/test_gpt2_generate_gpu.py) is plain torch on the CPU
from the model's bf16 weights, each sequence alone and unpadded.

Logits: each call's ``[B, vocab]`` logits, and the ``all_logits=True`` rows of the real columns of the T = 16
call, are bounded in the form of tests/test_attention_edges_gpu.py (`check`, M = 2, max and rms) by M x the error
of the EXISTING native full ``forward`` at the same positions against the same fp64 copy, plus half a bf16 ulp:
the yardstick is the training-time forward path, not the code under test.

Greedy tokens, on the model with the token embedding scaled by 5 (see tests/test_gpt2_generate_gpu.py: no token
hinges on rounding; asserted as top-2 gap > 20 x the measured logit error): ``generate`` with a batch-1 prefix
cache shared by both rows, and with ``prefill_chunk=16``, equals plain ``generate`` on the concatenated prompt
and the fp64 greedy continuation, eagerly and from the graph session, which captures nothing on a second call
of the same shape; the prefix cache is bitwise unchanged.

Measured on an MI355X: against the native forward's error as the yardstick, with the ulp term subtracted the
largest ratios are 0.057 (max form; all_logits, row 0) and 0.249 (rms form; the same rows; 0.247 for the T = 16
extend); as plain error / forward error 1.08 (max; the T = 1 extend) and 1.03 (rms; the T = 16 extend), so M = 2
holds as it stands.  The largest logit error is 2.66e-2 and the smallest fp64 top-2 gap 8.51: 320 x.
"""
import math

import pytest
import torch

from conftest import gpu_device
from test_attention_edges_gpu import M, check  # noqa: F401
from test_gpt2_generate_gpu import _model, forward64

from databricks_distributed_deep_learning_amd.models import KVCache

pytestmark = pytest.mark.gpu

LENS = [5, 65]
T, NEW = 16, [16, 3]
STEPS = 5
_cache = {}


def _tokens():
    g = torch.Generator().manual_seed(78)
    prompts = [torch.randint(0, 1000, (n,), generator=g) for n in LENS]
    chunk = torch.randint(0, 1000, (len(LENS), T), generator=g)
    one = torch.randint(0, 1000, (len(LENS), 2), generator=g)       # the T = 1 extend's token, the decode step's
    return prompts, chunk, one


def _shared(dev):
    """Computed once: the logits of the four calls and the all_logits rows, with the fp64 copy's and the existing
    native forward's at the same positions."""
    if "r" not in _cache:
        model = _model(dev)
        prompts, chunk, one = _tokens()
        S = max(LENS)
        ids = torch.zeros(len(LENS), S, dtype=torch.long)
        for b, r in enumerate(prompts):
            ids[b, :len(r)] = r
        cache = KVCache.allocate(model, len(LENS), S + T + 2)
        nl = torch.tensor(NEW, dtype=torch.int32, device=dev)
        got = [model.prefill(ids.to(dev), torch.tensor(LENS, dtype=torch.int32, device=dev), cache)]
        snap = (cache.data.clone(), cache.lens.clone(), cache.max_len)
        rows_all = model.extend(chunk.to(dev), cache, nl, all_logits=True).float().cpu()
        cache.data.copy_(snap[0]), cache.lens.copy_(snap[1])
        cache.max_len = snap[2]
        got.append(model.extend(chunk.to(dev), cache, nl))
        assert cache.lens.tolist() == [n + t for n, t in zip(LENS, NEW)] and cache.max_len == S + T
        got.append(model.extend(one[:, :1].to(dev), cache))
        got.append(model.decode_step(one[:, 1].to(dev), cache))
        assert cache.lens.tolist() == [n + t + 2 for n, t in zip(LENS, NEW)]
        got = torch.stack(got).float().cpu()                        # [4, B, V]
        ref, fwd, ref_all, fwd_all = [], [], [], []
        with torch.no_grad():
            for b, r in enumerate(prompts):
                n, t = len(r), NEW[b]
                full = torch.cat([r, chunk[b, :t], one[b]])
                at = torch.tensor([n - 1, n + t - 1, n + t, n + t + 1])
                r64, f = forward64(model.state_dict(), full), model(full[None].to(dev))[0].float().cpu()
                ref.append(r64[at]), fwd.append(f[at])
                ref_all.append(r64[n:n + t]), fwd_all.append(f[n:n + t])
        _cache["r"] = (model, got, torch.stack(ref, 1), torch.stack(fwd, 1), rows_all, ref_all, fwd_all)
    return _cache["r"]


def test_step_logits_against_fp64_copy():
    dev = gpu_device()
    _, got, ref, fwd, _, _, _ = _shared(dev)
    fails = []
    for i, name in enumerate(("prefill", "extend T=16 (16, 3)", "extend T=1", "decode step")):
        check(fails, f"{name} logits", got[i], ref[i], fwd[i])
    assert not fails, "\n".join(fails)


def test_all_logits_rows():
    dev = gpu_device()
    _, got, _, _, rows_all, ref_all, fwd_all = _shared(dev)
    fails = []
    for b, t in enumerate(NEW):
        check(fails, f"all_logits row {b}", rows_all[b, :t], ref_all[b], fwd_all[b])
        # the last real column is the [B, V] result (another GEMM kernel: not bitwise)
        torch.testing.assert_close(rows_all[b, t - 1], got[1, b], rtol=2.0 ** -6, atol=2.0 ** -4)
    assert not fails, "\n".join(fails)


def _padded(seqs, left):
    S = max(len(t) for t in seqs)
    ids, mask = torch.zeros(len(seqs), S, dtype=torch.long), torch.zeros(len(seqs), S, dtype=torch.long)
    for b, t in enumerate(seqs):
        sl = slice(S - len(t), S) if left else slice(0, len(t))
        ids[b, sl], mask[b, sl] = t, 1
    return ids, mask


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_greedy_generate_with_prefix_and_chunks(use_graph):
    dev = gpu_device()
    model, got, ref = _shared(dev)[:3]
    err = (got.double() - ref).abs().max().item()
    g = torch.Generator().manual_seed(79)
    head = torch.randint(0, 1000, (7,), generator=g)
    tails = [torch.randint(0, 1000, (n,), generator=g) for n in (40, 9)]
    whole = [torch.cat([head, t]) for t in tails]
    sd = model.state_dict()
    want, gap = [], math.inf
    for r in whole:             # the fp64 greedy continuation and its smallest top-2 gap
        seq = r.clone()
        for _ in range(STEPS):
            lg = forward64(sd, seq)[-1]
            top = lg.topk(2).values
            gap = min(gap, (top[0] - top[1]).item())
            seq = torch.cat([seq, lg.argmax()[None]])
        want.append(seq[len(r):])
    want = torch.stack(want)
    print(f"measured logit error {err:.4e}, smallest fp64 top-2 gap {gap:.4e} ({gap / err:.1f} x)")
    assert gap > 20 * err

    prefix = KVCache.allocate(model, 1, 7)
    model.prefill(head[None].to(dev), torch.tensor([7], dtype=torch.int32, device=dev), prefix)
    before, lens_before = prefix.data.clone(), prefix.lens.clone()
    wids, wmask = _padded(whole, True)
    plain = model.generate(wids.to(dev), attention_mask=wmask.to(dev), max_new_tokens=STEPS)
    assert torch.equal(plain[:, wids.shape[1]:].cpu(), want)
    for left in (False, True):
        ids, mask = _padded(tails, left)
        for kw in (dict(prefix=prefix), dict(prefix=prefix, prefill_chunk=16)):
            out = model.generate(ids.to(dev), attention_mask=mask.to(dev), max_new_tokens=STEPS, use_graph=use_graph,
                                 **kw)
            assert torch.equal(out[:, :ids.shape[1]].cpu(), ids) and torch.equal(out[:, ids.shape[1]:].cpu(), want), kw
    assert torch.equal(prefix.data.view(torch.int16), before.view(torch.int16))
    assert torch.equal(prefix.lens, lens_before) and prefix.max_len == 7
    for left in (False, True):
        ids, mask = _padded(whole, left)
        out = model.generate(ids.to(dev), attention_mask=mask.to(dev), max_new_tokens=STEPS, use_graph=use_graph,
                             prefill_chunk=16)
        assert torch.equal(out[:, ids.shape[1]:].cpu(), want)
    if use_graph:
        sess = model.decode_session
        n = sess.captures
        assert sess.graph is not None and n >= 1
        ids, mask = _padded(tails, True)
        model.generate(ids.to(dev), attention_mask=mask.to(dev), max_new_tokens=STEPS, use_graph=True, prefix=prefix)
        assert model.decode_session is sess and sess.captures == n


def test_value_errors():
    dev = gpu_device()
    model = _shared(dev)[0]
    c = KVCache.allocate(model, 1, 12)
    with pytest.raises(ValueError, match="capacity"):
        model.extend(torch.zeros(1, 13, dtype=torch.long, device=dev), c)
    with pytest.raises(ValueError, match="n_positions"):
        model.generate(torch.zeros(1, 100, dtype=torch.long, device=dev), max_new_tokens=29, prefill_chunk=16)
