"""``ops.next_token`` / ``ops.decode_embed`` on the CPU (the reference ops), and the cases themselves: the
``run_*`` functions take a device and are what tests/test_next_token_gpu.py runs against the HIP kernel.

The oracle is fp64 on the CPU from the same bf16 logits: ``torch.argmax`` for greedy, and for sampling the
fp64 kept set (every column >= the k-th largest value) and the fp64 CDF of ``exp((x - max) * inv_t)`` over
it in index order, ``inv_t`` being the fp32 value the op is given.

Exact sampled tokens: the test builds each ``u`` as the midpoint of the fp64 CDF interval of a chosen token
and asserts ABOUT ITS OWN INPUTS that every such ``u`` is at least 1e-4 of the total mass away from both
ends of that interval (hence from every CDF boundary).  The kernel's prefix sums carry about
(V / 256 + 10) * 2^-24 of the total mass of accumulation error (per-thread runs of V / 1024 terms under a
tree), 1.2e-5 at V = 50257 and 2.2e-5 at V = 90001, plus fp32 ``exp`` and the rounding of ``u * W``, each
below 1e-6: the 1e-4 margin is 4x .. 8x that, so the exact token is required, with no tolerance.
V = 90001 is past what the kernel keeps in LDS: its other loader.
"""
import pytest
import torch

from databricks_distributed_deep_learning_amd import ops

U_MARGIN = 1e-4
U_LAST = 1.0 - 2.0 ** -24


def _logits(V, B, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * scale).bfloat16()


def _call(logits, dev, **kw):
    kw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}
    return ops.next_token(logits.to(dev), **kw).cpu()


# ------------------------------------------------------------------ greedy
def tie_rows(V):
    """(name, row): the planted-maximum patterns.  The kernel's thread t owns columns [t R, (t + 1) R) (up
    to an alignment shift below 8), R = (V + 7) / 1024 rounded up to a multiple of 8 (8 at V = 1000, 56 at
    V = 50257); a wave owns 64 threads' worth."""
    R = ((V + 7 + 1023) // 1024 + 7) // 8 * 8
    base = _logits(V, 1, 1000 + V, 1.0)[0].clamp(max=4.0)

    def plant(cols):
        r = base.clone()
        r[[min(c, V - 1) for c in cols]] = 9.0
        return r
    rows = [("max at 0", plant([0])), ("max at V-1", plant([V - 1])),
            ("two threads of one wave", plant([R + R // 2, 5 * R + 1])),
            ("two waves", plant([3 * R + 1, 64 * R + 3])), ("two far waves", plant([64 * R + 3, V - 2])),
            ("both ends", plant([0, V - 1])),
            ("all equal", torch.full((V,), 1.5).bfloat16())]
    r = torch.full((V,), float("-inf")).bfloat16()
    r[V // 2] = -3.0
    rows.append(("-inf but one", r))
    return rows


def run_greedy(V, dev):
    rows = tie_rows(V)
    for name, r in rows:                                            # B = 1
        assert int(_call(r[None], dev)[0]) == int(torch.argmax(r.float())), (V, name)
    for i in range(0, len(rows), 2):                                # B = 3: rows 1 and 2 start off a 16-byte line
        pick = [rows[(i + j) % len(rows)] for j in range(3)]
        x = torch.stack([r for _, r in pick])
        assert torch.equal(_call(x, dev), torch.argmax(x.float(), -1)), (V, [n for n, _ in pick])
    x = _logits(V, 3, 5)
    assert torch.equal(_call(x, dev), torch.argmax(x.float(), -1))
    # u given but the sample flag off: greedy
    prm = ops.next_token_params(0.5, 3, sample=False)
    assert torch.equal(_call(x, dev, u=torch.full((3,), 0.9), params=prm), torch.argmax(x.float(), -1))


@pytest.mark.parametrize("V", [7, 1000, 50257])
def test_greedy(V):
    run_greedy(V, torch.device("cpu"))


# ------------------------------------------------------------------ the fp64 oracle for sampling
def kept64(x, k):
    """x [V] bf16 -> bool [V]: every column >= the k-th largest value."""
    x = x.double()
    if k is None or k >= x.numel():
        return torch.ones_like(x, dtype=torch.bool)
    return x >= x.sort(descending=True).values[k - 1]


def cdf64(x, k, inv_t):
    """(kept, cdf): cdf[j] = the inclusive prefix mass at column j as a fraction of the total, fp64."""
    kept = kept64(x, k)
    xd = x.double()
    w = torch.where(kept, torch.exp((xd - xd.max()) * inv_t), torch.zeros_like(xd))
    c = w.cumsum(0)
    return kept, c / c[-1]


def _tie_row(V, k, seed):
    """A row where 5 columns tie at the k-th largest value (so the kept set has more than k members)."""
    x = _logits(V, 1, seed)[0]
    order = x.float().sort(descending=True, stable=True).indices
    kth = x[order[k - 1]].clone()
    g = torch.Generator().manual_seed(seed + 1)
    tail = order[k:][torch.randperm(V - k, generator=g)[:4]]
    x[tail] = kth
    return x


def run_top_k(V, dev):
    ks = sorted({1, 2, min(50, V), V - 1, V}) + [None]
    us = [0.0, 0.25, 0.5, 0.75, 0.999, U_LAST]
    for k in ks:
        rows = [_logits(V, 1, 7 + V)[0], _logits(V, 1, 8 + V)[0]]
        if k is not None and k + 4 <= V:
            rows.append(_tie_row(V, k, 9 + V))
            assert int(kept64(rows[-1], k).sum()) >= k + 4
        x = torch.stack(rows)
        kept = torch.stack([kept64(r, k) for r in rows])
        for uv in us:
            tok = _call(x, dev, u=torch.full((len(rows),), uv), inv_temperature=1.0 / 0.9, top_k=k)
            assert bool(kept[torch.arange(len(rows)), tok].all()), (V, k, uv, tok.tolist())
            if k == 1:      # the rows whose maximum is unique (on the tie row all 5 maxima are kept)
                one = kept.sum(1) == 1
                assert int(one.sum()) >= 2 and torch.equal(tok[one], torch.argmax(x.float(), -1)[one]), (V, uv)


@pytest.mark.parametrize("V", [7, 1000, 50257])
def test_top_k_kept_set(V):
    run_top_k(V, torch.device("cpu"))


def sampling_case(V, k, temperature, seed):
    """logits [2, V], inv_t (the fp32 value), u [5, 2] and the tokens wanted [4, 2]: per row the most likely
    token, the least likely kept one whose interval is wide enough, the lowest and the highest kept index;
    u's last row is 1 - 2^-24."""
    x = _logits(V, 2, seed)
    inv_t = float(torch.tensor(1.0 / temperature, dtype=torch.float32))
    for b in range(2):          # mass at both ends of the row, so that their intervals are wide enough
        x[b, 0] = x[b, V - 1] = (x[b].float().max() - 0.5).bfloat16()
    u, want, kepts = torch.zeros(5, 2), torch.zeros(4, 2, dtype=torch.long), []
    for b in range(2):
        kept, cdf = cdf64(x[b], k, inv_t)
        kepts.append(kept)
        lo = torch.cat([torch.zeros(1, dtype=torch.float64), cdf[:-1]])
        width = cdf - lo
        idx = kept.nonzero().squeeze(1)
        wide = idx[width[idx] >= 3 * U_MARGIN]
        toks = [idx[width[idx].argmax()], wide[width[wide].argmin()], idx[0], idx[-1]]
        for i, t in enumerate(toks):
            want[i, b] = t
            u[i, b] = float((lo[t] + cdf[t]) / 2)
            # a condition on the inputs, not a tolerance on the kernel
            assert u[i, b].double() - lo[t] >= U_MARGIN and cdf[t] - u[i, b].double() >= U_MARGIN, (V, k, b, i)
        u[4, b] = U_LAST
    return x, inv_t, u, want, torch.stack(kepts)


def run_sampling(V, k, temperature, dev):
    x, inv_t, u, want, kept = sampling_case(V, k, temperature, 31 + V)
    T = u.shape[0]
    step = torch.zeros(2, dtype=torch.int32)
    tokens_out = torch.full((2, T), -1, dtype=torch.long)
    xd, ud, sd, td = x.to(dev), u.to(dev), step.to(dev), tokens_out.to(dev)
    for _ in range(T):          # one launch per row of u, through the device step counter
        ops.next_token(xd, u=ud, inv_temperature=inv_t, top_k=k, step=sd, tokens_out=td)
    got = td.cpu().t()
    assert sd.tolist() == [T, T]
    assert torch.equal(got[:4], want), (V, k, temperature, got[:4].tolist(), want.tolist())
    assert bool(kept[torch.arange(2), got[4]].all())        # u = 1 - 2^-24 does not run off the end


@pytest.mark.parametrize("temperature", [0.7, 1.0, 1.5])
@pytest.mark.parametrize("V,k", [(1000, None), (1000, 50), (50257, None), (50257, 50), (90001, 50)])
def test_sampling_exact_token(V, k, temperature):
    run_sampling(V, k, temperature, torch.device("cpu"))


# ------------------------------------------------------------------ bookkeeping
CANARY = -7


def _guarded(n, dtype, fill=0):
    """(whole, middle): ``middle`` is n elements with 8 canaries on each side."""
    whole = torch.full((n + 16,), CANARY, dtype=torch.int64).to(dtype) if dtype != torch.bool else \
        torch.ones(n + 16, dtype=torch.bool)
    whole[8:8 + n] = fill
    return whole


def _canaries_ok(whole, n):
    edge = torch.cat([whole[:8], whole[8 + n:]])
    return bool(edge.all()) if whole.dtype == torch.bool else bool((edge == CANARY).all())


def run_bookkeeping(dev):
    B, V, T, eos, pad = 3, 1000, 4, 5, 9
    emit = torch.tensor([[3, 5, 7, 8], [1, 2, 3, 4], [5, 6, 7, 8]])         # what the logits say, per call
    want = torch.tensor([[3, 5, pad, pad], [1, 2, 3, 4], [5, pad, pad, pad]])
    want_done = torch.tensor([[0, 1, 1, 1], [0, 0, 0, 0], [1, 1, 1, 1]], dtype=torch.bool)   # after call t
    lens0 = [4, 17, 0]
    bufs = {"step": _guarded(B, torch.int32).to(dev), "done": _guarded(B, torch.bool, False).to(dev),
            "out": _guarded(B, torch.int64, -1).to(dev), "lens": _guarded(B, torch.int32).to(dev),
            "tokens_out": _guarded(B * T, torch.int64, -1).to(dev)}
    view = {k: v[8:8 + (B * T if k == "tokens_out" else B)] for k, v in bufs.items()}
    view["tokens_out"] = view["tokens_out"].view(B, T)
    view["lens"].copy_(torch.tensor(lens0, dtype=torch.int32))
    for t in range(T):
        x = _logits(V, B, 40 + t, 1.0)
        x[torch.arange(B), emit[:, t]] = 20.0
        tok = ops.next_token(x.to(dev), eos_token_id=eos, pad_token_id=pad, **view)
        assert tok.data_ptr() == view["out"].data_ptr()
        assert view["out"].tolist() == want[:, t].tolist(), t
        assert view["done"].tolist() == want_done[:, t].tolist(), t
        assert view["step"].tolist() == [t + 1] * B
        assert view["lens"].tolist() == [n + t + 1 for n in lens0]
        tk = view["tokens_out"].cpu()
        assert torch.equal(tk[:, :t + 1], want[:, :t + 1]) and bool((tk[:, t + 1:] == -1).all())
    for k, n in (("step", B), ("done", B), ("out", B), ("lens", B), ("tokens_out", B * T)):
        assert _canaries_ok(bufs[k].cpu(), n), k
    # a column past tokens_out's width is not written (the counter still advances)
    ops.next_token(x.to(dev), step=view["step"], tokens_out=view["tokens_out"])
    assert view["step"].tolist() == [T + 1] * B and _canaries_ok(bufs["tokens_out"].cpu(), B * T)
    assert torch.equal(view["tokens_out"].cpu(), want)
    # stand-alone: nothing but the returned tokens is written
    before = {k: v.clone() for k, v in bufs.items() if k != "out"}
    out = _guarded(B, torch.int64, -1).to(dev)
    ops.next_token(x.to(dev), out=out[8:8 + B])
    assert out[8:8 + B].tolist() == emit[:, T - 1].tolist() and _canaries_ok(out.cpu(), B)
    assert all(torch.equal(bufs[k], v) for k, v in before.items())
    assert ops.next_token(x.to(dev)).tolist() == emit[:, T - 1].tolist()


def test_bookkeeping():
    run_bookkeeping(torch.device("cpu"))


# ------------------------------------------------------------------ decode_embed, guards
def run_decode_embed(E, B, dev, V=1000, P=128):
    g = torch.Generator().manual_seed(E + B)
    wte, wpe = torch.randn(V, E, generator=g).bfloat16(), torch.randn(P, E, generator=g).bfloat16()
    tok, lens = torch.randint(0, V, (B,), generator=g), torch.randint(0, P, (B,), generator=g).int()
    for t_edge, n_edge in ((0, 0), (V - 1, P - 1), (0, P - 1)):
        tok[0], lens[0] = t_edge, n_edge
        tok[-1], lens[-1] = V - 1 - t_edge, P - 1 - n_edge
        got = ops.decode_embed(tok.to(dev), lens.to(dev), wte.to(dev), wpe.to(dev)).cpu()
        want = (wte[tok].float() + wpe[lens.long()].float()).bfloat16()
        assert got.dtype == torch.bfloat16 and torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("E,B", [(128, 1), (768, 16)])
def test_decode_embed_reference(E, B):
    run_decode_embed(E, B, torch.device("cpu"))
    # fp32 tables: the plain sum
    wte, wpe = torch.randn(10, 8), torch.randn(4, 8)
    tok, lens = torch.tensor([9, 0]), torch.tensor([0, 3], dtype=torch.int32)
    assert torch.equal(ops.decode_embed(tok, lens, wte, wpe), wte[tok] + wpe[lens.long()])


def test_argument_guards():
    x = torch.randn(2, 10)
    with pytest.raises(ValueError, match="top_k"):
        ops.next_token(x, u=torch.rand(2), top_k=0)
    with pytest.raises(ValueError, match="inv_temperature"):
        ops.next_token(x, u=torch.rand(2), inv_temperature=0.0)
    with pytest.raises(ValueError, match="u must be"):
        ops.next_token(x, u=torch.rand(3))
    with pytest.raises(ValueError, match="step must be"):
        ops.next_token(x, step=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="tokens_out"):
        ops.next_token(x, tokens_out=torch.zeros(3, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="logits"):
        ops.next_token(torch.randn(10))
    with pytest.raises(ValueError, match="decode_embed"):
        ops.decode_embed(torch.zeros(2, dtype=torch.long), torch.zeros(3, dtype=torch.int32), torch.randn(4, 8),
                         torch.randn(4, 8))
