"""``ops.next_token`` with ``top_p``, ``min_p`` and ``repetition_penalty``, and ``generate`` with them, on the
CPU (the reference ops); the ``run_*`` functions take a device and are what tests/test_sampling_gpu.py runs
against the HIP kernel (``ddl_next_token_ex``).

The oracle is fp64 on the CPU from the same bf16 logits, by value and without the op's code: the top-k set
(``kept64``), then per distinct value the cumulative mass ``S(v)`` of the values >= v as a fraction of the
top-k mass: a column stays under top-p iff the mass strictly above its value is < p; under min-p iff
``(x - max) * inv_t >= log(m)``.

Exact equality with no tolerance, by margins asserted ABOUT THE INPUTS: the kernel's sums carry <= ~2.2e-5 of
the total mass at V = 90001 (tests/test_next_token_cpu.py), so every ``p`` is the midpoint of two consecutive
``S`` at least 4e-4 apart (>= 2e-4 on either side, 8x the budget), every ``log(m)`` is at least 1e-3 from every
column's ``(x - max) * inv_t`` (fp32 rounding of that product is below 1e-5 here), and every ``u`` is at least
``U_MARGIN`` inside its token's fp64 CDF interval.  Rows 1 and 2 of a batch are the first row rolled and
reversed: the same values, so the same ``S``, at other columns and (odd V) off a 16-byte line.
"""
import math

import pytest
import torch

from test_next_token_cpu import U_LAST, U_MARGIN, _call, _logits, kept64

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.ops.decode import sampling_kept

CPU = torch.device("cpu")
P_GAP = 4e-4
M_GAP = 1e-3


def f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def run_of(V):
    """Columns per kernel thread (see tests/test_next_token_cpu.py ``tie_rows``); a wave owns 64 of them."""
    return ((V + 7 + 1023) // 1024 + 7) // 8 * 8


def batch_of(row, B):
    return torch.stack([row, row.roll(1), row.flip(0)][:B])


# ------------------------------------------------------------------ the fp64 oracle
def masses(x, k, inv_t):
    """(values descending, S): the distinct values of the top-k set and the mass of the columns >= each, as a
    fraction of the set's mass."""
    kept = kept64(x, k)
    xd = x.double()
    vals, inv = torch.unique(xd[kept], return_inverse=True)
    m = torch.zeros_like(vals).index_add_(0, inv, torch.exp((xd[kept] - xd.max()) * inv_t))
    vals, m = vals.flip(0), m.flip(0)
    return vals, m.cumsum(0) / m.sum()


def kept_oracle(x, inv_t, k=None, p=None, m=None):
    kept = kept64(x, k)
    xd = x.double()
    if p is not None and p < 1.0:
        vals, S = masses(x, k, inv_t)
        above = torch.cat([torch.zeros(1, dtype=torch.float64), S[:-1]])
        kept = kept & (xd >= vals[above < p].min())
    if m:
        kept = kept & ((xd - xd.max()) * inv_t >= math.log(m))
    return kept


def cdf_of(x, kept, inv_t):
    xd = x.double()
    c = torch.where(kept, torch.exp((xd - xd.max()) * inv_t), torch.zeros_like(xd)).cumsum(0)
    return c / c[-1]


def choose_p(x, k, inv_t, target):
    """The fp32 p nearest ``target`` among the midpoints of consecutive ``S`` (0 first) at least P_GAP apart."""
    _, S = masses(x, k, inv_t)
    S = torch.cat([torch.zeros(1, dtype=torch.float64), S])
    mid = ((S[:-1] + S[1:]) / 2)[(S[1:] - S[:-1]) >= P_GAP]
    p = f32(mid[(mid - target).abs().argmin()])
    assert 0 < p < 1 and float((S - p).abs().min()) >= P_GAP / 2 - 1e-7, (p, target)    # about the inputs
    return p


def choose_m(x, inv_t, target):
    """The fp32 m nearest ``target`` whose log is at least M_GAP from every column's ``(x - max) * inv_t``."""
    xd = x.double()
    d = torch.unique((xd - xd.max()) * inv_t)
    d = d[torch.isfinite(d)]
    ok = (d[1:] - d[:-1]) >= 2.5 * M_GAP
    mid = ((d[1:] + d[:-1]) / 2)[ok]
    m = f32(math.exp(float(mid[(mid - math.log(target)).abs().argmin()])))
    assert 0 < m < 1 and float((d - math.log(m)).abs().min()) >= M_GAP, (m, target)     # about the inputs
    return m


def check_tokens(x, kepts, inv_t, dev, what, **kw):
    """x [B, V], kepts [B, V] (the oracle's): the lowest kept column at u = 0, membership at u in {0.999,
    U_LAST}, the exact token at the midpoint of four tokens' CDF intervals (the widest, the narrowest wide
    enough, the lowest and the highest wide enough), and the same tokens from a second call."""
    B = x.shape[0]
    rows = torch.arange(B)
    us = [torch.full((B,), 0.0), torch.full((B,), 0.999), torch.full((B,), U_LAST)]
    want = [torch.stack([k.nonzero()[0, 0] for k in kepts]), None, None]
    picks = [[], [], [], []]
    for b in range(B):
        cdf = cdf_of(x[b], kepts[b], inv_t)
        lo = torch.cat([torch.zeros(1, dtype=torch.float64), cdf[:-1]])
        width = cdf - lo
        wide = (kepts[b] & (width >= 3 * U_MARGIN)).nonzero().squeeze(1)
        assert wide.numel() >= 1, what
        for i, t in enumerate([wide[width[wide].argmax()], wide[width[wide].argmin()], wide[0], wide[-1]]):
            uv = f32((lo[t] + cdf[t]) / 2)
            assert uv - lo[t] >= U_MARGIN and cdf[t] - uv >= U_MARGIN, (what, b, i)     # about the inputs
            picks[i].append((uv, t))
    for pk in picks:
        us.append(torch.tensor([uv for uv, _ in pk]))
        want.append(torch.stack([t for _, t in pk]))
    for uv, w in zip(us, want):
        tok = _call(x, dev, u=uv, **kw)
        assert bool(kepts[rows, tok].all()), (what, uv.tolist(), tok.tolist())
        if w is not None:
            assert torch.equal(tok, w), (what, uv.tolist(), tok.tolist(), w.tolist())
        assert torch.equal(_call(x, dev, u=uv, **kw), tok), what       # repeatable


# ------------------------------------------------------------------ top-p
def run_top_p(V, B, temperature, k, target, dev):
    row = _logits(V, 1, 7 + V)[0]
    inv_t = f32(1.0 / temperature)
    p = choose_p(row, k, inv_t, target)
    x = batch_of(row, B)
    kepts = torch.stack([kept_oracle(r, inv_t, k, p) for r in x])
    assert 1 <= int(kepts[0].sum()) < (V if k is None else min(k, V))
    check_tokens(x, kepts, inv_t, dev, (V, B, temperature, k, p), inv_temperature=inv_t, top_k=k, top_p=p)


TOP_P_CASES = [(V, 3, t, None, p) for V in (7, 1000, 50257, 90001) for t in (0.7, 1.0) for p in (0.05, 0.5, 0.9)] + \
    [(V, 1, 1.0, None, 0.5) for V in (7, 1000, 50257, 90001)] + \
    [(V, 3, 1.5, 50, p) for V in (1000, 50257, 90001) for p in (0.5, 0.9)] + [(50257, 3, 1.5, None, 0.04)]


@pytest.mark.parametrize("V,B,temperature,k,target", TOP_P_CASES)
def test_top_p(V, B, temperature, k, target):
    run_top_p(V, B, temperature, k, target, CPU)


def run_top_p_edges(V, dev):
    """Five columns equal at the cut value, on different threads and waves: all kept.  p = 1: the call
    without top_p.  A p below the maximum's own share: the argmax for every u."""
    R = run_of(V)
    inv_t = f32(1.0 / 0.7)
    row = _logits(V, 1, 7 + V)[0]
    order = row.float().sort(descending=True, stable=True).indices
    cut = row[order[12]].clone()
    cols = [c % V for c in (3 * R + 1, 5 * R + 2, 64 * R + 3, 130 * R + 5)]
    assert len(set(cols) | {int(order[12])}) == 5 and not (set(cols) & set(order[:12].tolist()))
    row[cols] = cut
    vals, S = masses(row, None, inv_t)
    i = int((vals == cut.double()).nonzero()[0, 0])
    assert i >= 1 and float(S[i] - S[i - 1]) >= P_GAP
    p = f32((S[i] + S[i - 1]) / 2)
    x = batch_of(row, 3)
    kepts = torch.stack([kept_oracle(r, inv_t, None, p) for r in x])
    assert all(int((r == cut).sum()) >= 5 and bool(k[r == cut].all()) for k, r in zip(kepts, x))
    check_tokens(x, kepts, inv_t, dev, (V, "ties"), inv_temperature=inv_t, top_p=p)

    x = batch_of(_logits(V, 1, 8 + V)[0], 3)
    _, S = masses(x[0], None, inv_t)
    assert float(S[0]) >= 2 * P_GAP          # the maximum's share; p is half of it
    for uv in (0.0, 0.3, 0.8, U_LAST):
        u = torch.full((3,), uv)
        plain = _call(x, dev, u=u, inv_temperature=inv_t, top_k=40)
        assert torch.equal(_call(x, dev, u=u, inv_temperature=inv_t, top_k=40, top_p=1.0), plain), (V, uv)
        assert torch.equal(_call(x, dev, u=u, inv_temperature=inv_t, top_k=40, min_p=0.0), plain), (V, uv)
        assert torch.equal(_call(x, dev, u=u, inv_temperature=inv_t, top_k=40, repetition_penalty=1.0,
                                 history=torch.arange(6).view(3, 2) % V), plain), (V, uv)
        assert torch.equal(_call(x, dev, u=u, inv_temperature=inv_t, top_p=f32(float(S[0]) / 2)),
                           torch.argmax(x.float(), -1)), (V, uv)


@pytest.mark.parametrize("V", [1000, 50257, 90001])
def test_top_p_edges(V):
    run_top_p_edges(V, CPU)


# ------------------------------------------------------------------ min-p
def run_min_p(V, B, temperature, dev):
    row = _logits(V, 1, 7 + V)[0]
    inv_t = f32(1.0 / temperature)
    x = batch_of(row, B)
    for target in (0.3, 0.02):
        m = choose_m(row, inv_t, target)
        kepts = torch.stack([kept_oracle(r, inv_t, None, None, m) for r in x])
        assert 1 <= int(kepts[0].sum()) < V
        check_tokens(x, kepts, inv_t, dev, (V, B, temperature, m), inv_temperature=inv_t, min_p=m)
    # with top-k and top-p: the intersection (m cuts inside the top-k set, p inside what m leaves or not)
    k = min(50, V - 1)
    m = choose_m(row, inv_t, 0.05)
    for target in (0.5, 0.9):
        p = choose_p(row, k, inv_t, target)
        kepts = torch.stack([kept_oracle(r, inv_t, k, p, m) for r in x])
        both = torch.stack([kept_oracle(r, inv_t, k, p) & kept_oracle(r, inv_t, None, None, m) for r in x])
        assert torch.equal(kepts, both)
        check_tokens(x, kepts, inv_t, dev, (V, B, temperature, k, p, m), inv_temperature=inv_t, top_k=k, top_p=p,
                     min_p=m)


@pytest.mark.parametrize("V,B,temperature", [(7, 3, 1.0), (1000, 3, 0.7), (1000, 1, 1.5), (50257, 3, 1.0),
                                             (90001, 3, 0.7)])
def test_min_p(V, B, temperature):
    run_min_p(V, B, temperature, CPU)


@pytest.mark.parametrize("V", [7, 1000, 50257])
def test_reference_kept_set_is_the_oracles(V):
    row = _logits(V, 1, 7 + V)[0]
    inv_t = f32(1.0 / 0.7)
    k = min(50, V - 1)
    p, m = choose_p(row, k, inv_t, 0.9), choose_m(row, inv_t, 0.05)
    x = batch_of(row, 3)
    for kw in (dict(top_p=p), dict(top_k=k, top_p=p), dict(min_p=m), dict(top_k=k, top_p=p, min_p=m)):
        want = torch.stack([kept_oracle(r, inv_t, kw.get("top_k"), kw.get("top_p"), kw.get("min_p")) for r in x])
        assert torch.equal(sampling_kept(x.float(), inv_t, **kw), want), kw


# ------------------------------------------------------------------ repetition penalty
def penalised(row, ids, r):
    """The oracle's penalised row: fp32 from the original logit, one rounding to bf16, each id once."""
    out = row.clone()
    rt = torch.tensor(r, dtype=torch.float32)
    for j in {int(i) for i in ids if 0 <= int(i) < row.numel()}:
        v = row[j].float()
        out[j] = (v / rt if v > 0 else v * rt).bfloat16()
    return out


def run_penalty_greedy(V, dev):
    R = run_of(V)
    a, b2, c, d = ([1, 2, 3, 4] if V < 100 else [R + R // 2, 5 * R + 1, 64 * R + 3, (130 * R + 5) % V])
    base = _logits(V, 1, 1000 + V, 1.0)[0].clamp(max=4.0)
    row = base.clone()
    row[[a, b2, c, d]] = torch.tensor([9.0, 8.5, 8.0, 7.0]).bfloat16()
    x = batch_of(row, 3)
    col = [torch.tensor([j, (j + 1) % V, V - 1 - j]) for j in (a, b2, c, d)]    # where each plant sits per row
    Lh, To = 6, 4

    def call(hist=None, hl=None, gen=None, st=None, r=2.0, xx=x):
        kw = dict(repetition_penalty=r)
        if hist is not None:
            kw.update(history=hist, history_lens=hl)
        if gen is not None:
            kw.update(tokens_out=gen.clone(), step=None if st is None else st.clone())
        return _call(xx, dev, **kw)

    lens = lambda n: torch.full((3,), n, dtype=torch.int32)                     # noqa: E731
    fill = lambda cols, L: torch.stack(cols, 1)[:, [i % len(cols) for i in range(L)]].contiguous()   # noqa: E731
    # nothing counts: empty history, step 0, with the argmax planted in both -> it survives
    assert torch.equal(call(fill([col[0]], Lh), lens(0), fill([col[0]], To), lens(0)), col[0])
    # entries past history_lens / at columns >= step do not count either
    assert torch.equal(call(fill([col[1], col[0], col[0]], Lh), lens(1), fill([col[2], col[0]], To), lens(1)), col[0])
    # duplicates of one id: penalised once (9 / 2 = 4.5 stays above the row's 4.0; twice would not)
    hist = fill([col[0]], Lh)
    got = call(hist, lens(Lh), xx=batch_of(torch.where(torch.arange(V) == a, row, base), 3))
    assert torch.equal(got, col[0])
    # the penalised argmax loses to the runner-up; ids on two threads of a wave, on two waves; prompt-only,
    # generated-only, both; an id < 0 and ids >= V mixed in
    assert torch.equal(call(hist, lens(Lh)), col[1])
    assert torch.equal(call(fill([col[0], col[1]], Lh), lens(Lh)), col[2])
    assert torch.equal(call(fill([col[0], col[1], col[2]], Lh), lens(3)), col[3])
    assert torch.equal(call(None, None, fill([col[0], col[1]], To), lens(2)), col[2])
    assert torch.equal(call(fill([col[0]], Lh), lens(2), fill([col[1], col[2]], To), lens(2)), col[3])
    junk = fill([col[0], torch.full((3,), -1), torch.full((3,), V), col[1], torch.full((3,), 2 ** 40)], Lh)
    assert torch.equal(call(junk, lens(Lh)), col[2])
    # tokens_out without step: only the history counts
    assert torch.equal(call(hist, lens(Lh), fill([col[1]], To), None), col[1])
    # r = 1: the plain call; r < 1 rewards
    assert torch.equal(call(hist, lens(Lh), r=1.0), col[0])
    assert torch.equal(call(fill([col[3]], Lh), lens(Lh), r=0.5), col[3])
    # a negative maximum: the multiply branch (-1 * 2 = -2 < -1.5)
    neg = (-base.float().abs() - 3.0).bfloat16()
    neg[[a, b2]] = torch.tensor([-1.0, -1.5]).bfloat16()
    assert torch.equal(call(hist, lens(Lh), xx=batch_of(neg, 3)), col[1])
    assert torch.equal(call(fill([col[0], col[1]], Lh), lens(Lh), xx=batch_of(neg, 3), r=1.2), col[0])


def run_penalty_value(V, dev):
    """The penalised value, bit for bit: column A (penalised) wins the argmax against a later column holding
    exactly ``(x / r).to(bf16)`` (ties go to the lower index) and loses against the next bf16 above it."""
    r = 1.3
    rt = torch.tensor(r, dtype=torch.float32)
    A, O = (1, 3) if V < 100 else (run_of(V) + 3, 70 * run_of(V) + 1)
    for v in (7.53125, 3.015625, 100.5, -0.7578125, -12.0625):
        xa = torch.tensor(v).bfloat16()
        assert float(xa) == v
        y = (xa.float() / rt if v > 0 else xa.float() * rt).bfloat16()
        up = (y.view(torch.int16) + (1 if v > 0 else -1)).view(torch.bfloat16)      # the next bf16 above y
        assert float(up) > float(y)
        for other, want in ((y, A), (up, O)):
            row = torch.full((V,), -50.0).bfloat16()
            row[A], row[O] = xa, other
            x = torch.stack([row, row.roll(1), row.roll(3)])
            got = _call(x, dev, repetition_penalty=r, history=torch.tensor([[A], [A + 1], [A + 3]]))
            assert got.tolist() == [want, want + 1, want + 3], (V, v, float(other))


def run_penalty_sampled(V, dev):
    row = _logits(V, 1, 7 + V)[0]
    inv_t = f32(1.0 / 0.7)
    k = min(50, V - 1)
    top = row.float().topk(min(5, V)).indices
    r = 1.5
    x = batch_of(row, 3)
    hist = torch.stack([top, (top + 1) % V, V - 1 - top]).contiguous()      # each row's own top columns
    gen = hist[:, :2].flip(1).contiguous()
    pen = torch.stack([penalised(x[b], hist[b, :3].tolist() + gen[b, :1].tolist(), r) for b in range(3)])
    assert not torch.equal(pen, x)
    p = choose_p(pen[0], k, inv_t, 0.9)
    kepts = torch.stack([kept_oracle(q, inv_t, k, p) for q in pen])
    for q in pen[1:]:       # (the penalised rows hold the same values, so one p serves them)
        assert torch.equal(q.float().sort().values, pen[0].float().sort().values)
    check_tokens(pen, kepts, inv_t, dev, (V, "already penalised"), inv_temperature=inv_t, top_k=k, top_p=p)
    B = 3
    u = torch.tensor([0.0, 0.35, 0.7, U_LAST])
    for uv in u:
        uu = torch.full((B,), float(uv))
        want = _call(pen, dev, u=uu, inv_temperature=inv_t, top_k=k, top_p=p)
        kw = dict(u=uu, inv_temperature=inv_t, top_k=k, top_p=p, repetition_penalty=r, history=hist,
                  history_lens=torch.full((B,), 3, dtype=torch.int32))
        got = _call(x, dev, tokens_out=gen.clone(), step=torch.ones(B, dtype=torch.int32), **kw)
        assert torch.equal(got, want), (V, float(uv))
        assert torch.equal(_call(x, dev, tokens_out=gen.clone(), step=torch.ones(B, dtype=torch.int32), **kw), got)


@pytest.mark.parametrize("V", [7, 1000, 50257, 90001])
def test_penalty(V):
    run_penalty_greedy(V, CPU)
    run_penalty_value(V, CPU)
    run_penalty_sampled(V, CPU)


# ------------------------------------------------------------------ the old path, the bookkeeping
def run_unchanged_and_bookkeeping(dev):
    V, B = 1000, 3
    x = _logits(V, B, 5)
    for uv in (0.0, 0.4, 0.9):
        u = torch.full((B,), uv)
        want = _call(x, dev, u=u, inv_temperature=1.25, top_k=20)
        p5 = ops.next_token_params(1.25, 20)
        p8 = ops.next_token_params(1.25, 20, top_p=1.0)
        assert p5.shape == (5,) and p8.shape == (8,) and torch.equal(p8[:5], p5)
        assert torch.equal(_call(x, dev, u=u, params=p5), want) and torch.equal(_call(x, dev, u=u, params=p8), want)
    # the state, with the new settings on: row 0 emits eos at its second call, row 2 at once
    T, eos, pad = 4, 5, 9
    emit = torch.tensor([[3, 5, 7, 8], [1, 2, 3, 4], [5, 6, 7, 8]])
    want = torch.tensor([[3, 5, pad, pad], [1, 2, 3, 4], [5, pad, pad, pad]])
    prm = ops.next_token_params(1.0, 10, eos, pad, top_p=0.5, min_p=0.1, repetition_penalty=1.2).to(dev)
    st = {"step": torch.zeros(B, dtype=torch.int32), "done": torch.zeros(B, dtype=torch.bool),
          "out": torch.full((B,), -1), "lens": torch.tensor([4, 17, 0], dtype=torch.int32),
          "tokens_out": torch.full((B, T), -1)}
    st = {k: v.to(dev) for k, v in st.items()}
    hist = torch.tensor([[900], [901], [902]]).to(dev)
    for t in range(T):
        xt = _logits(V, B, 40 + t, 1.0)
        xt[torch.arange(B), emit[:, t]] = 30.0          # (30 / 1.2 still holds all but e^-20 of the mass)
        tok = ops.next_token(xt.to(dev), u=torch.full((B,), 0.5).to(dev), params=prm, history=hist, **st)
        assert tok.data_ptr() == st["out"].data_ptr() and st["out"].tolist() == want[:, t].tolist(), t
        assert st["step"].tolist() == [t + 1] * B and st["lens"].tolist() == [4 + t + 1, 17 + t + 1, t + 1]
        tk = st["tokens_out"].cpu()
        assert torch.equal(tk[:, :t + 1], want[:, :t + 1]) and bool((tk[:, t + 1:] == -1).all())
    assert st["done"].tolist() == [True, False, True]


def test_unchanged_and_bookkeeping():
    run_unchanged_and_bookkeeping(CPU)


def test_argument_guards():
    x, u = torch.randn(2, 10), torch.rand(2)
    for kw, msg in ((dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"), (dict(min_p=-0.1), "min_p"),
                    (dict(min_p=1.0), "min_p"), (dict(repetition_penalty=0.0), "repetition_penalty"),
                    (dict(history=torch.zeros(2, 3, dtype=torch.int32)), "history must be"),
                    (dict(history=torch.zeros(3, 3, dtype=torch.long)), "history must be"),
                    (dict(history=torch.zeros(2, 3, dtype=torch.long), history_lens=torch.zeros(2)), "history_lens"),
                    (dict(history_lens=torch.zeros(2, dtype=torch.int32)), "history_lens"),
                    (dict(params=torch.zeros(6, dtype=torch.int32)), "params must be")):
        with pytest.raises(ValueError, match=msg):
            ops.next_token(x, u=u, **kw)


# ------------------------------------------------------------------ the models
def model_cases():
    from test_gpt2_generate_cpu import _model as gpt2_model, _prompts
    from test_llama_generate_cpu import _model as llama_model
    return [("gpt2", gpt2_model, _prompts), ("llama", llama_model, _prompts)]


@pytest.mark.parametrize("family", [0, 1])
def test_generate_with_the_new_settings(family):
    name, make, prompts = model_cases()[family]
    model = make(0)
    ids, mask, rows = prompts(1, "left")
    S, NEW = ids.shape[1], 8
    base = dict(attention_mask=mask, max_new_tokens=NEW)
    for use_graph in (False, True):
        kw = dict(base, do_sample=True, temperature=0.8, top_k=40, top_p=0.9, min_p=0.02, repetition_penalty=1.3,
                  use_graph=use_graph)
        a = model.generate(ids, generator=torch.Generator().manual_seed(5), **kw)
        b = model.generate(ids, generator=torch.Generator().manual_seed(5), **kw)
        c = model.generate(ids, generator=torch.Generator().manual_seed(6), **kw)
        assert a.shape == (3, S + NEW) and torch.equal(a, b) and not torch.equal(a, c), (name, use_graph)
        # a nucleus below any token's share is greedy; so is a min_p just under 1
        greedy = model.generate(ids, **base, use_graph=use_graph)
        for kw2 in (dict(top_p=1e-6), dict(min_p=0.999999)):
            g = model.generate(ids, **base, do_sample=True, use_graph=use_graph,
                               generator=torch.Generator().manual_seed(7), **kw2)
            assert torch.equal(g, greedy), (name, use_graph, kw2)
        # a huge penalty, greedy: no row repeats a token of its prompt or of its continuation
        out = model.generate(ids, **base, repetition_penalty=1e4, use_graph=use_graph)
        for b_, r in enumerate(rows):
            seq = r.tolist() + out[b_, S:].tolist()
            assert len(set(seq)) == len(seq), (name, use_graph, b_, seq)
        assert not torch.equal(out, greedy) or all(len(set(r.tolist() + greedy[i, S:].tolist())) == len(r) + NEW
                                                   for i, r in enumerate(rows))
    # the session's greedy penalty equals the eager loop's (both by the reference ops here)
    assert torch.equal(model.generate(ids, **base, repetition_penalty=1.7, use_graph=True),
                       model.generate(ids, **base, repetition_penalty=1.7))


@pytest.mark.parametrize("family", [0, 1])
def test_generate_without_them_is_unchanged(family):
    name, make, prompts = model_cases()[family]
    model = make(0)
    ids, mask, _ = prompts(1, "right")
    for use_graph in (False, True):
        kw = dict(attention_mask=mask, max_new_tokens=8, do_sample=True, temperature=0.7, top_k=20,
                  use_graph=use_graph)
        want = model.generate(ids, generator=torch.Generator().manual_seed(11), **kw)
        sess = model.decode_session
        got = model.generate(ids, generator=torch.Generator().manual_seed(11), top_p=None, min_p=None,
                             repetition_penalty=None, **kw)
        assert torch.equal(got, want) and model.decode_session is sess
        if use_graph:       # neutral values: another session (its step takes the settings), the same tokens
            neutral = model.generate(ids, generator=torch.Generator().manual_seed(11), top_p=1.0, min_p=0.0,
                                     repetition_penalty=1.0, **kw)
            assert torch.equal(neutral, want) and model.decode_session is not sess and model.decode_session.ext


@pytest.mark.parametrize("family", [0, 1])
def test_generate_value_errors(family):
    name, make, prompts = model_cases()[family]
    model = make(0)
    ids, mask, _ = prompts(1, "right")
    for kw in (dict(top_p=0.0), dict(top_p=1.01), dict(min_p=-1e-3), dict(min_p=1.0), dict(repetition_penalty=0.0),
               dict(repetition_penalty=-2.0)):
        for use_graph in (False, True):
            with pytest.raises(ValueError, match=next(iter(kw))):
                model.generate(ids, attention_mask=mask, max_new_tokens=2, do_sample=True, use_graph=use_graph, **kw)
