"""Document-masked causal attention for packed rows (GPU only): the tiled kernels' DOC instances
(ddl_attn_doc_fwd / ddl_attn_doc_bwd), in which query i sees key j iff doc_start[b, i] <= j <= i.

References and tolerance are those of test_attention_edges_gpu.py (`check`, M = 2): the local `ref64_doc` /
`emu_doc` are test_attention_causal_gpu's `ref64_causal` / `emu_causal` with -inf added on the keys before
the query's document as well.  The emulation applies the same mask, so the margin over its error carries
over unchanged, as the causal test argues.

Lengths 65, 129, 193, 321: past one 64-key tile, past one 128-row forward workgroup, and 2 / 3 / 5 backward
tiles.  Layouts (document starts per batch row, always different in the two rows): starts on the tile edges,
starts one either side of them, a run of one-token documents followed by a long one, a document that starts
at 256 of 321 (the last query tile skips four whole key tiles), and a 128-row forward workgroup that holds
two documents of which the first started two tiles back.

Cases: parity on random inputs (p in {0, 0.25}); all-zero doc_start is the plain causal call bit for bit
(keep words included); one-token documents are exact; isolation (every other document replaced by large
values: this document's rows do not change by one bit); routing (a start moved by one position moves that
query's output by O(1)); the bias-gradient column sums; repeatability; bounds on another device refused.

Measured on an MI355X (88 cases, 160 comparisons, all passing): with the ulp term subtracted the largest ratios
are 0.95 (max form; dQ, S = 129, starts around the tile edges, p = 0.25) and 0.68 (rms form; dK, S = 193,
one-token documents, p = 0.25); dK reaches 0.82, out 0.39, dV 0.50.  As plain kernel error / emulation error
the largest are 1.51 (dQ), 1.38 (dK), 1.08 (out) and 1.00 (dV).  The column sums reach 0.18 of their bound.
"""
import math

import pytest
import torch

from conftest import gpu_device
from test_attention_causal_gpu import _tri, run_causal
from test_attention_edges_gpu import D, _bf, _heads, _merge, _split, check_all, keep_bits, random_inputs

pytestmark = pytest.mark.gpu

B, H = 2, 2
S_DOC = [65, 129, 193, 321]


# ------------------------------------------------------------------ layouts
def layouts(S):
    """name -> the document starts of the two batch rows (entries >= S dropped)."""
    def cut(st):
        return [s for s in st if s < S]
    out = {
        "edges": [cut([0, 64, 128, 192, 256]), cut([0, 128])],
        "around": [cut([0, 63, 65, 127, 129]), cut([0, 1, 191, 193, 255, 257])],
        "ones": [list(range(min(70, S // 2))), cut([0, 64])],
    }
    if S > 256:
        out["last256"] = [[0, 256], [0, 300]]
    if S > 160:
        out["two_in_wg"] = [[0, 10, 160], [0, 129]]
    return out


CASES = [(S, name) for S in S_DOC for name in layouts(S)]


def bounds(starts, S, dev):
    """doc_start, doc_end (int32 [B, S]) of per-row start lists, through ops.doc_bounds."""
    from databricks_distributed_deep_learning_amd import ops
    pos = torch.empty(len(starts), S, dtype=torch.long)
    for b, st in enumerate(starts):
        first = torch.zeros(S, dtype=torch.long)
        for s in st:
            first[s:] = s
        pos[b] = torch.arange(S) - first
    return ops.doc_bounds(pos.to(dev))


def spans(st, S):
    return list(zip(st, list(st[1:]) + [S]))


# ------------------------------------------------------------------ references
def _docmask(ds, S, dtype):
    """[B, 1, S, S]: -inf above the diagonal and on the keys before the query's document"""
    ar = torch.arange(S, device=ds.device)
    before = ar.view(1, 1, 1, S) < ds.view(-1, 1, S, 1)
    return _tri(S, ds.device, dtype).expand(ds.shape[0], 1, S, S).masked_fill(before, -math.inf)


def ref64_doc(qkv, H, ds, keep, p, g):
    """test_attention_causal_gpu.ref64_causal with the document -inf as well: out, dqkv."""
    Bq, S, _ = qkv.shape
    x = qkv.detach().double().requires_grad_(True)
    q, k, v = _split(x, H)
    s = q @ k.transpose(-1, -2) / math.sqrt(D) + _docmask(ds, S, torch.float64)
    P = torch.softmax(s, -1)
    Pd = P if keep is None else P * keep.double() / (1.0 - p)
    out = _merge(Pd @ v)
    out.backward(g.double())
    return out.detach(), x.grad


def emu_doc(qkv, H, ds, keep, p, g):
    """test_attention_causal_gpu.emu_causal with the document -inf as well: out, dqkv (both bf16)."""
    Bq, S, _ = qkv.shape
    q, k, v = _split(qkv.detach().float(), H)
    scale = 1.0 / math.sqrt(D)
    s = (q @ k.transpose(-1, -2)) * scale + _docmask(ds, S, torch.float32)
    P = torch.softmax(s, -1)
    kf = 1.0 if keep is None else keep.float() / (1.0 - p)
    Pd = _bf(P * kf)
    out = (Pd @ v).bfloat16()
    do = _heads(g.float(), H)
    delta = (do * out.float()).sum(-1, keepdim=True)
    dS = _bf(P * ((do @ v.transpose(-1, -2)) * kf - delta))
    dq = (dS @ k) * scale
    dk = (dS.transpose(-1, -2) @ q) * scale
    dv = Pd.transpose(-1, -2) @ do
    grad = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(Bq, S, 3 * H * D)
    return _merge(out), grad.bfloat16()


def run_doc(qkv, H, doc, p, g, key=123):
    """out, dqkv (the tensor the backward returned, with its column-sum rows) and the keep bits."""
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.ops import _native_attention as NA
    Bq, S, _ = qkv.shape
    x = qkv.detach().clone().requires_grad_(True)
    got = []
    x.register_hook(got.append)
    torch.manual_seed(key)
    out = ops.attention(x, H, None, p, True, causal=True, doc_start=doc)
    keep = None
    if p > 0:
        torch.manual_seed(key)
        keep = keep_bits(NA.new_seed(), Bq, S, H, p, qkv.device)
    out.backward(g)
    return out.detach(), got[0], keep


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("S,name", CASES)
def test_parity(S, name, p):
    dev = gpu_device()
    qkv, g, _ = random_inputs(B, S, H, None, dev, 3 + S)
    doc = bounds(layouts(S)[name], S, dev)
    out, grad, keep = run_doc(qkv, H, doc, p, g)
    r_out, r_grad = ref64_doc(qkv, H, doc[0], keep, p, g)
    e_out, e_grad = emu_doc(qkv, H, doc[0], keep, p, g)
    fails = []
    check_all(fails, f"doc S={S} {name} p={p}", out, grad, r_out, r_grad, e_out, e_grad, H)
    assert not fails, "\n".join(fails)
    # doc_start alone (the ends derived on the device) is the same call
    out2, grad2, _ = run_doc(qkv, H, doc[0], p, g)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)


# ------------------------------------------------------------------ 2. one document is plain causal
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("S", S_DOC)
def test_one_document_is_plain_causal(S, p):
    """doc_start all zero: the same tiles in the same order, so out, dQKV, the log-sum-exp and the keep
    words the forward stored are those of causal=True without doc_start, bit for bit."""
    from databricks_distributed_deep_learning_amd.ops import _lib, _native_attention  # noqa: F401 (signatures)
    dev = gpu_device()
    qkv, g, _ = random_inputs(B, S, H, None, dev, 13 + S)
    doc = bounds([[0], [0]], S, dev)
    assert not doc[0].any() and (doc[1] == S).all()
    o1, g1, _ = run_causal(qkv, H, None, p, g, key=7)
    o2, g2, _ = run_doc(qkv, H, doc, p, g, key=7)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    assert torch.equal(g1._ddl_colsum_rows[0], g2._ddl_colsum_rows[0])
    fn = _lib.fn("ddl_attn_dmask_words")
    fn.restype = _lib.L
    res = []
    for name, extra in (("ddl_attn_causal_fwd", ()), ("ddl_attn_doc_fwd", (doc[0].data_ptr(), doc[1].data_ptr()))):
        out = torch.empty(B, S, H * D, dtype=torch.bfloat16, device=dev)
        lse = torch.full((B, H, S), float("nan"), dtype=torch.float32, device=dev)
        words = torch.zeros(fn(B, S, H), dtype=torch.int32, device=dev)
        _lib.call(name, qkv.data_ptr(), 0, out.data_ptr(), lse.data_ptr(), B, S, H, 1.0 / math.sqrt(D), p, 99,
                  words.data_ptr() if p > 0 else 0, *extra)
        torch.cuda.synchronize()
        res.append((out, lse, words))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert p == 0 or res[0][2].any()


# ------------------------------------------------------------------ 3. one-token documents are exact
@pytest.mark.parametrize("S", [65, 193])
def test_length_one_documents_exact(S):
    """Row 0: every token its own document, p = 0.  Its one probability is 2^(rounding residue) = 1 to within
    2 ulp of fp32, which is 1 in bf16, so out = V and dV = dO bit for bit.  dS = P (dO . V - dO . O) is an exact
    zero when the two dot products are: V and dO here are multiples of 1/8 below 2, so every partial sum of
    their 64 products is a multiple of 1/64 below 2^9 -- exact in fp32 in any order -- and dQ = dK = 0."""
    dev = gpu_device()
    hd = H * D
    gen = torch.Generator().manual_seed(S)
    qkv = torch.randn(B, S, 3 * hd, generator=gen)
    qkv[..., 2 * hd:] = torch.randint(-15, 16, (B, S, hd), generator=gen).float() / 8
    g = (torch.randint(-15, 16, (B, S, hd), generator=gen).float() / 8).bfloat16().to(dev)
    qkv = qkv.bfloat16().to(dev)
    doc = bounds([list(range(S)), [0, 64]], S, dev)
    out, grad, _ = run_doc(qkv, H, doc, 0.0, g)
    assert torch.equal(out[0], qkv[0, :, 2 * hd:]), "out != V"
    assert torch.equal(grad[0, :, 2 * hd:], g[0]), "dV != dO"
    assert (grad[0, :, :2 * hd] == 0).all(), "dQ / dK not zero"
    assert grad[1, :, :2 * hd].float().abs().max() > 0          # the other row does carry dQ, dK


# ------------------------------------------------------------------ 4. isolation
def _some(n):
    """every document index up to 6 of them; beyond that the first two, the middle one and the last two"""
    return list(range(n)) if n <= 6 else sorted({0, 1, n // 2, n - 2, n - 1})


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("S,name", CASES)
def test_isolation(S, name, p):
    """The q, k, v and dout rows of every document but one replaced by other finite values 16 times as large:
    that document's rows of out, dQ, dK and dV do not change by one bit.  A masked score is set to -inf by a
    select and contributes exp2(-inf) = 0 exactly, and the tiles a row visits do not depend on values, so
    this needs no tolerance: a leaked key, a leaked query in dK / dV or a loop bound taken from the wrong row
    moves some bit."""
    dev = gpu_device()
    starts = layouts(S)[name]
    qkv, g, _ = random_inputs(B, S, H, None, dev, 51 + S)
    doc = bounds(starts, S, dev)
    base = run_doc(qkv, H, doc, p, g, key=77)
    gen = torch.Generator().manual_seed(S + 1)
    big_x = (16.0 * torch.randn(B, S, 3 * H * D, generator=gen)).bfloat16().to(dev)
    big_g = (16.0 * torch.randn(B, S, H * D, generator=gen)).bfloat16().to(dev)
    sp = [spans(st, S) for st in starts]
    picks = [_some(len(s)) for s in sp]
    for i in range(max(len(pk) for pk in picks)):
        x2, g2 = big_x.clone(), big_g.clone()
        own = []
        for b in range(B):
            a, e = sp[b][picks[b][i % len(picks[b])]]
            x2[b, a:e], g2[b, a:e] = qkv[b, a:e], g[b, a:e]
            own.append((a, e))
        out2, grad2, _ = run_doc(x2, H, doc, p, g2, key=77)
        assert torch.isfinite(grad2.float()).all() and torch.isfinite(out2.float()).all()
        for b, (a, e) in enumerate(own):
            assert torch.equal(out2[b, a:e], base[0][b, a:e]), f"row {b} doc [{a}, {e}): out differs"
            for j, nm in enumerate("QKV"):
                sl = slice(j * H * D, (j + 1) * H * D)
                assert torch.equal(grad2[b, a:e, sl], base[1][b, a:e, sl]), f"row {b} doc [{a}, {e}): d{nm} differs"
    assert base[0].float().abs().max() > 0 and base[1].float().abs().max() > 0


# ------------------------------------------------------------------ 5. routing
@pytest.mark.parametrize("s", [63, 64, 65, 128, 191])
def test_start_moved_by_one(s):
    """Layout A starts a document at s, layout B at s + 1.  In A query s sees itself alone (out = its v); in B
    it ends the first document and averages s + 1 keys: O(1) apart, and each run matches the fp64 reference of
    its own layout -- an off-by-one in the start compare makes one of them the other's."""
    dev = gpu_device()
    S = 193
    qkv, g, _ = random_inputs(B, S, H, None, dev, 71 + s)
    res = []
    for start in (s, s + 1):
        doc = bounds([[0, start], [0, start]], S, dev)
        out, grad, _ = run_doc(qkv, H, doc, 0.0, g)
        r_out, r_grad = ref64_doc(qkv, H, doc[0], None, 0.0, g)
        e_out, e_grad = emu_doc(qkv, H, doc[0], None, 0.0, g)
        fails = []
        check_all(fails, f"doc moved start={start}", out, grad, r_out, r_grad, e_out, e_grad, H)
        assert not fails, "\n".join(fails)
        res.append(out)
    assert torch.equal(res[0][:, s], qkv[:, s, 2 * H * D:])
    assert (res[0][:, s].float() - res[1][:, s].float()).abs().max().item() > 0.5
    assert torch.equal(res[0][:, :s], res[1][:, :s])


# ------------------------------------------------------------------ 6. column sums, repeatability
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("S,name", [(65, "around"), (193, "two_in_wg"), (321, "last256"), (321, "ones")])
def test_colsum_rows(S, name, p):
    """As test_attention_causal_gpu.test_colsum_rows: the rows attached to dQKV sum to its column sums within
    sum|x| * (2^-8 [each element's bf16 rounding] + N * 2^-24 [fp32 summation of N = B * S terms])."""
    dev = gpu_device()
    qkv, g, _ = random_inputs(B, S, H, None, dev, 21 + S)
    _, grad, _ = run_doc(qkv, H, bounds(layouts(S)[name], S, dev), p, g)
    rows, ver = grad._ddl_colsum_rows
    assert ver == grad._version and rows.shape == (B * 4 * -(-S // 64), 3 * H * D)
    got = rows.double().sum(0)
    x = grad.double().reshape(-1, 3 * H * D)
    want, mag = x.sum(0), x.abs().sum(0)
    bound = mag * (2.0 ** -8 + x.shape[0] * 2.0 ** -24) + 1e-30
    worst = ((got - want).abs() / bound).max().item()
    print(f"COLSUM doc S={S} {name} p={p} worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("S,name", [(65, "ones"), (193, "around"), (321, "edges")])
def test_repeatable(S, name):
    dev = gpu_device()
    qkv, g, _ = random_inputs(B, S, H, None, dev, 31 + S)
    doc = bounds(layouts(S)[name], S, dev)
    a = run_doc(qkv, H, doc, 0.25, g, key=5)
    b = run_doc(qkv, H, doc, 0.25, g, key=5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[1]._ddl_colsum_rows[0], b[1]._ddl_colsum_rows[0])


# ------------------------------------------------------------------ 7. dispatch
def test_mask_with_doc_start_takes_the_reference():
    """No native MASK && DOC instance: the key bias together with doc_start composes the reference ops (and
    the entry point refuses a mask)."""
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.ops import _lib, _native_attention  # noqa: F401 (signatures)
    from databricks_distributed_deep_learning_amd.ops.attention import attention_reference
    dev = gpu_device()
    S = 129
    qkv, g, mask = random_inputs(B, S, H, "suffix", dev, 5)
    doc = bounds(layouts(S)["around"], S, dev)
    from databricks_distributed_deep_learning_amd.ops import attention as A
    A._warned_mask_doc = False
    with pytest.warns(RuntimeWarning, match="no HIP kernel"):
        got = ops.attention(qkv, H, mask, 0.0, False, causal=True, doc_start=doc)
    want = attention_reference(qkv, H, mask, 0.0, False, causal=True, doc_start=doc[0])
    assert torch.equal(got, want)
    out = torch.empty(B, S, H * D, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
    rc = _lib.fn("ddl_attn_doc_fwd")(qkv.data_ptr(), mask.data_ptr(), out.data_ptr(), lse.data_ptr(), B, S, H, 0.125,
                                     0.0, 0, 0, doc[0].data_ptr(), doc[1].data_ptr(), _lib.stream())
    assert rc == -7


def test_bounds_on_another_device_are_refused():
    """doc_start on the host with qkv on the GPU is a ValueError at the op and through both models, not a host
    pointer handed to a kernel."""
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.models import cast_params, gpt2_tiny, llama_tiny
    dev = gpu_device()
    S = 65
    qkv, _, _ = random_inputs(B, S, H, None, dev, 1)
    ds, de = bounds(layouts(S)["around"], S, torch.device("cpu"))
    for arg in (ds, (ds, de), (ds.to(dev), de)):
        with pytest.raises(ValueError, match="doc_start"):
            ops.attention(qkv, H, None, 0.0, False, causal=True, doc_start=arg)
    ids = torch.randint(0, 1000, (B, S), device=dev)
    pos = torch.arange(S).expand(B, S).contiguous()             # on the host
    for make in (llama_tiny, gpt2_tiny):
        model = cast_params(make().to(dev), torch.bfloat16).eval()
        with pytest.raises(ValueError, match="position_ids"):
            model(ids, position_ids=pos)
