"""The grouped-query extend reference on the CPU (fp32 / fp64 / bf16): against a composition of the references
that existed before it, against the grouped-query decode reference at T = 1, the single rounding of the
rotated operands, dead positions, and every host guard."""
import pytest
import torch

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.ops.attention import (attention_decode_gqa_reference,
                                                                   attention_extend_gqa_reference,
                                                                   attention_extend_reference)
from databricks_distributed_deep_learning_amd.ops.llama import rope_qkv_reference


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def _case(G, B=3, Hkv=2, D=16, C=24, T=7, seed=0):
    H = Hkv * G
    g = torch.Generator().manual_seed(100 * G + seed)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, generator=g, dtype=torch.float64)
    ck = torch.randn(B, Hkv, C, D, generator=g, dtype=torch.float64)
    cv = torch.randn(B, Hkv, C, D, generator=g, dtype=torch.float64)
    return H, qkv, ck, cv, ops.rope_table(C, 10000.0, D).double()


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("G", [1, 2, 3, 4, 8])
def test_extend_gqa_reference_is_rope_then_extend(G, ragged):
    """fp64: per batch row, ``rope_qkv_reference`` on the row's chunk with ``table[n:n+T]``, then
    ``attention_extend_reference`` over the cache expanded by ``repeat_interleave(G)``.  Unequal n, one row at
    n = 0 and one that ends in the last slot."""
    B, Hkv, D, C, T = 3, 2, 16, 24, 7
    H, qkv, ck0, cv0, table = _case(G)
    lens, news = [0, C - T, 5], ([T, 3, 1] if ragged else None)
    lt, nt = _i32(lens), (_i32(news) if ragged else None)
    ck, cv = ck0.clone(), cv0.clone()
    out = attention_extend_gqa_reference(qkv, table, ck, cv, lt, H, Hkv, C - T, nt)
    assert out.shape == (B, T, H * D) and lt.tolist() == lens and (nt is None or nt.tolist() == news)
    wk, wv = ck0.clone(), cv0.clone()
    for b, n in enumerate(lens):
        t = news[b] if ragged else T
        packed = rope_qkv_reference(qkv[b:b + 1], table[n:n + T], H, Hkv)
        ek = ck0[b:b + 1].repeat_interleave(G, 1).contiguous()
        ev = cv0[b:b + 1].repeat_interleave(G, 1).contiguous()
        want = attention_extend_reference(packed, ek, ev, lt[b:b + 1], H, C - T, None if nt is None else nt[b:b + 1])
        assert (out[b] - want[0]).abs().max().item() <= 1e-12
        assert (out[b, t:] == 0).all()
        # positions n .. n + t - 1 of each KV head hold the rotated keys and the values
        _, k, v = packed.view(T, 3, H, D).unbind(1)
        assert torch.equal(ck[b, :, n:n + t], k[:t, ::G].transpose(0, 1))
        assert torch.equal(cv[b, :, n:n + t], v[:t, ::G].transpose(0, 1))
        wk[b, :, n:n + t], wv[b, :, n:n + t] = k[:t, ::G].transpose(0, 1), v[:t, ::G].transpose(0, 1)
    # ... and every other cache element is unchanged
    assert torch.equal(ck, wk) and torch.equal(cv, wv)
    # the public op routes CPU tensors to the reference; a dead tail of NaN and NaN in the padded columns
    # cannot reach the output or the cache
    ck2, cv2, q2 = ck0.clone(), cv0.clone(), qkv.clone()
    for b, n in enumerate(lens):
        ck2[b, :, n:], cv2[b, :, n:] = float("nan"), float("nan")
        if ragged:
            q2[b, news[b]:] = float("nan")
    assert torch.equal(ops.attention_extend_gqa(q2, table, ck2, cv2, lt, H, Hkv, C - T, nt), out)
    for b, n in enumerate(lens):
        t = news[b] if ragged else T
        assert torch.equal(ck2[b, :, n:n + t], ck[b, :, n:n + t]) and torch.equal(cv2[b, :, n:n + t], cv[b, :, n:n + t])
        assert ck2[b, :, n + t:].isnan().all() and torch.equal(ck2[b, :, :n], ck0[b, :, :n])


@pytest.mark.parametrize("G", [1, 2, 3, 4, 8])
def test_extend_gqa_reference_at_one_token_is_decode(G):
    B, Hkv, D, C = 3, 2, 16, 12
    H, qkv, ck0, cv0, table = _case(G, C=C, T=1)
    lt = _i32([0, C - 1, 5])
    ck, cv = ck0.clone(), cv0.clone()
    out = attention_extend_gqa_reference(qkv, table, ck, cv, lt, H, Hkv, C - 1)
    dk, dv = ck0.clone(), cv0.clone()
    want = attention_decode_gqa_reference(qkv[:, 0], table, dk, dv, lt, H, Hkv, C)
    assert (out[:, 0] - want).abs().max().item() <= 1e-12
    assert torch.equal(ck, dk) and torch.equal(cv, dv)


def test_extend_gqa_reference_rounds_rotated_operands_once():
    """bf16: the appended keys are the fp32 rotation rounded once -- rope_qkv_reference's bits."""
    B, H, Hkv, D, C, T = 2, 4, 2, 64, 16, 5
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, generator=g).bfloat16()
    ck, cv = torch.zeros(B, Hkv, C, D).bfloat16(), torch.zeros(B, Hkv, C, D).bfloat16()
    table = ops.rope_table(C, 10000.0, D)
    lens = [3, 11]
    ops.attention_extend_gqa(qkv, table, ck, cv, _i32(lens), H, Hkv, C - T)
    for b, n in enumerate(lens):
        packed = rope_qkv_reference(qkv[b:b + 1], table[n:n + T], H, Hkv).view(T, 3, H, D)
        assert torch.equal(ck[b, :, n:n + T], packed[:, 1, ::2].transpose(0, 1))
        assert torch.equal(cv[b, :, n:n + T], packed[:, 2, ::2].transpose(0, 1))


def test_extend_gqa_clamps_lens_and_new_lens():
    """A lens beyond max_len and a new_lens outside 1 .. T are clamped: every access stays in bounds."""
    H, qkv, ck, cv, table = _case(2, B=2, C=12, T=4)
    out = ops.attention_extend_gqa(qkv, table, ck, cv, _i32([99, -5]), H, 2, 8, _i32([0, 77]))
    assert torch.isfinite(out[0, 0]).all() and (out[0, 1:] == 0).all() and torch.isfinite(out[1]).all()


def test_host_guards():
    B, H, Hkv, D, C, T = 2, 4, 2, 16, 8, 3
    ck, cv = torch.zeros(B, Hkv, C, D), torch.zeros(B, Hkv, C, D)
    lens = torch.zeros(B, dtype=torch.int32)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D)
    table = ops.rope_table(8, 10000.0, D)
    f = ops.attention_extend_gqa
    f(qkv, table, ck, cv, lens, H, Hkv, C - T)
    with pytest.raises(ValueError, match="capacity"):
        f(qkv, table, ck, cv, lens, H, Hkv, C - T + 1)
    with pytest.raises(ValueError, match="at least 0"):
        f(qkv, table, ck, cv, lens, H, Hkv, -1)
    with pytest.raises(ValueError, match="rotary table"):
        f(qkv, table[:7], ck, cv, lens, H, Hkv, C - T)
    with pytest.raises(ValueError, match="multiple of num_kv_heads"):
        f(torch.randn(B, T, 7 * D), table, torch.zeros(B, 3, C, D), torch.zeros(B, 3, C, D), lens, 4, 3, 0)
    with pytest.raises(RuntimeError, match="autograd"):
        f(qkv.clone().requires_grad_(), table, ck, cv, lens, H, Hkv, 0)
    with pytest.raises(ValueError, match="cache must be"):
        f(qkv, table, torch.zeros(B, H, C, D), torch.zeros(B, H, C, D), lens, H, Hkv, 0)
    with pytest.raises(ValueError, match="contiguous"):
        big = torch.zeros(B, Hkv, C, 2 * D)
        f(qkv, table, big[..., :D], big[..., D:], lens, H, Hkv, 0)
    with pytest.raises(ValueError, match="^lens"):
        f(qkv, table, ck, cv, lens.long(), H, Hkv, 0)
    with pytest.raises(ValueError, match="new_lens"):
        f(qkv, table, ck, cv, lens, H, Hkv, 0, torch.ones(B + 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="qkv_new must be"):
        f(qkv[:, 0], table, ck, cv, lens, H, Hkv, 0)
    with pytest.raises(ValueError, match="qkv_new must be"):
        f(qkv[:, :0], table, ck, cv, lens, H, Hkv, 0)
    with pytest.raises(ValueError, match="table must be"):
        f(qkv, table[:, :8], ck, cv, lens, H, Hkv, 0)
