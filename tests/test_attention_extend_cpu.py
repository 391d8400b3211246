"""``ops.attention_extend`` on the CPU: the plain-torch reference path (fp32 / fp64), its append and its guards."""
import math

import pytest
import torch

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.ops.attention import attention_extend_reference, attention_reference

B, H, D, C = 2, 2, 64, 48


def _lens(v):
    return torch.tensor(v, dtype=torch.int32)


@pytest.mark.parametrize("chunk", [1, 3, 16])
def test_extend_in_chunks_is_causal_attention(chunk):
    """An fp64 cache extended chunk by chunk from empty reproduces the rows of one causal attention."""
    torch.manual_seed(chunk)
    S = 35
    qkv = torch.randn(B, S, 3 * H * D, dtype=torch.float64)
    want = attention_reference(qkv, H, causal=True)
    ck = torch.full((B, H, C, D), math.nan, dtype=torch.float64)
    cv = torch.full((B, H, C, D), math.nan, dtype=torch.float64)
    lens = _lens([0, 0])
    for c0 in range(0, S, chunk):
        T = min(chunk, S - c0)
        out = ops.attention_extend(qkv[:, c0:c0 + T].contiguous(), ck, cv, lens, H, c0)
        assert lens.tolist() == [c0, c0]        # untouched by the op
        torch.testing.assert_close(out, want[:, c0:c0 + T], rtol=1e-5, atol=1e-5)
        lens += T
    _, k, v = qkv.view(B, S, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    assert torch.equal(ck[:, :, :S], k) and torch.equal(cv[:, :, :S], v)
    assert ck[:, :, S:].isnan().all() and cv[:, :, S:].isnan().all()


def _ragged_case(dtype=torch.float32):
    torch.manual_seed(3)
    T, n, t = 7, [5, 11], [7, 2]
    qkv = torch.randn(B, T, 3 * H * D, dtype=dtype)
    ck, cv = torch.randn(B, H, C, D, dtype=dtype), torch.randn(B, H, C, D, dtype=dtype)
    return T, n, t, qkv, ck, cv


def test_append_padding_and_lens():
    """The cache gains exactly rows n .. n+t-1, padded output rows are zeros, lens and new_lens are not written;
    a row's valid outputs do not depend on its padded columns."""
    T, n, t, qkv, ck, cv = _ragged_case()
    lens, new_lens = _lens(n), _lens(t)
    k0, v0 = ck.clone(), cv.clone()
    out = ops.attention_extend(qkv, ck, cv, lens, H, max(n), new_lens)
    assert lens.tolist() == n and new_lens.tolist() == t
    _, k, v = qkv.view(B, T, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    for b in range(B):
        k0[b, :, n[b]:n[b] + t[b]], v0[b, :, n[b]:n[b] + t[b]] = k[b, :, :t[b]], v[b, :, :t[b]]
        assert (out[b, t[b]:] == 0).all()
    assert torch.equal(ck, k0) and torch.equal(cv, v0)
    # row 1 alone, its two real columns only, against its own 11 cached keys
    alone = attention_extend_reference(qkv[1:, :2].contiguous(), k0[1:].clone(), v0[1:].clone(), _lens([11]), H, 11)
    torch.testing.assert_close(out[1:, :2], alone, rtol=1e-5, atol=1e-5)


def test_nan_in_dead_tail_and_padded_columns_stays_out():
    T, n, t, qkv, ck, cv = _ragged_case()
    want = ops.attention_extend(qkv, ck.clone(), cv.clone(), _lens(n), H, 20, _lens(t))
    for b in range(B):
        ck[b, :, n[b]:], cv[b, :, n[b]:] = math.nan, math.nan
        qkv[b, t[b]:] = math.nan
    out = ops.attention_extend(qkv, ck, cv, _lens(n), H, 20, _lens(t))
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out, want, rtol=1e-6, atol=1e-6)


def test_guards():
    T, n, t, qkv, ck, cv = _ragged_case()
    with pytest.raises(ValueError, match="capacity"):
        ops.attention_extend(qkv, ck, cv, _lens(n), H, C - T + 1)
    ops.attention_extend(qkv, ck, cv, _lens(n), H, C - T)        # the last slot is usable
    with pytest.raises(ValueError):
        ops.attention_extend(qkv, ck, cv, _lens(n), H, -1)
    with pytest.raises(RuntimeError, match="autograd"):
        ops.attention_extend(qkv.clone().requires_grad_(True), ck, cv, _lens(n), H, 11)
