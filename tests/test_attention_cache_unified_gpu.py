"""The MHA and the grouped-query KV-cache entry points are one kernel each (GPU only; csrc/kernels/attn_decode.hip,
csrc/kernels/attn_extend.hip): ``ops.attention_decode`` / ``attention_extend`` / ``kv_cache_fill`` against
``ops.attention_decode_gqa`` / ``attention_extend_gqa`` / ``kv_cache_fill_gqa`` at Hkv = H, bit for bit.

GPT-2's packed ``[.., 3 H 64]`` projection is the grouped layout ``[q heads | k heads | v heads]`` with Hkv = H, and
under the identity table (cos 1, sin 0) the rotation ``x 1 - y 0`` returns the bits of a non-zero finite ``x``.
So the same tensors go to both entry points, and the outputs and the whole caches (every appended row among
them) must be EQUAL, not close.  The inputs are random bf16 with no exact-zero element (asserted): a zero could
come back with the other sign.  Dead cache rows hold arbitrary bit patterns, NaN / Inf among them.

Decode: B = 2, H = 4, C = 1024; lens (0, 33), (129, 64), (1023, 257); max_len tight (max n + 1) and C.  For
max_len <= 1024 both entry points split alike whatever the CU count (ceil(max_len / 64) <= 16 is at most both
split caps): asserted as a precondition.  Extend: B = 2, H = 4, C = 256; T in {1, 16, 17, 33, 70} (every
instance of the MHA entry point, two query tiles at T = 70); lens (0, 63), (64, 129); with and without ragged
new_lens, rows >= new_lens zero in both.  Fill: B = 2, S = 70, H = 4.
"""
import pytest
import torch

from conftest import gpu_device
from test_attention_decode_gqa_gpu import _bits, _garbage
from test_attention_edges_gpu import D

from databricks_distributed_deep_learning_amd import ops
from databricks_distributed_deep_learning_amd.ops import _lib

pytestmark = pytest.mark.gpu

B, H = 2, 4


def _identity(n_pos, dev):
    return torch.cat([torch.ones(n_pos, D // 2), torch.zeros(n_pos, D // 2)], 1).to(dev)


def _inputs(shape, lens, C, dev, seed):
    """The projection (randn bf16, no exact zero) and the two caches [B, H, C, D]: live rows randn, the rest
    arbitrary bits."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(*shape, generator=g).bfloat16().to(dev)
    assert (qkv != 0).all() and torch.isfinite(qkv.float()).all()
    ck, cv = _garbage((B, H, C, D), dev, seed + 1), _garbage((B, H, C, D), dev, seed + 2)
    for b, n in enumerate(lens):
        ck[b, :, :n] = torch.randn(H, n, D, generator=g).bfloat16().to(dev)
        cv[b, :, :n] = torch.randn(H, n, D, generator=g).bfloat16().to(dev)
    return qkv, ck, cv, torch.tensor(lens, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("tight", [True, False], ids=["tight", "capacity"])
@pytest.mark.parametrize("lens", [(0, 33), (129, 64), (1023, 257)])
def test_decode_mha_is_gqa_at_identity(lens, tight):
    dev = gpu_device()
    C = 1024
    max_len = max(lens) + 1 if tight else C
    qkv, ck, cv, lt = _inputs((B, 3 * H * D), lens, C, dev, 11 + lens[0])
    ck2, cv2 = ck.clone(), cv.clone()
    before_k = ck.clone()
    # precondition: both entry points split the keys alike (ceil(max_len / 64) <= 16 is at most both caps)
    assert _lib.fn("ddl_attn_decode_nsplit")(B, H, max_len) == _lib.fn("ddl_attn_decode_gqa_nsplit")(B, H, max_len)
    o1 = ops.attention_decode(qkv, ck, cv, lt, H, max_len)
    o2 = ops.attention_decode_gqa(qkv, _identity(C, dev), ck2, cv2, lt, H, H, max_len)
    torch.cuda.synchronize()
    assert torch.equal(_bits(o1), _bits(o2))
    assert torch.equal(_bits(ck), _bits(ck2)) and torch.equal(_bits(cv), _bits(cv2))
    # the appended rows are the projection's K / V rows, and nothing else changed
    x = qkv.view(B, 3, H, D)
    for b, n in enumerate(lens):
        assert torch.equal(_bits(ck[b, :, n]), _bits(x[b, 1])) and torch.equal(_bits(cv[b, :, n]), _bits(x[b, 2]))
        before_k[b, :, n] = x[b, 1]
    assert torch.equal(_bits(ck), _bits(before_k))


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("lens", [(0, 63), (64, 129)])
@pytest.mark.parametrize("T", [1, 16, 17, 33, 70])
def test_extend_mha_is_gqa_at_identity(T, lens, ragged):
    dev = gpu_device()
    C = 256
    max_len = max(lens)
    ts = ((T + 1) // 2, T) if ragged else (T, T)
    new_lens = torch.tensor(ts, dtype=torch.int32, device=dev) if ragged else None
    qkv, ck, cv, lt = _inputs((B, T, 3 * H * D), lens, C, dev, 1000 * T + lens[0])
    ck2, cv2 = ck.clone(), cv.clone()
    before_k = ck.clone()
    o1 = ops.attention_extend(qkv, ck, cv, lt, H, max_len, new_lens)
    o2 = ops.attention_extend_gqa(qkv, _identity(C, dev), ck2, cv2, lt, H, H, max_len, new_lens)
    torch.cuda.synchronize()
    assert torch.equal(_bits(o1), _bits(o2))
    assert torch.equal(_bits(ck), _bits(ck2)) and torch.equal(_bits(cv), _bits(cv2))
    x = qkv.view(B, T, 3, H, D)
    for b, (n, t) in enumerate(zip(lens, ts)):
        assert (_bits(o1[b, t:]) == 0).all() and (_bits(o2[b, t:]) == 0).all()
        assert torch.equal(_bits(ck[b, :, n:n + t]), _bits(x[b, :t, 1].transpose(0, 1)))
        assert torch.equal(_bits(cv[b, :, n:n + t]), _bits(x[b, :t, 2].transpose(0, 1)))
        before_k[b, :, n:n + t] = x[b, :t, 1].transpose(0, 1)
    assert torch.equal(_bits(ck), _bits(before_k))


def test_fill_mha_is_gqa_at_equal_heads():
    dev = gpu_device()
    S, C = 70, 128
    qkv, ck, cv, _ = _inputs((B, S, 3 * H * D), (0, 0), C, dev, 5)
    ck2, cv2 = ck.clone(), cv.clone()
    ops.kv_cache_fill(qkv, ck, cv, H)
    ops.kv_cache_fill_gqa(qkv, ck2, cv2, H, H)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ck[:, :, :S]), _bits(ck2[:, :, :S])) and torch.equal(_bits(cv[:, :, :S]), _bits(cv2[:, :, :S]))
    x = qkv.view(B, S, 3, H, D)
    assert torch.equal(_bits(ck[:, :, :S]), _bits(x[:, :, 1].transpose(1, 2)))
    assert torch.equal(_bits(cv[:, :, :S]), _bits(x[:, :, 2].transpose(1, 2)))
    assert torch.equal(_bits(ck), _bits(ck2)) and torch.equal(_bits(cv), _bits(cv2))
