"""``ops.rope_qkv(..., positions=...)`` on the HIP kernels (GPU only; the reference-path twin is in
test_packed_cpu.py).  The rotation is per token -- one table row, one rounding per output element -- so
both properties are exact: ``positions = arange(S)`` is the call without the argument, and a packed row is,
per document slice, that document rotated on its own, in the forward and in the backward."""
import pytest
import torch

from conftest import gpu_device

pytestmark = pytest.mark.gpu

B, S, D = 2, 70, 64
STARTS = [[0, 1, 33, 64], [0, 69]]


def _positions(dev):
    pos = torch.empty(B, S, dtype=torch.int32)
    for b, st in enumerate(STARTS):
        first = torch.zeros(S, dtype=torch.int32)
        for s in st:
            first[s:] = s
        pos[b] = torch.arange(S, dtype=torch.int32) - first
    return pos.to(dev)


def _run(x, table, H, Hkv, dy, pos=None):
    from databricks_distributed_deep_learning_amd import ops
    x = x.clone().requires_grad_(True)
    y = ops.rope_qkv(x, table, H, Hkv) if pos is None else ops.rope_qkv(x, table, H, Hkv, positions=pos)
    y.backward(dy)
    return y.detach(), x.grad


@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2), (9, 3)])
def test_rope_positions_native(H, Hkv):
    from databricks_distributed_deep_learning_amd import ops
    from databricks_distributed_deep_learning_amd.ops.llama import rope_qkv_reference
    dev = gpu_device()
    g = torch.Generator().manual_seed(H)
    table = ops.rope_table(128, 10000.0, D, device=dev)
    x = torch.randn(B, S, (H + 2 * Hkv) * D, generator=g).bfloat16().to(dev)
    dy = torch.randn(B, S, 3 * H * D, generator=g).bfloat16().to(dev)
    # arange is the call without the argument, bit for bit
    ar = torch.arange(S, dtype=torch.int32, device=dev).expand(B, S).contiguous()
    y0, g0 = _run(x, table, H, Hkv, dy)
    y1, g1 = _run(x, table, H, Hkv, dy, ar)
    assert torch.equal(y0, y1) and torch.equal(g0, g1)
    # a packed row is, per document slice, that document rotated alone
    pos = _positions(dev)
    yp, gp = _run(x, table, H, Hkv, dy, pos)
    for b, st in enumerate(STARTS):
        for a, e in zip(st, st[1:] + [S]):
            ya, ga = _run(x[b:b + 1, a:e], table, H, Hkv, dy[b:b + 1, a:e].contiguous())
            assert torch.equal(yp[b:b + 1, a:e], ya), f"forward, row {b} document [{a}, {e})"
            assert torch.equal(gp[b:b + 1, a:e], ga), f"backward, row {b} document [{a}, {e})"
    assert not torch.equal(yp, y0)
    # and what the reference computes, to a bf16 rounding of values below 8 (fused multiply-adds differ)
    assert (yp.float() - rope_qkv_reference(x, table, H, Hkv, pos).float()).abs().max().item() <= 2.0 ** -5
    # S may pass the table's rows as long as the positions stay inside it
    small = ops.rope_table(40, 10000.0, D, device=dev)
    p40 = pos.clamp(max=39)
    assert torch.equal(_run(x, small, H, Hkv, dy, p40)[0], _run(x, table, H, Hkv, dy, p40)[0])
