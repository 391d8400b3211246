"""NHWC convolution as implicit GEMM on MFMA (csrc/kernels/gemm.hip), with autograd.

forward : y[m, k]  = sum_(r,s,c) x[pix(m, r, s), c] * W[k, r, s, c]   mode CONV
          (1x1 / stride-1 convs are plain NT GEMMs over [N*H*W, C])
dgrad   : stride 1 -> a stride-1 conv of dy with the flipped, transposed weight
          stride 2 -> four output-parity classes, each a small stride-1 conv of dy
          over the taps of that parity, written through a strided row remap (no
          zero-insertion, no wasted MFMA work)
wgrad   : dW[k, (r,s,c)] = sum_m dy[m, k] * im2col(x)[m, (r,s,c)]      mode CONVW,
          split-K over the N*P*Q output pixels with fp32 partial slabs
Inputs whose channel count is not a multiple of 8 are zero-padded to 8 channels so
every gathered chunk is one 16-byte load -- except the stride-2 RGB stem, which runs
as a stride-1 conv of its 2x2 space-to-depth transform (16 channels, 4x4 taps:
reduction 256 instead of 392; ``_StemConvS2D``).
"""
from __future__ import annotations

import ctypes
import os

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import grad_ready, grad_sink
from ._native_gemm import MODE_CONV, MODE_CONVW, MODE_NN, MODE_NT, MODE_TN, gemm, plan, stats_rows_max
from ._native_norm import _BN_BWD_EPI, _BN_BWD_EPI_RES


def _desc(N, H, W, C, P, Q, stride, h_off, w_off, h_step, w_step, R, S, OH, OW, ostep=1, oa=0, ob=0):
    return [N, H, W, C, P, Q, stride, h_off, w_off, h_step, w_step, R, S, OH, OW, ostep, oa, ob]


STATS_MIN_K = int(os.environ.get("DDL_BN_STATS_MIN_K", "0"))
_DGRAD_NT = os.environ.get("DDL_DGRAD_NT", "1") != "0"


_CONV3X3 = os.environ.get("DDL_CONV3X3", "1") != "0"


def _direct3x3_ok(x_shape, w_shape, stride, pad):
    """Shapes the direct 3x3 kernel (csrc/kernels/conv3x3.hip) covers: stride 1, pad 1,
    64 -> 64 channels, 49 <= W <= 64 with W % 8 == 0 (ResNet stage-1 conv2)."""
    N, H, W_, C = x_shape
    K, R, S, _ = w_shape
    return (_CONV3X3 and R == 3 and S == 3 and stride == 1 and pad == 1 and C == 64 and K == 64
            and W_ % 8 == 0 and 49 <= W_ <= 64 and N * H * W_ * 64 * 2 < 2 ** 31)


def _direct3x3(x, w, y, part=None, res=None, bnb=None, grid=0):
    """y = conv3x3(x, w) by the direct kernel; with ``bnb`` (ops.bridge.BNBackward) the
    BatchNorm-backward epilogue.  Returns the number of statistics rows written."""
    N, H, W_, C = x.shape
    full = (N, H, W_, 64)
    if (tuple(w.shape) != (64, 3, 3, 64) or tuple(y.shape) != full or C != 64 or not x.is_contiguous()
            or not w.is_contiguous() or not y.is_contiguous() or x.dtype != torch.bfloat16
            or w.dtype != torch.bfloat16 or y.dtype != torch.bfloat16):
        raise ValueError("direct 3x3: operand shapes / layouts not covered")
    for t in ((res,) + ((bnb.x,) if bnb is not None else ())):
        if t is not None and (tuple(t.shape) != full or not t.is_contiguous() or t.dtype != torch.bfloat16):
            raise ValueError("direct 3x3: residual / BN input must match the output")
    if bnb is not None and bnb.mask is not None and bnb.mask.numel() * 8 < y.numel():
        raise ValueError("direct 3x3: ReLU mask too short")
    if part is not None and part.numel() < _direct3x3_rows(N * H * W_) * 128:
        raise ValueError("direct 3x3: statistics buffer too short")
    args = (_lib.p(bnb.x), _lib.p(bnb.mask), _lib.p(bnb.mean), _lib.p(bnb.istd)) if bnb is not None else (0, 0, 0, 0)
    rc = _lib.fn("ddl_conv3x3")(x.data_ptr(), w.data_ptr(), y.data_ptr(), N, H, W_, C, w.shape[0], _lib.p(part),
                                _lib.p(res), *args, int(grid), _lib.stream())
    if rc < 0:
        raise RuntimeError(f"ddl_conv3x3 failed: {rc}")
    return rc


# (N, K) the streaming kernel takes: ResNet stage 2 (B whole in registers) and stage 3's wide output
# (B in 256-column slabs over workgroups that share their A rows in one XCD's L2).
# (256, 1024) is covered by the kernel (128-column slabs) but measured no faster than
# the 256x256 kernel (benchmarks/stream_bench.py: 45 vs 36 us with statistics, 51 vs 52 with the
# BN-backward epilogue: its A operand is the 103 MB side and two slabs read it twice)
# (256, 1024) -- stage 3's conv1 input gradient with the BN-backward epilogue only (forward with
# statistics stays on the general GEMMs): ResNet-50 same-box backward 14.58 vs 14.63-14.64 ms (11,723-
# 11,739 img/s; with stage 2 only: 11,488-11,506)
_STREAM_SHAPES = ((512, 128), (128, 512), (1024, 256), (256, 1024))


def _stream(a, b, c, part=None, res=None, bnb=None):
    """c[M, N] = a[M, K] b[N, K]^T by the register-B streaming kernel (csrc/kernels/stream_gemm.hip)
    when it covers the shape -- ResNet stage 2 / 3: (N, K) = (512, 128), (128, 512), (1024, 256),
    (256, 1024), bf16, contiguous; a residual only together with the BN-backward epilogue (N = 512
    / 1024).  Returns the statistics rows
    written, or None when not covered (nothing launched)."""
    if not a.is_cuda:
        return None
    M, K = a.shape
    N = b.shape[0]
    if (N, K) not in _STREAM_SHAPES or tuple(c.shape) != (M, N) or b.shape[1] != K:
        return None
    ts = [a, b, c] + ([res] if res is not None else []) + ([bnb.x] if bnb is not None else [])
    if any(t.dtype != torch.bfloat16 or not t.is_contiguous() for t in ts):
        return None
    if res is not None and (bnb is None or N not in (512, 1024) or tuple(res.shape) != (M, N)):
        return None
    if bnb is not None and bnb.x.numel() != M * N:
        return None
    if (N, K) == (256, 1024) and bnb is None:      # its forward (statistics): the general GEMMs are faster
        return None
    if part is not None and part.numel() < 256 * 2 * N:
        return None
    args = (_lib.p(bnb.x), _lib.p(bnb.mask), _lib.p(bnb.mean), _lib.p(bnb.istd)) if bnb is not None else (0, 0, 0, 0)
    rc = _lib.fn("ddl_stream_gemm")(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, _lib.p(part), _lib.p(res),
                                    *args, 0, _lib.stream())
    if rc == -1:
        return None
    if rc < 0:
        raise RuntimeError(f"ddl_stream_gemm failed: {rc}")
    return rc


def _skinny(a, b, c, part=None, res=None, bnb=None):
    """c[M, N] = a[M, K] b[N, K]^T by the streaming kernel (csrc/kernels/skinny_gemm.hip) when
    it covers the shape -- (N, K) = (256, 64) or (64, 256), bf16, contiguous, residual only
    for N = 256, BN-backward epilogue for N = 64, or for N = 256 together with the residual.
    Stage-2 shapes go to the register-B kernel (``_stream``).
    Returns the statistics rows written, or None when not covered (nothing launched)."""
    if not a.is_cuda:
        return None
    M, K = a.shape
    N = b.shape[0]
    if (N, K) in _STREAM_SHAPES:
        return _stream(a, b, c, part, res, bnb)
    if (N, K) not in ((256, 64), (64, 256)) or tuple(c.shape) != (M, N) or b.shape[1] != K:
        return None
    ts = [a, b, c] + ([res] if res is not None else []) + ([bnb.x] if bnb is not None else [])
    if any(t.dtype != torch.bfloat16 or not t.is_contiguous() for t in ts):
        return None
    if (res is not None and N != 256) or (bnb is not None and N != 64 and res is None):
        return None
    if res is not None and tuple(res.shape) != (M, N) or bnb is not None and bnb.x.numel() != M * N:
        return None
    if part is not None and part.numel() < 1024 * 2 * N:
        return None
    args = (_lib.p(bnb.x), _lib.p(bnb.mask), _lib.p(bnb.mean), _lib.p(bnb.istd)) if bnb is not None else (0, 0, 0, 0)
    rc = _lib.fn("ddl_skinny_gemm")(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, _lib.p(part), _lib.p(res),
                                    *args, 0, _lib.stream())
    if rc == -1:
        return None
    if rc < 0:
        raise RuntimeError(f"ddl_skinny_gemm failed: {rc}")
    return rc


def _direct3x3_rows(M):
    return max(stats_rows_max(M), 256)


def _fwd(x, w, stride, pad, bias=None, act=None, residual=None, stats=None):
    """Implicit-GEMM conv forward; ``stats`` (ops.bridge.BNStats) also collects the
    BatchNorm statistics partials of the output in the GEMM epilogue."""
    N, H, W_, C = x.shape
    K, R, S, _ = w.shape
    if (bias is None and act is None and residual is None and x.is_cuda
            and _direct3x3_ok(x.shape, w.shape, stride, pad)):
        y = torch.empty(N, H, W_, K, dtype=x.dtype, device=x.device)
        use_stats = stats is not None
        part = torch.empty(_direct3x3_rows(N * H * W_) * 2 * K, dtype=torch.float32, device=x.device) \
            if use_stats else None
        r = _direct3x3(x, w, y, part)
        if part is not None:
            stats.set(y, part, r)
        return y
    P = (H + 2 * pad - R) // stride + 1
    Q = (W_ + 2 * pad - S) // stride + 1
    y = torch.empty(N, P, Q, K, dtype=x.dtype, device=x.device)
    M = N * P * Q
    part = None
    kernel = None
    plain11 = R == 1 and S == 1 and stride == 1 and pad == 0
    desc = None if plain11 else _desc(N, H, W_, C, P, Q, stride, -pad, -pad, 1, 1, R, S, P, Q)
    if stats is not None and bias is None and act is None and residual is None and x.is_cuda:
        # BatchNorm statistics from the GEMM epilogue instead of a separate read pass
        # over y: nearly free in the 256x256 kernel's register epilogue and, since the
        # 128-row kernels reduce with DPP row sums too, on every tuned kernel
        # (DDL_BN_STATS_MIN_K=0 measured +0.3% on ResNet-50 over 2048; a positive value
        # restricts shorter reductions to shapes whose tuned kernel is the 256x256 one)
        if R * S * C >= STATS_MIN_K:
            use = True
        elif plain11:
            use = plan(MODE_NT, x, C, w, C, y, K, M, K, C) == "big"
        else:
            use = plan(MODE_CONV, x, 0, w, R * S * C, y, K, M, K, R * S * C, conv=desc) == "big"
        if use:
            part = torch.empty(stats_rows_max(M) * 2 * K, dtype=torch.float32, device=x.device)
            kernel = None if R * S * C >= STATS_MIN_K else "big"
    if plain11 and bias is None and act is None and residual is None and x.is_cuda:
        sk_part = torch.empty(max(stats_rows_max(M), 1024) * 2 * K, dtype=torch.float32, device=x.device) \
            if part is not None else None
        rows = _skinny(x.view(M, C), w.view(K, C), y.view(M, K), part=sk_part)
        if rows is not None:
            if part is not None:
                stats.set(y, sk_part, rows)
            return y
    if plain11:
        r = gemm(MODE_NT, x, C, w, C, y, K, M, K, C, bias=bias, act=act, residual=residual, colstats=part,
                 kernel=kernel)
    else:
        r = gemm(MODE_CONV, x, 0, w, R * S * C, y, K, M, K, R * S * C, bias=bias, act=act, residual=residual,
                 conv=desc, colstats=part, kernel=kernel)
    if part is not None:
        stats.set(y, part, r)
    return y


class _WDgradCache:
    """Every conv's dgrad weight layout of an optimizer step in one launch.

    The layouts depend only on the weights, which change once per optimizer step (the
    arena's ``generation``).  The first dgrad after a step re-lays-out every weight this
    cache has seen (``ddl_conv_w_dgrad_batch``: one launch instead of one per conv and
    parity class -- 61 per ResNet-50 step); the others find their layout ready.  A job is
    valid for the (generation, weight version) it was filled at, so in-place torch updates
    of a weight (which bump ``_version``, not the generation) still re-lay it out."""

    def __init__(self):
        self.jobs = {}          # key -> [w, rs, ss, out, filled_at]
        self.gen = None
        self.table = None       # (device int64 table, host copy, njobs)

    def _build(self):
        rows, blk = [], 0
        for w, rs, ss, out, _ in self.jobs.values():
            K, R, S, C = w.shape
            gk, gc = (K + 31) // 32, (C + 31) // 32
            r8 = list(rs) + [0] * (8 - len(rs))
            s8 = list(ss) + [0] * (8 - len(ss))
            rows.append([w.data_ptr(), out.data_ptr(), K, R, S, C, len(rs), len(ss), gk, gc, blk] + r8 + s8)
            blk += gk * gc * len(rs) * len(ss)
        host = torch.tensor(rows, dtype=torch.int64)
        self.table = (host.to(next(iter(self.jobs.values()))[0].device), host, len(rows))

    def get(self, w, rs, ss, generation):
        key = (w.data_ptr(), tuple(w.shape), tuple(rs), tuple(ss))
        if generation != self.gen:
            self.gen = generation
            if self.jobs:
                if self.table is None:
                    self._build()
                dev, host, n = self.table
                rc = _lib.fn("ddl_conv_w_dgrad_batch")(dev.data_ptr(), host.data_ptr(), n, _lib.stream())
                if rc != 0:
                    raise RuntimeError(f"ddl_conv_w_dgrad_batch failed: {rc}")
                for job in self.jobs.values():
                    job[4] = (generation, job[0]._version)
        job = self.jobs.get(key)
        stamp = (generation, w._version)
        if job is not None and job[4] == stamp:
            return job[3]
        if job is None:
            job = [w, tuple(rs), tuple(ss), None, None]
            self.jobs[key] = job
            self.table = None
        job[3] = _w_dgrad_once(w, rs, ss, job[3])
        job[4] = stamp
        return job[3]


def _w_dgrad(w, rs, ss, param=None):
    """[C, len(rs), len(ss), K] = w[:, rs][:, :, ss] transposed.  With ``param`` (the
    arena parameter ``w`` is) the layout comes from the arena's per-step batch."""
    ref = getattr(param, "_ddl_arena", None) if param is not None else None
    arena = ref() if ref is not None else None
    if arena is not None and param.data_ptr() == w.data_ptr() and w.is_cuda \
            and not torch.cuda.is_current_stream_capturing():
        cache = getattr(arena, "_ddl_wdg", None)
        if cache is None:
            cache = arena._ddl_wdg = _WDgradCache()
        return cache.get(w, rs, ss, arena.generation)
    return _w_dgrad_once(w, rs, ss)


def _w_dgrad_once(w, rs, ss, out=None):
    """[C, len(rs), len(ss), K] = w[:, rs][:, :, ss] transposed, in one native launch."""
    K, R, S, C = w.shape
    if out is None:
        out = torch.empty(C, len(rs), len(ss), K, dtype=w.dtype, device=w.device)
    ra = (ctypes.c_int * len(rs))(*rs)
    sa = (ctypes.c_int * len(ss))(*ss)
    rc = _lib.fn("ddl_conv_w_dgrad")(w.data_ptr(), out.data_ptr(), K, R, S, C, len(rs), len(ss), ra, sa,
                                     _lib.stream())
    if rc != 0:
        raise RuntimeError(f"ddl_conv_w_dgrad failed: {rc}")
    return out


def _bnb_dgrad(mode, dy, lda, wt, ldb, dx, M, C, K, conv, residual, hint):
    """The dgrad GEMM with the consumer BatchNorm's backward reduction in its epilogue
    (``hint``: ops.bridge.BNBackward) when the tuned plain kernel runs whole-K tiles;
    returns False (nothing launched) otherwise."""
    kind, splits = plan(mode, dy, lda, wt, ldb, dx, C, M, C, K, conv=conv, residual=residual, full=True)
    if splits != 1 or kind.startswith("t"):
        return False
    rows = stats_rows_max(M)
    part = torch.empty((rows + -(-rows // 32)) * 2 * C, dtype=torch.float32, device=dx.device)
    # the fused epilogue moves the balance toward memory: its kernel is tuned on its own
    nrows = gemm(mode, dy, lda, wt, ldb, dx, C, M, C, K, act="bnb", aux=hint.x, conv=conv, residual=residual,
                 colstats=part, bnb=(hint.mask, hint.mean, hint.istd))
    hint.set(dx, part, nrows)
    return True


def _dgrad(dy, w, x_shape, stride, pad, residual=None, bnb=None, param=None):
    """dx (+ ``residual``, added in the GEMM epilogue; strided convs add it in place,
    so there ``residual`` must be a tensor the caller owns)."""
    N, H, W_, C = x_shape
    K, R, S, _ = w.shape
    _, P, Q, _ = dy.shape
    bnb = bnb if (_BN_BWD_EPI and bnb is not None and dy.dtype == torch.bfloat16 and C % 8 == 0
                  and tuple(bnb.x.shape) == tuple(x_shape) and (residual is None or _BN_BWD_EPI_RES)) else None
    if R == 1 and S == 1 and stride == 1 and pad == 0:
        dx = torch.empty(N, H, W_, C, dtype=dy.dtype, device=dy.device)
        if _DGRAD_NT:   # NT against W^T (k-contiguous operands; the weight copy is tiny)
            wt = _w_dgrad(w, [0], [0], param).view(C, K)
            M = N * H * W_
            # the streaming kernel first (ResNet stage-1 shapes), then the general GEMMs
            res2 = residual.view(M, C) if residual is not None else None
            if bnb is not None:
                part = torch.empty(max(stats_rows_max(M), 1024) * 2 * C + 64 * C, dtype=torch.float32,
                                   device=dx.device)
                rows = _skinny(dy.view(M, K), wt, dx.view(M, C), part=part, res=res2, bnb=bnb)
                if rows is not None:
                    bnb.set(dx, part, rows)
                    return dx
                # residual-adding stage-1 dgrads (N = 256): the streaming kernel without the
                # BN-backward epilogue beats the general GEMM with it
                if res2 is not None and _skinny(dy.view(M, K), wt, dx.view(M, C), res=res2) is not None:
                    return dx
            elif _skinny(dy.view(M, K), wt, dx.view(M, C), res=res2) is not None:
                return dx
            if bnb is None or not _bnb_dgrad(MODE_NT, dy, K, wt, K, dx, N * H * W_, C, K, None, residual, bnb):
                gemm(MODE_NT, dy, K, wt, K, dx, C, N * H * W_, C, K, residual=residual)
        else:
            gemm(MODE_NN, dy, K, w, C, dx, C, N * H * W_, C, K, residual=residual)
        return dx
    if stride == 1:
        wt = _w_dgrad(w, list(range(R - 1, -1, -1)), list(range(S - 1, -1, -1)), param)   # flipped [C, R, S, K]
        dx = torch.empty(N, H, W_, C, dtype=dy.dtype, device=dy.device)
        if dy.is_cuda and _direct3x3_ok(dy.shape, wt.shape, 1, pad) and (bnb is not None or residual is None):
            # the direct kernel (a stride-1 3x3 dgrad is the same convolution of dy)
            if bnb is not None:
                part = torch.empty(_direct3x3_rows(N * H * W_) * 2 * C, dtype=torch.float32, device=dx.device)
                bnb.set(dx, part, _direct3x3(dy, wt, dx, part, res=residual, bnb=bnb))
            else:
                _direct3x3(dy, wt, dx)
            return dx
        desc = _desc(N, P, Q, K, H, W_, 1, -(R - 1 - pad), -(S - 1 - pad), 1, 1, R, S, H, W_)
        if bnb is None or not _bnb_dgrad(MODE_CONV, dy, 0, wt, R * S * K, dx, N * H * W_, C, R * S * K, desc,
                                         residual, bnb):
            gemm(MODE_CONV, dy, 0, wt, R * S * K, dx, C, N * H * W_, C, R * S * K, conv=desc, residual=residual)
        return dx
    # stride s: output-parity classes (a, b); taps r = a+pad (mod s)
    classes = []
    empty = False
    for a in range(stride):
        rs = [r for r in range(R) if (r - a - pad) % stride == 0]
        for b in range(stride):
            ss = [s for s in range(S) if (s - b - pad) % stride == 0]
            Ho = (H - a + stride - 1) // stride
            Wo = (W_ - b + stride - 1) // stride
            if not rs or not ss or Ho <= 0 or Wo <= 0:
                empty = True
                continue
            classes.append((a, b, rs, ss, Ho, Wo))
    if residual is not None:
        # every output pixel belongs to at most one parity class: each class GEMM adds
        # the residual in place (epilogue reads res[p] and writes dx[p] in the same
        # lane); pixels of empty classes keep the residual (their dgrad is zero)
        dx = residual if residual.is_contiguous() else residual.contiguous()
    else:
        dx = (torch.zeros if empty else torch.empty)(N, H, W_, C, dtype=dy.dtype, device=dy.device)
    probs = []
    for a, b, rs, ss, Ho, Wo in classes:
        wc = _w_dgrad(w, rs, ss, param)                                   # [C, R', S', K]
        h_off = (a + pad - rs[0]) // stride
        w_off = (b + pad - ss[0]) // stride
        Rp, Sp = len(rs), len(ss)
        probs.append((wc, N * Ho * Wo, Rp * Sp * K,
                      _desc(N, P, Q, K, Ho, Wo, 1, h_off, w_off, -1, -1, Rp, Sp, H, W_, stride, a, b)))

    def serial(out, res=None):
        for wc, Mc, Kc, desc in probs:
            gemm(MODE_CONV, dy, 0, wc, Kc, out, C, Mc, C, Kc, conv=desc, row_remap=True, residual=res)

    def multi(out, narrow):
        bs = (ctypes.c_void_p * len(probs))(*[pr[0].data_ptr() for pr in probs])
        ms = (ctypes.c_int * len(probs))(*[pr[1] for pr in probs])
        ks = (ctypes.c_int * len(probs))(*[pr[2] for pr in probs])
        cv = (ctypes.c_int * (18 * len(probs)))(*[v for pr in probs for v in pr[3]])
        rc = _lib.fn("ddl_gemm_conv_multi")(int(narrow), len(probs), dy.data_ptr(), bs, ms, ks, out.data_ptr(), C, C,
                                            cv, _lib.stream())
        if rc != 0:
            raise RuntimeError(f"ddl_gemm_conv_multi failed: {rc}")

    if residual is not None:
        serial(dx, dx)
    elif 1 < len(probs) <= 4:
        key = (tuple(dy.shape), tuple(w.shape), stride, pad)
        choice = _MULTI_CHOICE.get(key)
        if choice is None:
            # part of the reproducible kernel plan: the committed table (ops/gemm_plans.json) holds it
            # under "dgrad_path|..."; only a miss is timed here (and recorded for the next table)
            from . import _native_gemm as NG
            skey = "dgrad_path|" + "|".join(str(v) for v in key)
            planned = NG.lookup_choice(skey)
            if planned is not None and planned[0] in ("serial", "multi", "multi_narrow"):
                choice = _MULTI_CHOICE[key] = planned[0]
            else:
                choice = _pick_dgrad_path(key, serial, multi, dx)
                NG.record_choice(skey, (choice, 1))
        if choice == "serial":
            serial(dx)
        else:
            multi(dx, choice == "multi_narrow")
    else:
        serial(dx)
    return dx


_MULTI_CHOICE: dict = {}


def _pick_dgrad_path(key, serial, multi, dx):
    """Time the per-class launches against the single multi-class launch (once per shape)."""
    if not dx.is_cuda or torch.cuda.is_current_stream_capturing():
        return "serial"
    scratch = torch.empty_like(dx)
    serial(scratch)                      # also tunes the per-class GEMMs
    cands = {"serial": lambda: serial(scratch), "multi": lambda: multi(scratch, False),
             "multi_narrow": lambda: multi(scratch, True)}
    best, best_t = "serial", float("inf")
    for name, fn in cands.items():
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            fn()
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1)
        if t < best_t:
            best, best_t = name, t
    _MULTI_CHOICE[key] = best
    return best


def _direct3x3_wgrad(dy, x, dw, accumulate, grid=0):
    """dW of the direct 3x3 conv: per-workgroup fp32 partials + one reduce (conv3x3.hip)."""
    N, H, W_, C = x.shape
    if (tuple(dy.shape) != (N, H, W_, 64) or tuple(dw.shape) != (64, 3, 3, 64) or not dy.is_contiguous()
            or not x.is_contiguous() or not dw.is_contiguous() or dy.dtype != torch.bfloat16
            or x.dtype != torch.bfloat16 or dw.dtype not in (torch.bfloat16, torch.float32)):
        raise ValueError("direct 3x3 wgrad: operand shapes / layouts not covered")
    g = grid if grid > 0 else 256
    ws = torch.empty(g * 576 * 64, dtype=torch.float32, device=x.device)
    rc = _lib.fn("ddl_conv3x3_wgrad")(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), N, H, W_, C, 64, ws.data_ptr(),
                                      ws.numel(), int(accumulate), int(dw.dtype == torch.float32), int(grid),
                                      _lib.stream())
    if rc != 0:
        raise RuntimeError(f"ddl_conv3x3_wgrad failed: {rc}")
    return dw


def _wgrad(dy, x, w_shape, stride, pad, out=None):
    N, H, W_, C = x.shape
    K, R, S, _ = w_shape
    _, P, Q, _ = dy.shape
    acc = out is not None
    dw = out if acc else torch.empty(K, R, S, C, dtype=dy.dtype, device=dy.device)
    if x.is_cuda and _direct3x3_ok(x.shape, w_shape, stride, pad) and dw.is_contiguous():
        return _direct3x3_wgrad(dy, x, dw, acc)
    M = N * P * Q
    if R == 1 and S == 1 and stride == 1 and pad == 0:
        gemm(MODE_TN, dy, K, x, C, dw, C, K, C, M, accumulate=acc)
    else:
        gemm(MODE_CONVW, dy, K, x, 0, dw, R * S * C, K, R * S * C, M, accumulate=acc,
             conv=_desc(N, H, W_, C, P, Q, stride, -pad, -pad, 1, 1, R, S, P, Q))
    return dw


def _conv3_fold_ok(x, w, stride, pad) -> bool:
    """Convolutions whose backward the fused conv3 / bn3 kernel covers (csrc/kernels/conv3_bwd.hip):
    1x1, stride 1, (C_out, C_in) in bridge.CONV3_SHAPES, bf16, contiguous, on the GPU.  Stage 1's
    downsample conv has the same shape and gets a hint too; the dual BatchNorm apply never keeps it
    for its second input, so nothing is ever parked there and that conv's backward is unchanged."""
    from . import bridge as B
    K, R, S, C = w.shape
    return (B.CONV3_FUSED and R == 1 and S == 1 and stride == 1 and pad == 0 and (K, C) in B.CONV3_SHAPES
            and x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.is_contiguous()
            and w.is_contiguous() and x.numel() // C * K * 2 < 2 ** 31)


def _conv3_bwd_fused(parked, x, w, bnb, param, sink):
    """dx (the BatchNorm-backward sums of ``bnb`` from its epilogue) and dW (into ``sink`` when
    given) of a 1x1 convolution whose output gradient is the parked BatchNorm apply
    (ops.bridge.Conv3Fold): one pass over dz, the BN input, x and the BN-backward operand.
    Returns (dx, dw) -- dw None with a sink -- or None when not covered (nothing launched)."""
    dz, x3, mean3, istd3, coef = parked
    N, H, W_, C = x.shape
    K = w.shape[0]
    M = N * H * W_
    if (bnb is None or not _BN_BWD_EPI or tuple(bnb.x.shape) != tuple(x.shape) or not bnb.x.is_contiguous()
            or bnb.x.dtype != torch.bfloat16 or x3.numel() != M * K or dz.numel() != M * K
            or not dz.is_contiguous() or not x3.is_contiguous()
            or (bnb.mask is not None and bnb.mask.numel() * 8 < M * C)):
        return None
    if sink is not None and (not sink.is_contiguous() or sink.dtype not in (torch.bfloat16, torch.float32)):
        return None
    wt = _w_dgrad(w, [0], [0], param).view(C, K)
    dx = torch.empty(N, H, W_, C, dtype=x.dtype, device=x.device)
    dw = sink if sink is not None else torch.empty(K, 1, 1, C, dtype=x.dtype, device=x.device)
    G = _lib.fn("ddl_conv3_bwd_grid")(M, 0)
    part = torch.empty(max(stats_rows_max(M), 1024) * 2 * C + 64 * C, dtype=torch.float32, device=x.device)
    wpart = torch.empty(G * K * C, dtype=torch.bfloat16, device=x.device)
    rc = _lib.fn("ddl_conv3_bwd")(dz.data_ptr(), x3.data_ptr(), mean3.data_ptr(), istd3.data_ptr(), coef.data_ptr(),
                                  x.data_ptr(), bnb.x.data_ptr(), _lib.p(bnb.mask), bnb.mean.data_ptr(),
                                  bnb.istd.data_ptr(), wt.data_ptr(), dx.data_ptr(), part.data_ptr(),
                                  wpart.data_ptr(), wpart.numel(), dw.data_ptr(), int(dw.dtype == torch.float32),
                                  int(sink is not None), M, K, C, 0, _lib.stream())
    if rc == -1:
        return None
    if rc < 0:
        raise RuntimeError(f"ddl_conv3_bwd failed: {rc}")
    bnb.set(dx, part, rc)
    return dx, (None if sink is not None else dw)


def _conv3_materialise(parked, dy):
    """The gradient the ordinary dgrad / wgrad need when a BatchNorm parked its apply pass
    (ops.bridge.Conv3Fold) but the fused kernel does not run: dx3 by the apply kernel, and the
    received gradient corrected by - dz + dx3 when it is not dz itself (a second consumer, a hook)."""
    from .bridge import Conv3Fold
    dz, x3, mean3, istd3, coef = parked
    C = x3.shape[-1]
    dx3 = torch.empty_like(x3)
    _lib.call("ddl_bn_bwd_apply_coef", 1, dz.data_ptr(), x3.data_ptr(), mean3.data_ptr(), istd3.data_ptr(),
              coef.data_ptr(), x3.numel() // C, C, dx3.data_ptr())
    if Conv3Fold.is_parked(parked, dy):
        return dx3
    return (dy - dz.view_as(dy)) + dx3.view_as(dy)


class _Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, pad, bridge=None, stats=None, grad_to=None):
        ctx.w_param = w
        ctx.bridge = bridge
        ctx.grad_to = grad_to
        ctx.c3 = None
        # input is a training BatchNorm's output: its backward reduction can ride this dgrad
        # (not when the gradient is offered to a sibling conv, which adds unmasked terms)
        ctx.bnb = getattr(x, "_ddl_bnb", None) if grad_to is None else None
        x = x.contiguous()
        w = w.contiguous()
        ctx.stride, ctx.pad = stride, pad
        ctx.save_for_backward(x, w)
        y = _fwd(x, w, stride, pad, stats=stats)
        if _conv3_fold_ok(x, w, stride, pad) and y.is_contiguous():
            # the BatchNorm that consumes y may leave its backward apply pass to this conv's backward
            from .bridge import Conv3Fold
            ctx.c3 = y._ddl_c3 = Conv3Fold()
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = None
        parked = ctx.c3.take() if ctx.c3 is not None else None
        if parked is not None:
            from .bridge import Conv3Fold
            if (Conv3Fold.is_parked(parked, dy) and ctx.needs_input_grad[0] and ctx.needs_input_grad[1]
                    and ctx.bridge is None and ctx.grad_to is None):
                sink = grad_sink(ctx.w_param)
                if sink is not None and sink.shape != w.shape:
                    sink = None
                out = _conv3_bwd_fused(parked, x, w, ctx.bnb, ctx.w_param, sink)
                if out is not None:
                    ctx.bnb = None
                    if sink is not None:
                        grad_ready(ctx.w_param)
                    return out[0], out[1], None, None, None, None, None
            dy = _conv3_materialise(parked, dy)
        del parked
        fork = _lib.fork_event() if ctx.needs_input_grad[1] else None   # wgrad may start here
        if ctx.needs_input_grad[0]:
            res = ctx.bridge.take() if ctx.bridge is not None else None
            if res is not None:
                res = res.contiguous().view(x.shape)
            dx = _dgrad(dy, w, x.shape, ctx.stride, ctx.pad, residual=res, bnb=ctx.bnb, param=ctx.w_param)
            ctx.bnb = None
            if ctx.grad_to is not None and ctx.grad_to.offer(dx):
                dx = None       # the sibling conv's dgrad epilogue adds it
        if ctx.needs_input_grad[1]:
            sink = grad_sink(ctx.w_param)
            # concurrent with the dgrad just issued (DDL_WGRAD_STREAM, _lib.side_stream)
            if sink is not None and sink.shape == w.shape:
                with _lib.side_stream(dy, x, after=fork):
                    _wgrad(dy, x, w.shape, ctx.stride, ctx.pad, out=sink)
                grad_ready(ctx.w_param)
            else:
                dw = _wgrad(dy, x, w.shape, ctx.stride, ctx.pad)
        return dx, dw, None, None, None, None, None


def _s2d_input(x, pad):
    """[N, H, W, C<=4] -> space-to-depth [N, (H+2p)/2, (W+2p)/2, 16]: channel index
    (dy, dx, c) of the 2x2 pixel block, c padded to 4 (odd padded extents padded by one)."""
    N, H, W_, C = x.shape
    Hp, Wp = H + 2 * pad, W_ + 2 * pad
    Hp2, Wp2 = Hp + Hp % 2, Wp + Wp % 2
    if x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous():
        # one native pass (csrc/kernels/stem_conv.hip ddl_s2d_input) instead of a pad + a permuted copy
        xs = torch.empty(N, Hp2 // 2, Wp2 // 2, 16, dtype=x.dtype, device=x.device)
        _lib.call("ddl_s2d_input", x.data_ptr(), N, H, W_, C, pad, xs.data_ptr(), Hp2 // 2, Wp2 // 2)
        return xs
    xp = F.pad(x, (0, 4 - C, pad, pad + Wp2 - Wp, pad, pad + Hp2 - Hp))
    return xp.view(N, Hp2 // 2, 2, Wp2 // 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(N, Hp2 // 2, Wp2 // 2, 16)


def _s2d_weight(w):
    """[K, R, S, C<=4] (R, S odd) -> [K, ceil(R/2), ceil(S/2), 16] for the stride-1 conv on
    the space-to-depth input (taps past R / S are zero)."""
    K, R, S, C = w.shape
    R2, S2 = (R + 1) // 2, (S + 1) // 2
    if w.is_cuda and w.dtype == torch.bfloat16 and w.is_contiguous():
        ws = torch.empty(K, R2, S2, 16, dtype=w.dtype, device=w.device)
        _lib.call("ddl_s2d_weight", w.data_ptr(), K, R, S, C, ws.data_ptr(), R2, S2)
        return ws
    wp = F.pad(w, (0, 4 - C, 0, 2 * S2 - S, 0, 2 * R2 - R))
    return wp.view(K, R2, 2, S2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(K, R2, S2, 16)


def _s2d_weight_grad(dws, w_shape):
    """Inverse of _s2d_weight for a gradient: [K, R2, S2, 16] -> [K, R, S, C]."""
    K, R, S, C = w_shape
    R2, S2 = dws.shape[1], dws.shape[2]
    d = dws.view(K, R2, S2, 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(K, 2 * R2, 2 * S2, 4)
    return d[:, :R, :S, :C]


def _stem_wgrad_ok(xs, dy, ws_shape, w_shape) -> bool:
    """Shapes the direct stem weight-gradient kernel (stem_wgrad.hip) covers."""
    if not (xs.is_cuda and dy.is_cuda):
        return False
    N, Hx, Wx, Cs = xs.shape
    _, P, Q, K = dy.shape
    return (tuple(ws_shape) == (64, 4, 4, 16) and Cs == 16 and K == 64 and Hx == P + 3 and Wx == Q + 3
            and P % 2 == 0 and Q % 16 == 0 and 16 <= Q <= 112 and w_shape[1] <= 8 and w_shape[2] <= 8
            and w_shape[3] <= 4 and xs.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16
            and xs.is_contiguous() and dy.is_contiguous() and xs.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0)


def _stem_wgrad(xs, dy, dw, accumulate, grid=0):
    """Stem weight gradient straight from the space-to-depth operands into ``dw`` [64, R, S, C]
    (the original weight layout; += with ``accumulate``): per-workgroup fp32 partials of the
    4x4x16 taps + one reduce that also undoes the space-to-depth (stem_wgrad.hip)."""
    N, _, _, _ = xs.shape
    _, P, Q, _ = dy.shape
    K, R, S, C = dw.shape
    g = grid if grid > 0 else 256
    ws = torch.empty(g * 64 * 256, dtype=torch.float32, device=xs.device)
    rc = _lib.fn("ddl_stem_wgrad")(xs.data_ptr(), dy.data_ptr(), dw.data_ptr(), N, P, Q, K, R, S, C, ws.data_ptr(),
                                   ws.numel(), int(accumulate), int(dw.dtype == torch.float32), int(grid),
                                   _lib.stream())
    if rc != 0:
        raise RuntimeError(f"ddl_stem_wgrad failed: {rc}")
    return dw


def _stem_fwd_ok(xs, ws) -> bool:
    """Shapes the direct stem forward kernel (stem_conv.hip) covers: output P x Q with P % 4 == 0,
    Q % 16 == 0, 16 <= Q <= 112, 64 channels."""
    if not xs.is_cuda:
        return False
    N, Hx, Wx, Cs = xs.shape
    P, Q = Hx - 3, Wx - 3
    return (tuple(ws.shape) == (64, 4, 4, 16) and Cs == 16 and P >= 4 and P % 4 == 0 and Q % 16 == 0
            and 16 <= Q <= 112 and xs.dtype == torch.bfloat16 and ws.dtype == torch.bfloat16
            and xs.is_contiguous() and ws.is_contiguous() and xs.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0)


def _stem_fwd(xs, ws, stats=None, grid=0):
    """Stem forward on the space-to-depth operands (stem_conv.hip): y [N, P, Q, 64]; ``stats``
    (ops.bridge.BNStats) receives the BatchNorm partial sums of y from the kernel."""
    N, Hx, Wx, _ = xs.shape
    P, Q = Hx - 3, Wx - 3
    y = torch.empty(N, P, Q, 64, dtype=xs.dtype, device=xs.device)
    use_stats = stats is not None
    g = grid if grid > 0 else 256
    part = torch.empty(g * 2 * 64, dtype=torch.float32, device=xs.device) if use_stats else None
    rc = _lib.fn("ddl_stem_fwd")(xs.data_ptr(), ws.data_ptr(), y.data_ptr(), N, P, Q, 64, _lib.p(part), int(grid),
                                 _lib.stream())
    if rc < 0:
        raise RuntimeError(f"ddl_stem_fwd failed: {rc}")
    if part is not None:
        stats.set(y, part, rc)
    return y


class _StemConvS2D(torch.autograd.Function):
    """Stride-2 convolution of a <=4-channel image (the ResNet stem, 7x7/2 on RGB) as a
    stride-1 convolution of its 2x2 space-to-depth transform: 16 channels (16-byte
    gathers, no 3->8 channel padding) and a 4x4 kernel, so the implicit GEMM's reduction
    is 4*4*16 = 256 instead of 7*7*8 = 392.  The input gradient is never needed (image)."""

    @staticmethod
    def forward(ctx, x, w, pad, stats=None):
        ctx.w_param = w
        xs = _s2d_input(x, pad)
        ws = _s2d_weight(w.contiguous())
        ctx.save_for_backward(xs)
        ctx.ws_shape = ws.shape
        ctx.w_shape = w.shape
        # output extent: (H + 2p - R) / 2 + 1 = s2d extent - R2 + 1 for R = 2 R2 - 1
        y = _stem_fwd(xs, ws, stats) if _stem_fwd_ok(xs, ws) else _fwd(xs, ws, 1, 0, stats=stats)
        N, H, W_, _ = x.shape
        K, R, S, _ = w.shape
        P, Q = (H + 2 * pad - R) // 2 + 1, (W_ + 2 * pad - S) // 2 + 1
        return y if y.shape[1] == P and y.shape[2] == Q else y[:, :P, :Q].contiguous()

    @staticmethod
    def backward(ctx, dy):
        (xs,) = ctx.saved_tensors
        dy = dy.contiguous()
        dw = None
        if ctx.needs_input_grad[1]:
            _, P, Q, _ = dy.shape
            if xs.shape[1] - ctx.ws_shape[1] + 1 != P or xs.shape[2] - ctx.ws_shape[2] + 1 != Q:
                xs = xs[:, :P + ctx.ws_shape[1] - 1, :Q + ctx.ws_shape[2] - 1].contiguous()
            if _stem_wgrad_ok(xs, dy, ctx.ws_shape, ctx.w_shape):
                sink = grad_sink(ctx.w_param)
                if sink is not None and tuple(sink.shape) == tuple(ctx.w_shape) and sink.is_contiguous() \
                        and sink.dtype in (torch.bfloat16, torch.float32):
                    _stem_wgrad(xs, dy, sink, accumulate=True)
                    grad_ready(ctx.w_param)
                    return None, None, None, None
                dw = torch.empty(ctx.w_shape, dtype=dy.dtype, device=dy.device)
                _stem_wgrad(xs, dy, dw, accumulate=False)
                return None, dw, None, None
            dws = _wgrad(dy, xs, ctx.ws_shape, 1, 0)
            g = _s2d_weight_grad(dws, ctx.w_shape)
            sink = grad_sink(ctx.w_param)
            if sink is not None and sink.shape == g.shape:
                sink.add_(g)
                grad_ready(ctx.w_param)
            else:
                dw = g.contiguous()
        return None, dw, None, None


class _PatchEmbed(torch.autograd.Function):
    """ViT patch embedding (P x P patches, stride P) as an implicit-im2col GEMM on the
    image itself -- no patchify copy.

    NHWC ``[B, H, W, C]`` is reinterpreted (a view) as ``[B*H/P, P, W/P, P*C]``: one
    "image" per patch row, ``P`` rows of ``W/P`` super-pixels of ``P*C`` contiguous
    channels.  The patch embedding is then a ``P x 1`` stride-1 convolution of it with
    output ``[B*H/P, 1, W/P, D]`` = ``[B, patches, D]`` in patch order, and the reduction
    index ``(kh, kw*C + c)`` is exactly the ``(kh, kw, c)`` order of the weight (HF's
    ``[D, C, P, P]`` projection permuted, ``models/vit.py`` ``from_hf_state_dict``).  The
    bias rides the GEMM epilogue.  Backward: the weight gradient as the conv's wgrad
    (implicit im2col again), the bias gradient as column sums; no input gradient."""

    @staticmethod
    def forward(ctx, x, w, b, P):
        B, H, W_, C = x.shape
        D = w.shape[0]
        xv = x.contiguous().view(B * (H // P), P, W_ // P, P * C)
        wv = w.contiguous().view(D, P, 1, P * C)
        y = _fwd(xv, wv, 1, 0, bias=b)
        ctx.save_for_backward(xv)
        ctx.params = (w, b)
        ctx.wshape = wv.shape
        return y.view(B, (H // P) * (W_ // P), D)

    @staticmethod
    def backward(ctx, dy):
        (xv,) = ctx.saved_tensors
        w, b = ctx.params
        D = w.shape[0]
        dy4 = dy.contiguous().view(xv.shape[0], 1, xv.shape[2], D)
        dw = db = None
        if ctx.needs_input_grad[1]:
            sink = grad_sink(w)
            if sink is not None:
                _wgrad(dy4, xv, ctx.wshape, 1, 0, out=sink.view(ctx.wshape))
                grad_ready(w)
            else:
                dw = _wgrad(dy4, xv, ctx.wshape, 1, 0).view(w.shape)
        if b is not None and ctx.needs_input_grad[2]:
            from ._native_elementwise import colsum
            sink = grad_sink(b)
            if sink is not None:
                colsum(dy4.view(-1, D), sink, accumulate=True)
                grad_ready(b)
            else:
                db = colsum(dy4.view(-1, D), torch.empty(D, dtype=torch.float32, device=dy.device)).to(b.dtype)
        return None, dw, db, None


def patch_embed(x, w, b, P):
    """[B, H, W, C] NHWC image -> [B, (H/P)(W/P), D] patch embeddings (None if not covered)."""
    B, H, W_, C = x.shape
    if (x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or (b is not None and b.dtype != w.dtype)
            or H % P or W_ % P or (P * C) % 8 or w.shape[0] % 8 or w.shape[1] != P * P * C or x.requires_grad):
        return None
    return _PatchEmbed.apply(x, w, b, P)


def conv2d(x, w, stride, padding, bridge=None, stats=None, grad_to=None):
    from .bridge import join
    from .conv import conv2d_reference
    C = x.shape[-1]
    if (stride == 2 and C <= 4 and w.shape[1] % 2 == 1 and w.shape[2] % 2 == 1 and
            x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and w.shape[0] % 8 == 0 and
            not x.requires_grad and bridge is None):
        return _StemConvS2D.apply(x, w, padding, stats)
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or w.shape[0] % 8 or C % 8:
        # the bridge attaches to the caller's tensor (before any channel padding)
        x, bridge = join(x, bridge), None
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or w.shape[0] % 8:
        return conv2d_reference(x, w, stride, padding)
    if C % 8:
        c8 = (C + 7) // 8 * 8
        x = F.pad(x, (0, c8 - C))
        w = F.pad(w, (0, c8 - C))
        grad_to = None      # the gradient would be the padded tensor's
    return _Conv.apply(x, w, stride, padding, bridge, stats, grad_to)


def conv2d_bias_act(x, w, b, stride, padding, relu=False, residual=None):
    """Inference conv with the folded-BN bias, residual add and ReLU in the GEMM epilogue."""
    C = x.shape[-1]
    if C % 8:
        c8 = (C + 7) // 8 * 8
        x = F.pad(x, (0, c8 - C))
        w = F.pad(w, (0, c8 - C))
    res = residual.contiguous() if residual is not None else None
    return _fwd(x.contiguous(), w.contiguous(), stride, padding, bias=b, act="relu" if relu else None, residual=res)
