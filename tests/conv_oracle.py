"""An independent reference for the convolution kernels, the bound the oracle tests share, and the
case tables both test files build their operands from.

Everything here is device-agnostic torch written out from the formulas, in NHWC with ``[K, R, S, C]``
weights: nothing from ``ops/``, no ``F.conv2d``, no ``conv_transpose2d``, no autograd.  A convolution
is a loop over its taps ``(r, s)``: pad, slice, ``einsum``.  Every reference takes ``dtype`` (fp64 for
the oracle) and ``absolute=True`` for its absolute-sum companion ``A = sum |term|``: the same
computation on ``|x|``, ``|w|``, ``|res|``, ``|base|``.  The number of terms ``n`` of an element is the
same computation on all-ones operands (``ones``), so padding taps do not count.

Two tiers of checks use it (tests/test_conv_oracle_gpu.py):

exact   small-integer operands with zeros.  While every element has ``A <= 256`` (and every statistics
        sum stays below 2^24) every product, every partial sum in any order and every split-K partial
        -- even one stored in bf16 -- is an integer that bf16 and fp32 hold exactly: the kernel's
        answer must equal the oracle bit for bit.
real    randn operands rounded to bf16, per element
            a   = 2 n 2^-24 A        (fp32 accumulation in any order; 2: the MFMA's internal rounding)
            tol = a + half_ulp_out(|r| + a)     (the one rounding to the stored format)
        plus ``2^-8 A`` where split-K partials are stored in bf16 (each rounded once, sum |partial| <= A).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F      # F.pad only

from norm_oracle import _MANT, _rounder, half_ulp  # noqa: F401  (shared with the norm oracle, not copied)


# ---------------------------------------------------------------------------- helpers
def out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def ones(t):
    """All-ones operand of the shape of ``t`` (None stays None): a reference run on these counts terms."""
    return None if t is None else torch.ones(t.shape, dtype=torch.float64, device=t.device)


def _prep(t, dtype, absolute):
    t = t.to(dtype)
    return t.abs() if absolute else t


def _window(xp, r, s, P, Q, stride):
    """The pixels of the padded image that tap (r, s) pairs with output pixels (0..P-1, 0..Q-1)."""
    return xp[:, r:r + (P - 1) * stride + 1:stride, s:s + (Q - 1) * stride + 1:stride]


def half_ulp_t(v: torch.Tensor, dtype) -> torch.Tensor:
    """``half_ulp`` per element: half the spacing of ``dtype`` numbers at ``|v|`` (0 at 0)."""
    v = v.abs().double()
    _, e = torch.frexp(v)                                  # v = m 2^e, m in [0.5, 1): floor(log2 v) = e - 1
    out = torch.exp2((e - 1 - _MANT[dtype]).double())
    return torch.where(v > 0, out, torch.zeros_like(out))


def tol(ref, A, n, out_dtype, bf16_partials=False):
    """The real-valued tier's per-element bound (module docstring)."""
    a = 2.0 * n.double() * 2.0 ** -24 * A.double()
    if bf16_partials:
        a = a + 2.0 ** -8 * A.double()
    return a + half_ulp_t(ref.double().abs() + a, out_dtype)


def ratio(got, ref, A, n, out_dtype, bf16_partials=False) -> float:
    """max(|err| / tol); inf for a non-finite result, 0 where both error and tolerance are 0."""
    if not bool(torch.isfinite(got.double()).all()):
        return float("inf")
    err = (got.double() - ref.double()).abs()
    t = tol(ref, A, n, out_dtype, bf16_partials)
    q = torch.where(err > 0, err / t, torch.zeros_like(err))      # err > 0 at tol 0: inf
    return float(q.max()) if q.numel() else 0.0


# ---------------------------------------------------------------------------- convolution
def conv_fwd(x, w, stride, pad, dtype=torch.float64, res=None, bias=None, absolute=False):
    """y[n,p,q,k] = sum_(r,s,c) x[n, p*stride - pad + r, q*stride - pad + s, c] w[k,r,s,c] (+ bias[k])
    (+ res[n,p,q,k])."""
    N, H, W_, C = x.shape
    K, R, S, _ = w.shape
    P, Q = out_hw(H, W_, R, S, stride, pad)
    xf, wf = _prep(x, dtype, absolute), _prep(w, dtype, absolute)
    xp = F.pad(xf, (0, 0, pad, pad, pad, pad))
    y = torch.zeros(N, P, Q, K, dtype=dtype, device=x.device)
    for r in range(R):
        for s in range(S):
            y += torch.einsum("npqc,kc->npqk", _window(xp, r, s, P, Q, stride), wf[:, r, s])
    if bias is not None:
        y = y + _prep(bias, dtype, absolute)
    if res is not None:
        y = y + _prep(res, dtype, absolute)
    return y


def conv_dgrad(dy, w, x_shape, stride, pad, dtype=torch.float64, base=None, absolute=False):
    """dx[n,h,w,c] = sum over the (p,q,r,s) with p*stride - pad + r = h, q*stride - pad + s = w of
    dy[n,p,q,k] w[k,r,s,c], summed over k (+ base)."""
    N, H, W_, C = x_shape
    K, R, S, _ = w.shape
    _, P, Q, _ = dy.shape
    df, wf = _prep(dy, dtype, absolute), _prep(w, dtype, absolute)
    dxp = torch.zeros(N, H + 2 * pad, W_ + 2 * pad, C, dtype=dtype, device=dy.device)
    for r in range(R):
        for s in range(S):
            _window(dxp, r, s, P, Q, stride).add_(torch.einsum("npqk,kc->npqc", df, wf[:, r, s]))
    dx = dxp[:, pad:pad + H, pad:pad + W_].contiguous()
    if base is not None:
        dx = dx + _prep(base, dtype, absolute)
    return dx


def conv_wgrad(dy, x, w_shape, stride, pad, dtype=torch.float64, base=None, absolute=False):
    """dw[k,r,s,c] = sum_(n,p,q) dy[n,p,q,k] x[n, p*stride - pad + r, q*stride - pad + s, c] (+ base)."""
    K, R, S, C = w_shape
    _, P, Q, _ = dy.shape
    df, xf = _prep(dy, dtype, absolute), _prep(x, dtype, absolute)
    xp = F.pad(xf, (0, 0, pad, pad, pad, pad))
    dw = torch.zeros(K, R, S, C, dtype=dtype, device=dy.device)
    for r in range(R):
        for s in range(S):
            dw[:, r, s] = torch.einsum("npqk,npqc->kc", df, _window(xp, r, s, P, Q, stride))
    if base is not None:
        dw = dw + _prep(base, dtype, absolute)
    return dw


# ---------------------------------------------------------------------------- BatchNorm epilogues
def bn_stats_rows(y, dtype=torch.float64, absolute=False):
    """(sum y, sum y^2) per channel of a stored output (the absolute companion of sum y is sum |y|)."""
    yf = _prep(y, dtype, absolute).reshape(-1, y.shape[-1])
    return yf.sum(0), (yf * yf).sum(0)


def pack_mask(bits: torch.Tensor) -> torch.Tensor:
    """bool bits (element order) -> uint8, bit i of byte b = element 8 b + i."""
    b = bits.reshape(-1, 8).to(torch.int32)
    wts = (2 ** torch.arange(8, device=bits.device, dtype=torch.int32))
    return (b * wts).sum(1).to(torch.uint8)


def bnb_epilogue(v, mask, dtype=torch.float64):
    """dz = v * mask for v = conv (+ res) already in ``dtype`` (``mask``: bool bits or None)."""
    return v if mask is None else v * mask.to(dtype)


def bnb_sums(dz, aux, mean, istd, dtype=torch.float64, absolute=False):
    """(sum dz, sum dz (x - mean) istd) per channel; absolute: (sum |dz|, sum |dz| (|x| + |mean|) |istd|),
    every term of the expanded formula."""
    C = dz.shape[-1]
    d, x = _prep(dz, dtype, absolute).reshape(-1, C), _prep(aux, dtype, absolute).reshape(-1, C)
    m, i = _prep(mean, dtype, absolute), _prep(istd, dtype, absolute)
    if absolute:
        return d.sum(0), (d * (x + m)).sum(0) * i
    return d.sum(0), (d * (x - m)).sum(0) * i


# ---------------------------------------------------------------------------- space-to-depth stem
def stem_fwd(x, w, dtype=torch.float64, absolute=False):
    """The original stem: 7x7, stride 2, pad 3, ``x [N,H,W,3]``, ``w [64,7,7,3]``."""
    return conv_fwd(x, w, 2, 3, dtype, absolute=absolute)


def stem_wgrad(dy, x, dtype=torch.float64, base=None, absolute=False):
    """The original stem's weight gradient in the ``[64,7,7,3]`` layout."""
    return conv_wgrad(dy, x, (dy.shape[-1], 7, 7, x.shape[-1]), 2, 3, dtype, base, absolute)


def s2d_input(x, pad):
    """[N,H,W,C<=4] -> the padded image's 2x2 space-to-depth [N, ceil((H+2p)/2), ceil((W+2p)/2), 16]:
    channel (dy, dx, c) = dy*8 + dx*4 + c, c padded to 4 with zeros."""
    N, H, W_, C = x.shape
    Hp, Wp = H + 2 * pad, W_ + 2 * pad
    H2, W2 = (Hp + 1) // 2, (Wp + 1) // 2
    xp = torch.zeros(N, 2 * H2, 2 * W2, 4, dtype=x.dtype, device=x.device)
    xp[:, pad:pad + H, pad:pad + W_, :C] = x
    out = torch.zeros(N, H2, W2, 16, dtype=x.dtype, device=x.device)
    for dy in range(2):
        for dx in range(2):
            out[..., dy * 8 + dx * 4:dy * 8 + dx * 4 + 4] = xp[:, dy::2, dx::2]
    return out


def s2d_weight(w):
    """[K,R,S,C<=4] -> [K, ceil(R/2), ceil(S/2), 16]: tap (2 r2 + dy, 2 s2 + dx), zeros past R / S / C."""
    K, R, S, C = w.shape
    R2, S2 = (R + 1) // 2, (S + 1) // 2
    out = torch.zeros(K, R2, S2, 16, dtype=w.dtype, device=w.device)
    for r in range(R):
        for s in range(S):
            o = (r % 2) * 8 + (s % 2) * 4
            out[:, r // 2, s // 2, o:o + C] = w[:, r, s]
    return out


def un_s2d_weight_grad(dws, w_shape):
    """The gradient of the original weight from the space-to-depth one: dw[k,r,s,c] =
    dws[k, r//2, s//2, (r%2)*8 + (s%2)*4 + c] (taps past R / S and the channels past C drop out)."""
    K, R, S, C = w_shape
    dw = torch.zeros(K, R, S, C, dtype=dws.dtype, device=dws.device)
    for r in range(R):
        for s in range(S):
            o = (r % 2) * 8 + (s % 2) * 4
            dw[:, r, s] = dws[:, r // 2, s // 2, o:o + C]
    return dw


# ---------------------------------------------------------------------------- patch embedding
def patch_embed_fwd(x, w, b, P, dtype=torch.float64, absolute=False):
    """[B,H,W,C] image, [D, P*P*C] weight in (kh, kw, c) order, bias -> [B, (H/P)(W/P), D]."""
    B, H, W_, C = x.shape
    D = w.shape[0]
    y = conv_fwd(x, w.reshape(D, P, P, C), P, 0, dtype, bias=b, absolute=absolute)
    return y.reshape(B, (H // P) * (W_ // P), D)


def patch_embed_grads(dy, x, P, dtype=torch.float64, absolute=False):
    """(dW [D, P*P*C], db [D]) of the patch embedding."""
    B, H, W_, C = x.shape
    D = dy.shape[-1]
    dy4 = dy.reshape(B, H // P, W_ // P, D)
    dw = conv_wgrad(dy4, x, (D, P, P, C), P, 0, dtype, absolute=absolute).reshape(D, P * P * C)
    return dw, _prep(dy, dtype, absolute).reshape(-1, D).sum(0)


# ---------------------------------------------------------------------------- operands
EXACT_A_MAX = 256.0
EXACT_STAT_MAX = 2.0 ** 24
LAMBDA = 40.0       # nonzero terms aimed at per element in the exact tier: E[A] ~ 3 LAMBDA = 120 with a
#                     standard deviation of ~22 (256 is 6 sigma away), P(sum == 0) ~ 2 %


def density(nterms: int) -> float:
    """Per-operand density at which an element of ``nterms`` products keeps ~LAMBDA nonzero ones."""
    return min(1.0, math.sqrt(LAMBDA / max(nterms, 1)))


def gen(seed: int) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def int_tensor(g, shape, vmax, dens, dtype=torch.bfloat16):
    """Integers of {-vmax..vmax} \\ {0}, kept with probability ``dens`` (zeros otherwise)."""
    mag = torch.randint(1, vmax + 1, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    keep = torch.rand(shape, generator=g) < dens
    return (mag * sign * keep).to(dtype)


def real_tensor(g, shape, scale=1.0, dtype=torch.bfloat16):
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def operand(tier, g, shape, vmax, dens, scale=1.0, dtype=torch.bfloat16):
    """One operand of a case: small integers at ``dens`` (exact tier) or randn * scale (real tier)."""
    if tier == "exact":
        return int_tensor(g, shape, vmax, dens, dtype)
    return real_tensor(g, shape, scale, dtype)


TIERS = ("exact", "real")

# ---- direct 3x3: ((N, H, W), grid)
DIRECT_SHAPES = [((1, 1, 56), 0), ((1, 2, 64), 0), ((2, 3, 56), 0), ((3, 5, 64), 2), ((1, 13, 56), 1),
                 ((2, 4, 56), 0)]


def direct_case(tier, shape, seed=0):
    """Operands of one direct-3x3 case: x / dy (conv input), w, wt (for the epilogue test: any
    [64,3,3,64]), res, aux, mask bits, mean, istd, and the wgrad pair (xg, dyg) with its bases."""
    N, H, W_ = shape
    g = gen(1000 + seed + N * 10000 + H * 100 + W_)
    full = (N, H, W_, 64)
    d = density(9 * 64)
    o = {"x": operand(tier, g, full, 3, d), "w": operand(tier, g, (64, 3, 3, 64), 2, d, 0.05),
         "res": operand(tier, g, full, 3, 1.0), "aux": operand(tier, g, full, 3, 1.0),
         "bits": torch.rand(full, generator=g) > 0.3}
    if tier == "exact":
        o["mean"] = torch.randint(-2, 3, (64,), generator=g).float()
        o["istd"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (64,), generator=g)]
    else:
        o["mean"] = torch.randn(64, generator=g) * 0.1
        o["istd"] = torch.rand(64, generator=g) + 0.5
    dg = density(N * H * W_)
    o["xg"], o["dyg"] = operand(tier, g, full, 2, dg), operand(tier, g, full, 2, dg)
    o["base"] = operand(tier, g, (64, 3, 3, 64), 3, 1.0, 1.0, torch.float32)      # bf16-representable in both tiers
    if tier == "real":
        o["base"] = o["base"].bfloat16().float()
    return o


# ---- implicit GEMM: (N, H, W, C, K, R, S, stride, pad)
IGEMM_SHAPES = [
    (2, 5, 7, 8, 8, 3, 3, 1, 1),
    (3, 7, 9, 8, 16, 3, 3, 1, 1),
    (2, 7, 5, 8, 16, 3, 3, 1, 0),
    (1, 9, 11, 24, 40, 3, 3, 2, 1),
    (1, 6, 6, 8, 16, 5, 5, 2, 2),
    (2, 8, 8, 16, 64, 1, 1, 2, 0),
    (1, 4, 4, 8, 8, 7, 7, 2, 3),
    (1, 6, 9, 8, 16, 3, 1, 1, 0),
]
# the smallest shape of the 4-wave weight-gradient kernel's contract (256 | K, 128 | R S C, 128 | N P Q):
# a 2x2 kernel with padding taps over 2 * 8 * 8 output pixels
WG_SHAPE = (2, 7, 7, 32, 256, 2, 2, 1, 1)
FWD_KINDS = (None, "big", "small", "narrow", "duo")
WGRAD_KINDS = (None, "big", "small", "narrow", "tnarrow", "duo")
DGRAD_PATHS = ("serial", "multi", "multi_narrow")


def igemm_case(tier, case, seed=0):
    """x, w, dy, the dgrad residual and the wgrad operands / base of one implicit-GEMM case."""
    N, H, W_, C, K, R, S, stride, pad = case
    P, Q = out_hw(H, W_, R, S, stride, pad)
    g = gen(2000 + seed + sum(v * (i + 3) for i, v in enumerate(case)))
    df, dd = density(R * S * C), density(-(-R // stride) * -(-S // stride) * K)
    dg = density(N * P * Q)
    o = {"x": operand(tier, g, (N, H, W_, C), 3, df), "w": operand(tier, g, (K, R, S, C), 2, df),
         "dy": operand(tier, g, (N, P, Q, K), 3, dd), "wd": operand(tier, g, (K, R, S, C), 2, dd),
         "res": operand(tier, g, (N, H, W_, C), 3, 1.0),
         "xg": operand(tier, g, (N, H, W_, C), 2, dg), "dyg": operand(tier, g, (N, P, Q, K), 2, dg),
         "base": operand(tier, g, (K, R, S, C), 3, 1.0).float()}
    return o


# ---- stem (space-to-depth operands): ((N, P, Q), grid)
STEM_FWD_SHAPES = [((1, 4, 16), 0), ((2, 8, 48), 3), ((1, 12, 112), 1)]
STEM_WGRAD_SHAPES = [((1, 2, 16), 0), ((3, 6, 64), 4), ((1, 4, 112), 0)]
STEM_PATH_SHAPES = [(2, 32, 32), (2, 13, 37)]      # (N, H, W) of the whole path


def stem_case(tier, shape, seed=0):
    """Space-to-depth operands of the direct stem kernels: xs [N,P+3,Q+3,16] and ws [64,4,4,16] dense in
    all 16 channels and all 16 taps (the forward kernel must use them all; the weight gradient's
    un-space-to-depth must drop the eighth tap and the fourth channel), dy and the fp32 base."""
    N, P, Q = shape
    g = gen(3000 + seed + N * 100000 + P * 1000 + Q)
    d, dg = density(256), density(N * P * Q)
    return {"xs": operand(tier, g, (N, P + 3, Q + 3, 16), 3, d), "ws": operand(tier, g, (64, 4, 4, 16), 2, d, 0.1),
            "xg": operand(tier, g, (N, P + 3, Q + 3, 16), 2, dg), "dyg": operand(tier, g, (N, P, Q, 64), 2, dg),
            "base": operand(tier, g, (64, 7, 7, 3), 3, 1.0).float()}


def stem_path_case(tier, shape, seed=0):
    N, H, W_ = shape
    P, Q = out_hw(H, W_, 7, 7, 2, 3)
    g = gen(4000 + seed + H * 100 + W_)
    d, dg = density(147), density(N * P * Q)
    return {"x": operand(tier, g, (N, H, W_, 3), 3, d), "w": operand(tier, g, (64, 7, 7, 3), 2, d, 0.1),
            "xg": operand(tier, g, (N, H, W_, 3), 2, dg), "dyg": operand(tier, g, (N, P, Q, 64), 2, dg)}


# ---- patch embedding: (B, H, W, C, P, D)
PATCH_SHAPE = (2, 16, 16, 3, 8, 24)


def patch_case(tier, seed=0):
    B, H, W_, C, P, D = PATCH_SHAPE
    g = gen(5000 + seed)
    d, dg = density(P * P * C), density(B * (H // P) * (W_ // P))
    return {"x": operand(tier, g, (B, H, W_, C), 3, d), "w": operand(tier, g, (D, P * P * C), 2, d, 0.1),
            "b": operand(tier, g, (D,), 3, 1.0), "xg": operand(tier, g, (B, H, W_, C), 2, dg),
            "dy": operand(tier, g, (B, (H // P) * (W_ // P), D), 2, dg)}


# ---------------------------------------------------------------------------- references per case
# One table of (oracle value, absolute sum A, term count n) per check of a case, computed once on the
# CPU in fp64 and shared: the GPU tests compare kernels with it, the CPU tests check that every
# exact-tier entry meets the exact tier's conditions.
import functools  # noqa: E402
from types import SimpleNamespace  # noqa: E402


def _triple(f, mask=None):
    """f(T, absolute) -> Ref: T maps every operand (identity, or ``ones`` for the term count)."""
    r = SimpleNamespace(ref=f(lambda t: t, False), A=f(lambda t: t, True), n=f(ones, False), stats=None)
    if mask is not None:
        m = mask.to(torch.float64)
        r.ref, r.A, r.n = r.ref * m, r.A * m, r.n * m
    return r


@functools.lru_cache(maxsize=None)
def direct_refs(tier, shape):
    N, H, W_ = shape
    o = direct_case(tier, shape)
    xs, ws = (N, H, W_, 64), (64, 3, 3, 64)
    refs = {"fwd": _triple(lambda T, a: conv_fwd(T(o["x"]), T(o["w"]), 1, 1, absolute=a))}
    refs["fwd"].stats = (bn_stats_rows(refs["fwd"].ref), bn_stats_rows(refs["fwd"].ref, absolute=True))
    for with_res in (False, True):
        for with_mask in (False, True):
            r = _triple(lambda T, a: conv_fwd(T(o["x"]), T(o["w"]), 1, 1, res=T(o["res"]) if with_res else None,
                                              absolute=a), o["bits"] if with_mask else None)
            r.stats = (bnb_sums(r.ref, o["aux"], o["mean"], o["istd"]),
                       bnb_sums(r.ref, o["aux"], o["mean"], o["istd"], absolute=True))
            refs[f"bnb_res{int(with_res)}_mask{int(with_mask)}"] = r
    refs["dgrad"] = _triple(lambda T, a: conv_dgrad(T(o["x"]), T(o["w"]), xs, 1, 1, absolute=a))
    refs["wgrad"] = _triple(lambda T, a: conv_wgrad(T(o["dyg"]), T(o["xg"]), ws, 1, 1, absolute=a))
    refs["wgrad_acc"] = _triple(lambda T, a: conv_wgrad(T(o["dyg"]), T(o["xg"]), ws, 1, 1, base=T(o["base"]),
                                                        absolute=a))
    return o, refs


@functools.lru_cache(maxsize=None)
def igemm_refs(tier, case):
    N, H, W_, C, K, R, S, stride, pad = case
    o = igemm_case(tier, case)
    xs, ws = (N, H, W_, C), (K, R, S, C)
    refs = {"fwd": _triple(lambda T, a: conv_fwd(T(o["x"]), T(o["w"]), stride, pad, absolute=a)),
            "dgrad": _triple(lambda T, a: conv_dgrad(T(o["dy"]), T(o["wd"]), xs, stride, pad, absolute=a)),
            "wgrad": _triple(lambda T, a: conv_wgrad(T(o["dyg"]), T(o["xg"]), ws, stride, pad, absolute=a)),
            "wgrad_acc": _triple(lambda T, a: conv_wgrad(T(o["dyg"]), T(o["xg"]), ws, stride, pad, base=T(o["base"]),
                                                         absolute=a))}
    if stride > 1:
        refs["dgrad_res"] = _triple(lambda T, a: conv_dgrad(T(o["dy"]), T(o["wd"]), xs, stride, pad,
                                                            base=T(o["res"]), absolute=a))
    return o, refs


@functools.lru_cache(maxsize=None)
def stem_refs(tier, shape):
    o = stem_case(tier, shape)
    s2, orig = (64, 4, 4, 16), (64, 7, 7, 3)
    refs = {"fwd": _triple(lambda T, a: conv_fwd(T(o["xs"]), T(o["ws"]), 1, 0, absolute=a))}
    refs["fwd"].stats = (bn_stats_rows(refs["fwd"].ref), bn_stats_rows(refs["fwd"].ref, absolute=True))
    refs["wgrad"] = _triple(lambda T, a: un_s2d_weight_grad(
        conv_wgrad(T(o["dyg"]), T(o["xg"]), s2, 1, 0, absolute=a), orig))
    refs["wgrad_acc"] = _triple(lambda T, a: un_s2d_weight_grad(
        conv_wgrad(T(o["dyg"]), T(o["xg"]), s2, 1, 0, absolute=a), orig) + _prep(T(o["base"]), torch.float64, a))
    return o, refs


@functools.lru_cache(maxsize=None)
def stem_path_refs(tier, shape):
    o = stem_path_case(tier, shape)
    return o, {"fwd": _triple(lambda T, a: stem_fwd(T(o["x"]), T(o["w"]), absolute=a)),
               "wgrad": _triple(lambda T, a: stem_wgrad(T(o["dyg"]), T(o["xg"]), absolute=a))}


@functools.lru_cache(maxsize=None)
def patch_refs(tier):
    o = patch_case(tier)
    P = PATCH_SHAPE[4]
    return o, {"fwd": _triple(lambda T, a: patch_embed_fwd(T(o["x"]), T(o["w"]), T(o["b"]), P, absolute=a)),
               "dw": _triple(lambda T, a: patch_embed_grads(T(o["dy"]), T(o["xg"]), P, absolute=a)[0]),
               "db": _triple(lambda T, a: patch_embed_grads(T(o["dy"]), T(o["xg"]), P, absolute=a)[1])}


def all_exact_refs():
    """(label, Ref) of every exact-tier check the GPU file runs."""
    for shape, _ in DIRECT_SHAPES:
        for k, r in direct_refs("exact", shape)[1].items():
            yield f"direct{shape}:{k}", r
    for case in IGEMM_SHAPES + [WG_SHAPE]:
        for k, r in igemm_refs("exact", case)[1].items():
            if case is WG_SHAPE and not k.startswith("wgrad"):
                continue
            yield f"igemm{case}:{k}", r
    for shape in sorted({s for s, _ in STEM_FWD_SHAPES} | {s for s, _ in STEM_WGRAD_SHAPES}):
        for k, r in stem_refs("exact", shape)[1].items():
            yield f"stem{shape}:{k}", r
    for shape in STEM_PATH_SHAPES:
        for k, r in stem_path_refs("exact", shape)[1].items():
            yield f"stem_path{shape}:{k}", r
    for k, r in patch_refs("exact")[1].items():
        yield f"patch:{k}", r
