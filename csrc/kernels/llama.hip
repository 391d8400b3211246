// Llama-family memory-bound kernels: RMSNorm, RoPE + grouped-query pack, SwiGLU (forward and backward).
//
// All of them: bf16 storage, fp32 arithmetic, every stored element rounded once, 16 bytes per lane and
// access, grids sized from the host-known shapes alone, no atomics (fixed summation orders: two runs
// give the same bits).
#include "ddl_common.h"

namespace {

__device__ __forceinline__ void unpack8(const uint4& u, float* v) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = lo_f(w[i]);
        v[2 * i + 1] = hi_f(w[i]);
    }
}
__device__ __forceinline__ uint4 pack8(const float* v) {
    uint4 u;
    u.x = pack2bf(v[0], v[1]);
    u.y = pack2bf(v[2], v[3]);
    u.z = pack2bf(v[4], v[5]);
    u.w = pack2bf(v[6], v[7]);
    return u;
}
__device__ __forceinline__ uint4 ld16(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void st16(bf16_t* p, const uint4& u) { *reinterpret_cast<uint4*>(p) = u; }

// ------------------------------------------------------------------------------------------ RMSNorm
// One wave per row, four rows per block.  A pass covers 512 columns (64 lanes x 8); NP passes cover the
// row, lanes past H idle in a ragged last pass (and all but H / 8 lanes when H < 512).  The row stays in
// registers as raw bf16 between the sum of squares and the scaling.
template <int NP>
__global__ __launch_bounds__(256) void rmsnorm_fwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                     bf16_t* __restrict__ y, float* __restrict__ save_rstd, long rows,
                                                     int H, float eps) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                 // wave-uniform: the DPP sum below sees all 64 lanes
    uint4 xr[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int col = 512 * k + 8 * lane;
        xr[k] = col < H ? ld16(x + row * H + col) : make_uint4(0, 0, 0, 0);
    }
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        float v[8];
        unpack8(xr[k], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += v[j] * v[j];
    }
    const float rstd = rsqrtf(wave_sum_dpp(ss) / H + eps);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int col = 512 * k + 8 * lane;
        if (col < H) {
            float v[8], g[8], o[8];
            unpack8(xr[k], v);
            load8(w + col, g);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = v[j] * rstd * g[j];
            store8(y + row * H + col, o);
        }
    }
    if (lane == 0) save_rstd[row] = rstd;
}

// dx per row and one fp32 partial row of dw per block.  A block owns rows_per_blk consecutive rows, its
// four waves take them round-robin and keep their share of dw = sum dy * xhat in registers; the waves'
// shares are then summed through LDS in wave order 0..3 (fixed) and written as the block's partial row.
// ADD: `add` (the gradient of x from its other consumer, the residual branch) joins dx before the one
// rounding.
template <int NP, bool ADD>
__global__ __launch_bounds__(256) void rmsnorm_bwd_k(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                     const bf16_t* __restrict__ w, const float* __restrict__ rstd,
                                                     const bf16_t* __restrict__ add, bf16_t* __restrict__ dx,
                                                     float* __restrict__ part, long rows, int H, int rows_per_blk) {
    __shared__ float s_acc[NP * 512];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float dw[NP][8];
#pragma unroll
    for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) dw[k][j] = 0.f;
    const long r0 = (long)blockIdx.x * rows_per_blk;
    const long r1 = min(rows, r0 + rows_per_blk);
    for (long row = r0 + wv; row < r1; row += 4) {      // wave-uniform
        const float rs = rstd[row];
        uint4 xr[NP], dr[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int col = 512 * k + 8 * lane;
            const bool in = col < H;
            xr[k] = in ? ld16(x + row * H + col) : make_uint4(0, 0, 0, 0);
            dr[k] = in ? ld16(dy + row * H + col) : make_uint4(0, 0, 0, 0);
        }
        // sum(g * x), g = dy * w: mean(g * xhat) = rstd * that / H
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int col = 512 * k + 8 * lane;
            if (col < H) {
                float xv[8], d[8], g[8];
                unpack8(xr[k], xv);
                unpack8(dr[k], d);
                load8(w + col, g);
#pragma unroll
                for (int j = 0; j < 8; ++j) s += d[j] * g[j] * xv[j];
            }
        }
        const float m = wave_sum_dpp(s) * rs / H;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int col = 512 * k + 8 * lane;
            if (col < H) {
                float xv[8], d[8], g[8], o[8];
                unpack8(xr[k], xv);
                unpack8(dr[k], d);
                load8(w + col, g);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xh = xv[j] * rs;
                    o[j] = rs * (d[j] * g[j] - xh * m);
                    dw[k][j] += d[j] * xh;
                }
                if constexpr (ADD) {
                    float a[8];
                    load8(add + row * H + col, a);
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[j] += a[j];
                }
                store8(dx + row * H + col, o);
            }
        }
    }
    for (int t = 0; t < 4; ++t) {
        if (wv == t) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                float* a = s_acc + 512 * k + 8 * lane;
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] = t == 0 ? dw[k][j] : a[j] + dw[k][j];
            }
        }
        __syncthreads();
    }
    for (int c = threadIdx.x; c < H; c += 256) part[(long)blockIdx.x * H + c] = s_acc[c];
}

// dw = the column sums of the partial rows, in colsum64's fixed order; rounded once.
__global__ __launch_bounds__(1024) void rmsnorm_dw_k(const float* __restrict__ part, int nblk, int H,
                                                     bf16_t* __restrict__ dw) {
    __shared__ float red[1024];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const float s = colsum64(part, nblk, H, c, c < H, red);
    if (threadIdx.x < 64 && c < H) dw[c] = f2bf(s);
}

// --------------------------------------------------------------------------------- RoPE + GQA pack
// Work item: 8 columns i0 .. i0+7 (i0 = 8 j, j < 4) of one head of the fused projection together with
// their rotation partners i0+32 .. i0+39: two 16-byte loads.  A block takes `tpb` consecutive tokens,
// (H + 2 Hkv) * 4 items each.  The table row of position s is [cos 0..31 | sin 0..31] in fp32.
struct RopeDims {
    int H, Hkv, G, S, tpb;
    FastDiv items, seq;      // items per token; S
};

__device__ __forceinline__ void rope_cs(const float* __restrict__ tab, uint32_t s, int j, float* c, float* sn) {
    load8(tab + (long)s * 64 + 8 * j, c);
    load8(tab + (long)s * 64 + 32 + 8 * j, sn);
}

// POS: token (b, s) is rotated by table row pos[b, s] (packed rows: the position inside its document) in
// place of row s; the value is the caller's contract and is clamped into the table all the same.
template <bool POS>
__global__ __launch_bounds__(256) void rope_qkv_fwd_k(const bf16_t* __restrict__ in, const float* __restrict__ tab,
                                                      bf16_t* __restrict__ out, long ntok, RopeDims d,
                                                      const int* __restrict__ pos, uint32_t n_pos) {
    const long tok0 = (long)blockIdx.x * d.tpb;
    const int nt = (int)min((long)d.tpb, ntok - tok0);
    const uint32_t s0 = (uint32_t)(tok0 % d.S);
    const uint32_t n = (uint32_t)nt * d.items.d;
    const long in_w = (long)(d.H + 2 * d.Hkv) * 64, out_w = 3L * d.H * 64;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const uint32_t lt = fdiv(i, d.items), r = i - lt * d.items.d;
        const int hin = r >> 2, j = r & 3;
        const bf16_t* src = in + (tok0 + lt) * in_w + hin * 64 + 8 * j;
        uint4 a = ld16(src), b = ld16(src + 32);
        bf16_t* o = out + (tok0 + lt) * out_w + 8 * j;
        if (hin >= d.H + d.Hkv) {                         // v: copied as it is to its G query-head slots
            o += (2L * d.H + (long)(hin - d.H - d.Hkv) * d.G) * 64;
            for (int g = 0; g < d.G; ++g) { st16(o + g * 64, a); st16(o + g * 64 + 32, b); }
            continue;
        }
        const uint32_t st = s0 + lt;
        const uint32_t s = POS ? min((uint32_t)pos[tok0 + lt], n_pos - 1) : st - fdiv(st, d.seq) * d.seq.d;
        float c[8], sn[8], x1[8], x2[8], o1[8], o2[8];
        rope_cs(tab, s, j, c, sn);
        unpack8(a, x1);
        unpack8(b, x2);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            o1[e] = x1[e] * c[e] - x2[e] * sn[e];
            o2[e] = x2[e] * c[e] + x1[e] * sn[e];
        }
        a = pack8(o1);
        b = pack8(o2);
        if (hin < d.H) {
            o += (long)hin * 64;
            st16(o, a);
            st16(o + 32, b);
        } else {
            o += ((long)d.H + (long)(hin - d.H) * d.G) * 64;
            for (int g = 0; g < d.G; ++g) { st16(o + g * 64, a); st16(o + g * 64 + 32, b); }
        }
    }
}

// Backward, the same items over the fused projection's gradient: dq rotated by the transpose, dk and dv
// summed over their group's G query-head slots in fp32 (slot order), the dk sum rotated once.
template <bool POS>
__global__ __launch_bounds__(256) void rope_qkv_bwd_k(const bf16_t* __restrict__ dout, const float* __restrict__ tab,
                                                      bf16_t* __restrict__ din, long ntok, RopeDims d,
                                                      const int* __restrict__ pos, uint32_t n_pos) {
    const long tok0 = (long)blockIdx.x * d.tpb;
    const int nt = (int)min((long)d.tpb, ntok - tok0);
    const uint32_t s0 = (uint32_t)(tok0 % d.S);
    const uint32_t n = (uint32_t)nt * d.items.d;
    const long in_w = (long)(d.H + 2 * d.Hkv) * 64, out_w = 3L * d.H * 64;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const uint32_t lt = fdiv(i, d.items), r = i - lt * d.items.d;
        const int hin = r >> 2, j = r & 3;
        const bf16_t* src = dout + (tok0 + lt) * out_w + 8 * j;
        bf16_t* dst = din + (tok0 + lt) * in_w + hin * 64 + 8 * j;
        int ng = 1;
        if (hin < d.H) {
            src += (long)hin * 64;
        } else {
            ng = d.G;
            src += hin < d.H + d.Hkv ? ((long)d.H + (long)(hin - d.H) * d.G) * 64
                                     : (2L * d.H + (long)(hin - d.H - d.Hkv) * d.G) * 64;
        }
        float g1[8], g2[8];
        unpack8(ld16(src), g1);
        unpack8(ld16(src + 32), g2);
        for (int g = 1; g < ng; ++g) {
            float t1[8], t2[8];
            unpack8(ld16(src + g * 64), t1);
            unpack8(ld16(src + g * 64 + 32), t2);
#pragma unroll
            for (int e = 0; e < 8; ++e) { g1[e] += t1[e]; g2[e] += t2[e]; }
        }
        if (hin < d.H + d.Hkv) {
            const uint32_t st = s0 + lt;
            const uint32_t s = POS ? min((uint32_t)pos[tok0 + lt], n_pos - 1) : st - fdiv(st, d.seq) * d.seq.d;
            float c[8], sn[8];
            rope_cs(tab, s, j, c, sn);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float a = g1[e] * c[e] + g2[e] * sn[e];
                const float b = g2[e] * c[e] - g1[e] * sn[e];
                g1[e] = a;
                g2[e] = b;
            }
        }
        st16(dst, pack8(g1));
        st16(dst + 32, pack8(g2));
    }
}

// ------------------------------------------------------------------------------------------ SwiGLU
// sigmoid(g) = 1 / (1 + 2^(-g log2 e)): the exponential saturates to 0 or +inf at the ends of the range
// and the reciprocal of +inf is 0, so no inf - inf or inf * 0 arises for any finite gate.
__device__ __forceinline__ float sigmoid_f(float g) {
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(g * -1.4426950408889634f));
}

// One thread per 8 columns of one row of z; n8 = rows * I / 8 < 2^31.
__global__ __launch_bounds__(256) void swiglu_fwd_k(const bf16_t* __restrict__ gu, bf16_t* __restrict__ z, uint32_t n8,
                                                    int I, FastDiv i8) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n8) return;
    const uint32_t row = fdiv(t, i8), c = (t - row * i8.d) * 8;
    float g[8], u[8], o[8];
    load8(gu + (long)row * 2 * I + c, g);
    load8(gu + (long)row * 2 * I + I + c, u);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = g[j] * sigmoid_f(g[j]) * u[j];
    store8(z + (long)row * I + c, o);
}

__global__ __launch_bounds__(256) void swiglu_bwd_k(const bf16_t* __restrict__ gu, const bf16_t* __restrict__ dz,
                                                    bf16_t* __restrict__ dgu, uint32_t n8, int I, FastDiv i8) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n8) return;
    const uint32_t row = fdiv(t, i8), c = (t - row * i8.d) * 8;
    float g[8], u[8], d[8], dg[8], du[8];
    load8(gu + (long)row * 2 * I + c, g);
    load8(gu + (long)row * 2 * I + I + c, u);
    load8(dz + (long)row * I + c, d);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float sg = sigmoid_f(g[j]);
        dg[j] = d[j] * u[j] * sg * (1.f + g[j] * (1.f - sg));
        du[j] = d[j] * (g[j] * sg);
    }
    store8(dgu + (long)row * 2 * I + c, dg);
    store8(dgu + (long)row * 2 * I + I + c, du);
}

int np_for(int H) {
    const int np = (H + 511) / 512;
    return np <= 1 ? 1 : np <= 2 ? 2 : np <= 4 ? 4 : np <= 8 ? 8 : 16;
}

bool rope_dims(long B, long S, int H, int Hkv, RopeDims& d) {
    if (B < 1 || S < 1 || S >= (1L << 30) || Hkv < 1 || H < Hkv || H % Hkv || H > (1 << 16)) return false;
    const int items = (H + 2 * Hkv) * 4;
    d.H = H;
    d.Hkv = Hkv;
    d.G = H / Hkv;
    d.S = (int)S;
    d.tpb = std::max(1, 1024 / items);
    d.items = make_fastdiv((uint32_t)items);
    d.seq = make_fastdiv((uint32_t)S);
    return true;
}

}  // namespace

DDL_API int ddl_rmsnorm_supported(int H) { return H % 8 == 0 && H >= 64 && H <= 8192; }

DDL_API int ddl_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, long rows, int H, float eps,
                            hipStream_t st) {
    if (!ddl_rmsnorm_supported(H) || rows < 0 || (rows + 3) / 4 > 0x7fffffffL) return -1;
    if (rows == 0) return 0;
    const unsigned grid = (unsigned)((rows + 3) / 4);
#define RMSF(N) rmsnorm_fwd_k<N><<<grid, 256, 0, st>>>((const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, rstd, rows, H, eps)
    switch (np_for(H)) {
        case 1: RMSF(1); break;
        case 2: RMSF(2); break;
        case 4: RMSF(4); break;
        case 8: RMSF(8); break;
        default: RMSF(16); break;
    }
#undef RMSF
    DDL_RETURN_LAUNCH();
}

// Rows per backward block: at least 8 (two per wave), and no more than 1024 blocks (partial rows).
static int rmsnorm_rpb(long rows) {
    long rpb = std::max(8L, (rows + 1023) / 1024);
    return (int)((rpb + 3) / 4 * 4);
}

DDL_API int ddl_rmsnorm_bwd_nblk(long rows) {
    if (rows <= 0 || rows > (1L << 40)) return 0;
    const int rpb = rmsnorm_rpb(rows);
    return (int)((rows + rpb - 1) / rpb);
}

// part: ddl_rmsnorm_bwd_nblk(rows) * H floats.  add: nullable.
DDL_API int ddl_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, const void* add, void* dx,
                            float* part, void* dw, long rows, int H, hipStream_t st) {
    if (!ddl_rmsnorm_supported(H) || rows < 1) return -1;
    const int nblk = ddl_rmsnorm_bwd_nblk(rows);
    if (nblk < 1) return -1;
    const int rpb = rmsnorm_rpb(rows);
#define RMSB(N, A)                                                                                                   \
    rmsnorm_bwd_k<N, A><<<nblk, 256, 0, st>>>((const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)w, rstd,           \
                                              (const bf16_t*)add, (bf16_t*)dx, part, rows, H, rpb)
#define RMSB2(N) do { if (add) RMSB(N, true); else RMSB(N, false); } while (0)
    switch (np_for(H)) {
        case 1: RMSB2(1); break;
        case 2: RMSB2(2); break;
        case 4: RMSB2(4); break;
        case 8: RMSB2(8); break;
        default: RMSB2(16); break;
    }
#undef RMSB2
#undef RMSB
    rmsnorm_dw_k<<<(H + 63) / 64, 1024, 0, st>>>(part, nblk, H, (bf16_t*)dw);
    DDL_RETURN_LAUNCH();
}

DDL_API int ddl_rope_qkv_supported(int H, int Hkv, int head_dim) {
    return head_dim == 64 && Hkv >= 1 && H >= Hkv && H % Hkv == 0 && H <= (1 << 16);
}

// in [B, S, (H + 2 Hkv) * 64] -> out [B, S, 3, H, 64]; tab [n_pos, 64] fp32; S <= n_pos or -2.
DDL_API int ddl_rope_qkv_fwd(const void* in, const float* tab, void* out, long B, long S, int H, int Hkv, long n_pos,
                             hipStream_t st) {
    RopeDims d;
    if (!rope_dims(B, S, H, Hkv, d)) return -1;
    if (S > n_pos) return -2;
    const long ntok = B * S, grid = (ntok + d.tpb - 1) / d.tpb;
    if (grid > 0x7fffffffL) return -1;
    rope_qkv_fwd_k<false><<<(unsigned)grid, 256, 0, st>>>((const bf16_t*)in, tab, (bf16_t*)out, ntok, d, nullptr, 0);
    DDL_RETURN_LAUNCH();
}

DDL_API int ddl_rope_qkv_bwd(const void* dout, const float* tab, void* din, long B, long S, int H, int Hkv, long n_pos,
                             hipStream_t st) {
    RopeDims d;
    if (!rope_dims(B, S, H, Hkv, d)) return -1;
    if (S > n_pos) return -2;
    const long ntok = B * S, grid = (ntok + d.tpb - 1) / d.tpb;
    if (grid > 0x7fffffffL) return -1;
    rope_qkv_bwd_k<false><<<(unsigned)grid, 256, 0, st>>>((const bf16_t*)dout, tab, (bf16_t*)din, ntok, d, nullptr, 0);
    DDL_RETURN_LAUNCH();
}

// The same with explicit positions: pos int32 [B, S], token (b, s) rotated by table row pos[b, s], each in
// [0, n_pos) (the caller's contract; S itself may exceed n_pos).
DDL_API int ddl_rope_qkv_pos_fwd(const void* in, const float* tab, void* out, const int* pos, long B, long S, int H,
                                 int Hkv, long n_pos, hipStream_t st) {
    RopeDims d;
    if (!rope_dims(B, S, H, Hkv, d) || !pos || n_pos < 1 || n_pos > 0x7fffffffL) return -1;
    const long ntok = B * S, grid = (ntok + d.tpb - 1) / d.tpb;
    if (grid > 0x7fffffffL) return -1;
    rope_qkv_fwd_k<true><<<(unsigned)grid, 256, 0, st>>>((const bf16_t*)in, tab, (bf16_t*)out, ntok, d, pos,
                                                         (uint32_t)n_pos);
    DDL_RETURN_LAUNCH();
}

DDL_API int ddl_rope_qkv_pos_bwd(const void* dout, const float* tab, void* din, const int* pos, long B, long S, int H,
                                 int Hkv, long n_pos, hipStream_t st) {
    RopeDims d;
    if (!rope_dims(B, S, H, Hkv, d) || !pos || n_pos < 1 || n_pos > 0x7fffffffL) return -1;
    const long ntok = B * S, grid = (ntok + d.tpb - 1) / d.tpb;
    if (grid > 0x7fffffffL) return -1;
    rope_qkv_bwd_k<true><<<(unsigned)grid, 256, 0, st>>>((const bf16_t*)dout, tab, (bf16_t*)din, ntok, d, pos,
                                                         (uint32_t)n_pos);
    DDL_RETURN_LAUNCH();
}

DDL_API int ddl_swiglu_supported(long rows, int I) {
    return I >= 8 && I % 8 == 0 && rows >= 0 && rows * (I / 8) < (1L << 31) - 256;
}

DDL_API int ddl_swiglu_fwd(const void* gu, void* z, long rows, int I, hipStream_t st) {
    if (!ddl_swiglu_supported(rows, I)) return -1;
    if (rows == 0) return 0;
    const uint32_t n8 = (uint32_t)(rows * (I / 8));
    swiglu_fwd_k<<<(n8 + 255) / 256, 256, 0, st>>>((const bf16_t*)gu, (bf16_t*)z, n8, I, make_fastdiv(I / 8));
    DDL_RETURN_LAUNCH();
}

DDL_API int ddl_swiglu_bwd(const void* gu, const void* dz, void* dgu, long rows, int I, hipStream_t st) {
    if (!ddl_swiglu_supported(rows, I)) return -1;
    if (rows == 0) return 0;
    const uint32_t n8 = (uint32_t)(rows * (I / 8));
    swiglu_bwd_k<<<(n8 + 255) / 256, 256, 0, st>>>((const bf16_t*)gu, (const bf16_t*)dz, (bf16_t*)dgu, n8, I,
                                                   make_fastdiv(I / 8));
    DDL_RETURN_LAUNCH();
}
