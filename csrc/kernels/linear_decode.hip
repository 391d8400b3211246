// Linear layer at M <= 16 rows (a decode step's GEMMs): y[M, N] = act(x W^T + bias) + residual,
// x [M, K] bf16, W [N, K] bf16 row-major (the layout every Linear and the tied embedding have),
// K % 8 == 0, any N (no padded weight copy), fp32 accumulation, bf16 output.
//
// The tiled GEMMs cut M by 128 / 256 rows, so at M = 1 a whole weight is streamed by N / 256
// workgroups.  Here the weight is the only traffic that matters and each element of it is read from
// memory once, straight into VGPRs as an MFMA operand (no LDS staging: nothing is shared between
// waves): v_mfma_f32_16x16x32_bf16 with W as the 16-row operand and x, zero-padded to 16 rows, as the
// other.  MFMA rather than VALU dot products: at M = 16 a VALU form needs 16 FMAs per weight element,
// about the chip's whole fp32 VALU rate at the HBM streaming rate, while the matrix pipe makes the
// arithmetic free at every M <= 16 with one code path.  An MFMA's 32-deep k slice may be any 32
// elements as long as both operands agree: lane (r, q) loads k = 64 s + 16 q + 8 j + 0..7 (j = 0, 1),
// i.e. 32 contiguous bytes per lane, and the four q lanes of a row cover one 128-byte line.
//
// Decomposition: a wave owns NT 16-row weight tiles (NT = 4 for a large N such as the vocabulary,
// 1 otherwise) and a range of 64-deep k steps; the 4 waves of a workgroup take consecutive k ranges of
// the same rows and add up through LDS in wave order.  Where N alone gives too few workgroups, K is
// also split over gridDim.y: fp32 partials to a workspace and a second launch that adds them in split
// order and applies the epilogue.  No float atomics anywhere, so results are bitwise repeatable.
#include "ddl_common.h"

namespace {

constexpr int LD_WAVES = 4;
constexpr int LD_KSTEP = 64;
constexpr int LD_MAX_KSPLIT = 16;
constexpr int LD_BIG_N = 4096;      // above: 4 weight tiles per wave

struct LdPlan {
    int nt, ntiles, ksplit, per;    // tiles per wave, workgroups over N, workgroups over K, k steps per wave
};

inline LdPlan ld_plan(int N, int K) {
    LdPlan p;
    p.nt = N > LD_BIG_N ? 4 : 1;
    p.ntiles = (N + 16 * p.nt - 1) / (16 * p.nt);
    const int ksteps = (K + LD_KSTEP - 1) / LD_KSTEP;
    const int want = std::max(1, (2 * num_cus() + p.ntiles - 1) / p.ntiles);    // two workgroups per CU
    p.per = std::max(1, ksteps / (want * LD_WAVES));
    p.per = std::max(p.per, (ksteps + LD_MAX_KSPLIT * LD_WAVES - 1) / (LD_MAX_KSPLIT * LD_WAVES));
    p.ksplit = (ksteps + p.per * LD_WAVES - 1) / (p.per * LD_WAVES);
    return p;
}

__device__ __forceinline__ float epilogue(float v, long m, int n, int N, const bf16_t* bias, const bf16_t* residual, int act) {
    if (bias) v += bf2f(bias[n]);
    if (act == 1) v = gelu_erf(v);
    if (residual) v += bf2f(residual[m * N + n]);
    return v;
}

template <int NT>
__global__ __launch_bounds__(LD_WAVES * 64) void linear_small_m_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                                  const bf16_t* __restrict__ bias,
                                                                  const bf16_t* __restrict__ residual, bf16_t* __restrict__ y,
                                                                  float* __restrict__ ws, int M, int N, int K, int act,
                                                                  int per) {
    __shared__ f32x4 red[LD_WAVES][NT][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * NT * 16;
    const int ksteps = (K + LD_KSTEP - 1) / LD_KSTEP;
    const int ks0 = (blockIdx.y * LD_WAVES + wave) * per, ks1 = std::min(ks0 + per, ksteps);

    const bool ok_m = r < M;
    const bf16_t* xp = x + (long)(ok_m ? r : 0) * K;
    const bf16_t* wp[NT];
    bool ok_n[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = n0 + 16 * t + r;
        ok_n[t] = n < N;
        wp[t] = w + (long)(ok_n[t] ? n : 0) * K;
    }
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int ks = ks0; ks < ks1; ++ks) {
        uint4 xa[2], wa[NT][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = ks * LD_KSTEP + 16 * q + 8 * j;
            const bool ok_k = k < K;        // K % 8 == 0: a 16-byte piece is all inside or all outside
            xa[j] = make_uint4(0, 0, 0, 0);
            if (ok_m && ok_k) xa[j] = *reinterpret_cast<const uint4*>(xp + k);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                wa[t][j] = make_uint4(0, 0, 0, 0);
                if (ok_n[t] && ok_k) wa[t][j] = *reinterpret_cast<const uint4*>(wp[t] + k);
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wa[t][j]),
                                                                 __builtin_bit_cast(bf16x8, xa[j]), acc[t], 0, 0, 0);
    }

    // lane holds rows m = r, columns n0 + 16 t + 4 q + 0..3; the 4 waves' k ranges add up in wave order
#pragma unroll
    for (int t = 0; t < NT; ++t) red[wave][t][lane] = acc[t];
    __syncthreads();
    if (tid < NT * 64) {
        const int t = tid >> 6;
        f32x4 s = red[0][t][lane];
#pragma unroll
        for (int wv = 1; wv < LD_WAVES; ++wv) s += red[wv][t][lane];
        if (r < M) {
            const int nb = n0 + 16 * t + 4 * q;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = nb + e;
                if (n < N) {
                    if (gridDim.y == 1) y[(long)r * N + n] = f2bf(epilogue(s[e], r, n, N, bias, residual, act));
                    else ws[((long)blockIdx.y * M + r) * N + n] = s[e];
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void linear_small_m_combine_k(const float* __restrict__ ws, const bf16_t* __restrict__ bias,
                                                                const bf16_t* __restrict__ residual, bf16_t* __restrict__ y,
                                                                int M, int N, int ksplit, int act) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, MN = (long)M * N;
    if (i >= MN) return;
    float v = ws[i];
    for (int s = 1; s < ksplit; ++s) v += ws[s * MN + i];
    const long m = i / N;
    y[i] = f2bf(epilogue(v, m, (int)(i - m * N), N, bias, residual, act));
}

}  // namespace

// the decomposition the launch uses for this (N, K): out = {tiles per wave, workgroups over N, K splits,
// 64-deep k steps per wave}
DDL_API int ddl_linear_small_m_plan(int N, int K, int* out) {
    const LdPlan p = ld_plan(std::max(1, N), std::max(8, K));
    out[0] = p.nt; out[1] = p.ntiles; out[2] = p.ksplit; out[3] = p.per;
    return 0;
}
// floats of workspace (0 without a K split)
DDL_API long ddl_linear_small_m_ws(int M, int N, int K) {
    const LdPlan p = ld_plan(std::max(1, N), std::max(8, K));
    return p.ksplit == 1 ? 0 : (long)p.ksplit * M * N;
}

// act: 0 none, 1 erf-GELU; bias / residual nullable (bf16); ws: ddl_linear_small_m_ws floats
DDL_API int ddl_linear_small_m(const void* x, const void* w, const void* bias, const void* residual, void* y, void* ws, int M,
                               int N, int K, int act, hipStream_t st) {
    if (M < 1 || M > 16 || N < 1 || K < 8 || K % 8 || act < 0 || act > 1) return (int)hipErrorInvalidValue;
    const LdPlan p = ld_plan(N, K);
    if (p.ksplit > 1 && !ws) return (int)hipErrorInvalidValue;
    const dim3 grid(p.ntiles, p.ksplit);
    if (p.nt == 4)
        linear_small_m_k<4><<<grid, LD_WAVES * 64, 0, st>>>((const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)bias,
                                                            (const bf16_t*)residual, (bf16_t*)y, (float*)ws, M, N, K, act, p.per);
    else
        linear_small_m_k<1><<<grid, LD_WAVES * 64, 0, st>>>((const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)bias,
                                                            (const bf16_t*)residual, (bf16_t*)y, (float*)ws, M, N, K, act, p.per);
    if (p.ksplit > 1) {
        const long MN = (long)M * N;
        linear_small_m_combine_k<<<(unsigned)((MN + 255) / 256), 256, 0, st>>>((const float*)ws, (const bf16_t*)bias,
                                                                              (const bf16_t*)residual, (bf16_t*)y, M, N,
                                                                              p.ksplit, act);
    }
    DDL_RETURN_LAUNCH();
}
