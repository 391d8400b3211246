// Linear layer at M <= 16 rows with an FP8 weight: y[M, N] = act((x Wq^T) * scale + bias) + residual,
// x [M, K] bf16, Wq [N, K] one byte per element (OCP e4m3, torch.float8_e4m3fn's bits), row-major,
// scale [N] fp32 (one per output row), K % 16 == 0, any N, fp32 accumulation, bf16 output.
//
// A decode step's linears are bound by the bytes of weight they stream (linear_decode.hip); this is
// the same contract with half the bytes.  The activation stays bf16 and the arithmetic stays on
// v_mfma_f32_16x16x32_bf16: the weight bytes are turned into bf16 in registers by
// v_cvt_scalef32_pk_bf16_fp8 (scale 1.0), two per instruction, exactly -- e4m3's four significant bits
// and its exponent range (2^-9 .. 448, subnormals included) all sit inside bf16 -- so what is
// accumulated is x[m, k] * value(Wq[n, k]) with no rounding before the fp32 sum.  scale[n] multiplies
// the finished sum once, in the epilogue, never an element.
//
// Lane-to-k mapping.  A k step is 128 deep.  Lane (r, q) of a 16-row weight tile owns bytes
// 128 s + 32 q + 0..31 of row r: two 16-byte loads, and the four q lanes of a row cover one 128-byte
// line, as in the bf16 kernel.  Those 32 weights are four MFMA operands: operand j is bytes
// 8 j .. 8 j + 7, set against x elements k = 128 s + 32 q + 8 j + 0..7 of row r (r < M; zero above),
// 64 contiguous bytes of x per lane.  Tail rule: K % 16 == 0, so a 16-byte piece of W is all inside
// or all outside K, and so are the two 16-byte pieces of x that face it.
//
// x traffic.  Per weight byte this issues twice the x loads of the bf16 kernel (x is in L2 / L1; it
// costs load instructions and L1 bandwidth, not HBM).  It is paid for with more weight tiles per wave
// at every N: a wave owns NT = 2 tiles (N <= 1024) or 4 (above), so its four x loads serve 4 or 8
// weight loads -- one half or one third of the load instructions are x, where one tile per wave would
// make it two thirds.  The x slice is not staged through LDS: the four waves of a workgroup take
// different k ranges, so nothing of x is shared between them, and a wave-private LDS copy would trade
// each global load for a DMA plus a ds_read.
//
// Decomposition (the bf16 kernel's, with its own plan): the 4 waves of a workgroup take consecutive k
// ranges of the same NT tiles and add up through LDS in wave order; where N alone gives too few
// workgroups, K is also split over gridDim.y: raw fp32 partials to a workspace and a second launch
// that adds them in split order, applies the scale and the epilogue.  No float atomics, no scratch:
// results are bitwise repeatable.
//
// Plan.  A step of a wave has NT x 2 KB of weight in flight (the loop holds one step's loads), so a
// workgroup has 16 KB (NT = 2) or 32 KB (NT = 4).  At 6.3 TB/s and about 2 us of memory latency the
// chip wants some 12 MB in flight, 48 KB per CU: the plan asks for 4 workgroups per CU at NT = 2 and 2
// at NT = 4, 64 KB per CU either way, and splits K to get them (at most LF_MAX_KSPLIT ways).
#include "ddl_common.h"

namespace {

constexpr int LF_WAVES = 4;
constexpr int LF_KSTEP = 128;
constexpr int LF_MAX_KSPLIT = 16;
constexpr int LF_NT4_N = 1024;      // above: 4 weight tiles per wave, else 2

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

struct LfPlan {
    int nt, ntiles, ksplit, per;    // tiles per wave, workgroups over N, workgroups over K, k steps per wave
};

inline LfPlan lf_plan(int N, int K) {
    LfPlan p;
    p.nt = N > LF_NT4_N ? 4 : 2;
    p.ntiles = (N + 16 * p.nt - 1) / (16 * p.nt);
    const int ksteps = (K + LF_KSTEP - 1) / LF_KSTEP;
    const int wgs = (p.nt == 4 ? 2 : 4) * num_cus();
    const int want = std::max(1, (wgs + p.ntiles - 1) / p.ntiles);
    p.per = std::max(1, ksteps / (want * LF_WAVES));
    p.per = std::max(p.per, (ksteps + LF_MAX_KSPLIT * LF_WAVES - 1) / (LF_MAX_KSPLIT * LF_WAVES));
    p.ksplit = (ksteps + p.per * LF_WAVES - 1) / (p.per * LF_WAVES);
    return p;
}

// 8 e4m3 bytes (two dwords, byte i = weight k + i) -> 8 bf16, exactly: four packed converts
__device__ __forceinline__ bf16x8 e4m3x8_to_bf16(uint32_t lo, uint32_t hi) {
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
    const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
    const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
    return (bf16x8){a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// the finished fp32 sum -> one multiply by the row's scale (never contracted into the bias add), then
// the bf16 kernel's order: bias, act, residual
__device__ __forceinline__ float epilogue(float v, float scale, long m, int n, int N, const bf16_t* bias,
                                          const bf16_t* residual, int act) {
    v = __fmul_rn(v, scale);
    if (bias) v += bf2f(bias[n]);
    if (act == 1) v = gelu_erf(v);
    if (residual) v += bf2f(residual[m * N + n]);
    return v;
}

template <int NT>
__global__ __launch_bounds__(LF_WAVES * 64) void linear_small_m_fp8_k(const bf16_t* __restrict__ x,
                                                                      const uint8_t* __restrict__ w,
                                                                      const float* __restrict__ scale,
                                                                      const bf16_t* __restrict__ bias,
                                                                      const bf16_t* __restrict__ residual,
                                                                      bf16_t* __restrict__ y, float* __restrict__ ws, int M,
                                                                      int N, int K, int act, int per) {
    __shared__ f32x4 red[LF_WAVES][NT][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * NT * 16;
    const int ksteps = (K + LF_KSTEP - 1) / LF_KSTEP;
    const int ks0 = (blockIdx.y * LF_WAVES + wave) * per, ks1 = std::min(ks0 + per, ksteps);

    // the scales of the four outputs this lane finishes (tile `wave`, columns 4 q + 0..3), loaded ahead
    // of the first operand loads
    float sc[4] = {0.f, 0.f, 0.f, 0.f};
    if (gridDim.y == 1 && wave < NT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int n = n0 + 16 * wave + 4 * q + e;
            if (n < N) sc[e] = scale[n];
        }
    }

    const bool ok_m = r < M;
    const bf16_t* xp = x + (long)(ok_m ? r : 0) * K;
    const uint8_t* wp[NT];
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
        uint4 wa[NT][2], xa[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = ks * LF_KSTEP + 32 * q + 16 * h;
            const bool ok_k = k < K;        // K % 16 == 0: a 16-byte piece of W is all inside or all outside
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                wa[t][h] = make_uint4(0, 0, 0, 0);
                if (ok_n[t] && ok_k) wa[t][h] = *reinterpret_cast<const uint4*>(wp[t] + k);
            }
#pragma unroll
            for (int j = 2 * h; j < 2 * h + 2; ++j) {
                xa[j] = make_uint4(0, 0, 0, 0);
                if (ok_m && ok_k) xa[j] = *reinterpret_cast<const uint4*>(xp + k + 8 * (j - 2 * h));
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(e4m3x8_to_bf16(wa[t][h].x, wa[t][h].y),
                                                                 __builtin_bit_cast(bf16x8, xa[2 * h]), acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(e4m3x8_to_bf16(wa[t][h].z, wa[t][h].w),
                                                                 __builtin_bit_cast(bf16x8, xa[2 * h + 1]), acc[t], 0, 0, 0);
            }
    }

    // lane holds row m = r, columns n0 + 16 t + 4 q + 0..3; the 4 waves' k ranges add up in wave order
#pragma unroll
    for (int t = 0; t < NT; ++t) red[wave][t][lane] = acc[t];
    __syncthreads();
    if (wave < NT) {
        const int t = wave;
        f32x4 s = red[0][t][lane];
#pragma unroll
        for (int wv = 1; wv < LF_WAVES; ++wv) s += red[wv][t][lane];
        if (r < M) {
            const int nb = n0 + 16 * t + 4 * q;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = nb + e;
                if (n < N) {
                    if (gridDim.y == 1) y[(long)r * N + n] = f2bf(epilogue(s[e], sc[e], r, n, N, bias, residual, act));
                    else ws[((long)blockIdx.y * M + r) * N + n] = s[e];
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void linear_small_m_fp8_combine_k(const float* __restrict__ ws,
                                                                    const float* __restrict__ scale,
                                                                    const bf16_t* __restrict__ bias,
                                                                    const bf16_t* __restrict__ residual,
                                                                    bf16_t* __restrict__ y, int M, int N, int ksplit, int act) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, MN = (long)M * N;
    if (i >= MN) return;
    const long m = i / N;
    const int n = (int)(i - m * N);
    const float sc = scale[n];
    float v = ws[i];
    for (int s = 1; s < ksplit; ++s) v += ws[s * MN + i];
    y[i] = f2bf(epilogue(v, sc, m, n, N, bias, residual, act));
}

}  // namespace

// the decomposition the launch uses for this (N, K): out = {tiles per wave, workgroups over N, K splits,
// 128-deep k steps per wave}
DDL_API int ddl_linear_small_m_fp8_plan(int N, int K, int* out) {
    const LfPlan p = lf_plan(std::max(1, N), std::max(16, K));
    out[0] = p.nt; out[1] = p.ntiles; out[2] = p.ksplit; out[3] = p.per;
    return 0;
}
// floats of workspace (0 without a K split)
DDL_API long ddl_linear_small_m_fp8_ws(int M, int N, int K) {
    const LfPlan p = lf_plan(std::max(1, N), std::max(16, K));
    return p.ksplit == 1 ? 0 : (long)p.ksplit * M * N;
}

// wq: e4m3 bytes [N, K]; scale: fp32 [N]; act: 0 none, 1 erf-GELU; bias / residual nullable (bf16);
// ws: ddl_linear_small_m_fp8_ws floats
DDL_API int ddl_linear_small_m_fp8(const void* x, const void* wq, const void* scale, const void* bias, const void* residual,
                                   void* y, void* ws, int M, int N, int K, int act, hipStream_t st) {
    if (M < 1 || M > 16 || N < 1 || K < 16 || K % 16 || act < 0 || act > 1 || !x || !wq || !scale || !y)
        return (int)hipErrorInvalidValue;
    const LfPlan p = lf_plan(N, K);
    if (p.ksplit > 1 && !ws) return (int)hipErrorInvalidValue;
    const dim3 grid(p.ntiles, p.ksplit);
    if (p.nt == 4)
        linear_small_m_fp8_k<4><<<grid, LF_WAVES * 64, 0, st>>>((const bf16_t*)x, (const uint8_t*)wq, (const float*)scale,
                                                                (const bf16_t*)bias, (const bf16_t*)residual, (bf16_t*)y,
                                                                (float*)ws, M, N, K, act, p.per);
    else
        linear_small_m_fp8_k<2><<<grid, LF_WAVES * 64, 0, st>>>((const bf16_t*)x, (const uint8_t*)wq, (const float*)scale,
                                                                (const bf16_t*)bias, (const bf16_t*)residual, (bf16_t*)y,
                                                                (float*)ws, M, N, K, act, p.per);
    if (p.ksplit > 1) {
        const long MN = (long)M * N;
        linear_small_m_fp8_combine_k<<<(unsigned)((MN + 255) / 256), 256, 0, st>>>(
            (const float*)ws, (const float*)scale, (const bf16_t*)bias, (const bf16_t*)residual, (bf16_t*)y, M, N, p.ksplit,
            act);
    }
    DDL_RETURN_LAUNCH();
}
