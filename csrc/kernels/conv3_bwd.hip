// Backward of a ResNet stage-1 bottleneck's conv3 -> bn3 pair in ONE streaming pass:
//   dx3  = A o dz + B o x3 + D          (bn3's backward apply, per-channel coefficients)
//   dz2  = relu_mask2 o (dx3 . W3)      (conv3 dgrad with bn2's backward reduction in its epilogue:
//                                        one [sum dz2 | sum dz2 * xhat2] row per workgroup)
//   dW3 += dx3^T . a2                   (conv3 wgrad)
// for (C_out, C_in) = (256, 64), bf16, fp32 accumulate.
//
// Unfused this is three memory-bound passes (bn_bwd_apply_rows_k, skinny_gemm_k<64, 256, EPI_BNB>,
// stream_wgrad_k<256, 64>): dx3 -- four C_in-wide units -- is written once and read twice, 23 units
// in all.  Here dx3 never leaves the CU: a persistent workgroup walks a contiguous chunk of 32-row
// tiles; the tile's dz, x3, a2, x2 rows and bn2 mask bytes arrive by LDS-DMA into a ring of images
// (NBUF - 1 tiles in flight), all threads rewrite the dz image in place as bf16(dx3) -- the same
// fp32 expression and rounding as bn_bwd_apply_rows_k, so the MFMAs read exactly what that pass
// would have stored -- and both products run from that image: the dgrad against the weight resident
// in LDS (the k order of skinny_gemm_k: dz2 is bitwise what the unfused path gives), the wgrad by
// transposed LDS reads into accumulators that live in registers for the workgroup's whole life.
// 11 units of traffic.  Workgroups are independent: one bf16 dW partial (the format and the reduce order of stream_wgrad_k:
// at equal row chunks dW is bitwise the unfused result too) and one statistics row each.
// Rows past M are zeroed in the dx3 image (the DMA clamps them to a valid row): they add nothing to
// dW or the statistics, and their dz2 rows are dropped by the store's range check.
// Reference behaviour: autograd of torchvision's Bottleneck conv3 / bn3 under cuDNN.
#include "ddl_lds.h"

#include <algorithm>

namespace {

constexpr int NW = 8, NTH = NW * 64;
constexpr int TM = 32;                          // rows per tile: one MFMA k-step of the wgrad
constexpr int DPT = 6, SPT = 1;                 // DMA / store instructions per wave per tile

struct C3Params {
    const bf16_t* dz;      // [M][CO] gradient of bn3's output (ReLU mask applied)
    const bf16_t* x3;      // [M][CO] bn3's input
    const float* mean3;
    const float* istd3;
    const float* coef3;    // [3][CO]: gamma * istd | mean(dz) | mean(dz * xhat)  (bn_bwd_finalize)
    const bf16_t* a2;      // [M][CI] conv3's input
    const bf16_t* x2;      // [M][CI] bn2's input
    const uint8_t* mask2;  // bn2's ReLU bit mask (null: all kept)
    const float* mean2;
    const float* istd2;
    const bf16_t* wt;      // [CI][CO] W3 transposed
    bf16_t* dz2;           // [M][CI]
    float* colstats;       // [gridDim.x][2][CI]
    bf16_t* wpart;         // [gridDim.x][CO][CI] bf16
    long M;
    int tiles, chunk;
    uint32_t dz2_bytes;
};

// 8 elements of dx = A dz + B x + D in the shared spelling of the apply pass (ddl_common.h), so the
// bf16 image is bit-identical to the tensor that pass stores
__device__ __forceinline__ u32x4 bn_apply8(bf16x8 dzv, bf16x8 xv, const float* A, const float* B, const float* D,
                                           bool valid) {
    const u32x4 gw = __builtin_bit_cast(u32x4, dzv), xw = __builtin_bit_cast(u32x4, xv);
    const uint32_t keep = valid ? ~0u : 0u;     // rows past M: zeros
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float g0 = lo_f(gw[i]), g1 = hi_f(gw[i]);
        const float x0 = lo_f(xw[i]), x1 = hi_f(xw[i]);
        const float o0 = bn_bwd_apply1(A[2 * i], g0, B[2 * i], x0, D[2 * i]);
        const float o1 = bn_bwd_apply1(A[2 * i + 1], g1, B[2 * i + 1], x1, D[2 * i + 1]);
        o[i] = pack2bf(o0, o1) & keep;
    }
    return o;
}

// (CO, CI) = (256, 64).  LDS: W^T image [CI][CO] (32 KB) | NBUF x { dz [TM][CO] | x3 [TM][CO] |
// a2 [TM][CI] | x2 [TM][CI] (the dz2 tile is written over it) | mask (1 KB) }; all bf16 images
// swizzled: 16-byte chunk c of row r at chunk c ^ (r & 15) (512-byte rows) / c ^ (r & 7) (128-byte)
template <int CO, int CI, int NBUF>
__global__ __launch_bounds__(NTH, 1) void conv3_bwd_k(C3Params p) {
    static_assert(CO == 256 && CI == 64 && (NBUF == 2 || NBUF == 3), "shape");
    constexpr int WBYTES = CI * CO * 2, ZBYTES = TM * CO * 2, ABYTES = TM * CI * 2;
    constexpr int O_DZ = 0, O_X3 = ZBYTES, O_A2 = 2 * ZBYTES, O_X2 = O_A2 + ABYTES, O_MK = O_X2 + ABYTES;
    constexpr int BUFB = O_MK + 1024;
    constexpr int LDS = WBYTES + NBUF * BUFB;
    static_assert(LDS <= 160 * 1024, "LDS");
    __shared__ __attribute__((aligned(16))) char smem[LDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, r16 = lane & 15;
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    const __amdgpu_buffer_rsrc_t crs = rsrc(p.dz2, p.dz2_bytes);
    const int t0 = blockIdx.x * p.chunk, t1 = min(p.tiles, t0 + p.chunk);

    // every wave issues DPT DMA instructions per tile: 2 of dz, 2 of x3 (1 KB = 2 rows each), one of
    // a2 (waves 0-3) or x2 (waves 4-7) (1 KB = 8 rows), one of the mask (256 B, the same in every wave).
    // Non-temporal: every row is streamed once
    auto prefetch = [&](int t, int buf) {
        char* base = smem + WBYTES + buf * BUFB;
        const long m0 = (long)t * TM;
#pragma unroll
        for (int qq = 0; qq < 2; ++qq) {
            const int q = qq * NW + wv, r = q * 2 + (lane >> 5), c = (lane & 31) ^ (r & 15);
            const long gr = min(m0 + r, p.M - 1);          // rows past the end: any valid row
            glds16_nt(p.dz + gr * CO + c * 8, base + O_DZ + q * 1024);
            glds16_nt(p.x3 + gr * CO + c * 8, base + O_X3 + q * 1024);
        }
        {
            const int q = wv & 3, r = q * 8 + (lane >> 3), c = (lane & 7) ^ (r & 7);
            const long gr = min(m0 + r, p.M - 1);
            glds16_nt((wv < 4 ? p.a2 : p.x2) + gr * CI + c * 8, base + (wv < 4 ? O_A2 : O_X2) + q * 1024);
        }
        {
            // TM rows x CI / 8 mask bytes = 256 contiguous bytes (the mask ends on a dword:
            // clamping never misplaces a valid row's bytes).  Every wave issues this same instruction
            // (identical data, one would do), and without a mask it loads bytes nobody reads: what
            // matters is that each wave's DMA count per tile is the constant DPT the waits count
            const long b = min(m0 * (CI / 8) + lane * 4, p.M * (CI / 8) - 4);
            const uint8_t* src = p.mask2 ? p.mask2 + b : (const uint8_t*)p.a2;
            glds4(src, base + O_MK);
        }
    };
    // W^T rows: 4 DMA instructions per wave (dma_rows<NW, CO, CI> without its row clamp, which no
    // row here needs and which costs instructions)
#pragma unroll
    for (int qq = 0; qq < CI / 2 / NW; ++qq) {
        const int q = qq * NW + wv, r = q * 2 + (lane >> 5), c = (lane & 31) ^ (r & 15);
        glds16_nt(p.wt + (long)r * CO + c * 8, smem + q * 1024);
    }
#pragma unroll
    for (int u = 0; u < NBUF - 1; ++u)
        if (t0 + u < t1) prefetch(t0 + u, u);

    // ---- transform: thread owns 16-byte chunk tc of rows tr and tr + 16
    const int tc = tid & 31, tr = tid >> 5;
    float cA[8], cB[8], cD[8];
    bn_bwd_apply_coefs8(p.mean3, p.istd3, p.coef3, CO, tc * 8, cA, cB, cD);
    const uint32_t toff = tr * (CO * 2) + ((tc ^ tr) << 4);          // tr < 16; row tr + 16: + 16 rows

    // ---- dgrad: waves 0-3 own 16 output columns each, both 16-row fragments (the accumulation order
    // of skinny_gemm_k<64, 256, EPI_BNB>, whose statistics rows this kernel reproduces bit for bit when
    // both walk the same row chunks); lane holds dz2[16 i + r16][16 dj + 4 g .. + 3]
    const int dj = wv & 3;
    const bool dgw = wv < 4;
    uint32_t aoff[2][CO / 32], boff[CO / 32];
#pragma unroll
    for (int kk = 0; kk < CO / 32; ++kk) {
        const int rb = 16 * dj + r16;
        boff[kk] = lds0 + rb * (CO * 2) + (((kk * 4 + g) ^ (rb & 15)) << 4);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ra = 16 * i + r16;
            aoff[i][kk] = ra * (CO * 2) + (((kk * 4 + g) ^ (ra & 15)) << 4);
        }
    }
    uint32_t coff[2], moff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int drow = 16 * i + r16;
        coff[i] = drow * (CI * 2) + (((2 * dj + (g >> 1)) ^ (drow & 7)) << 4) + (g & 1) * 8;
        moff[i] = drow * (CI / 8) + (dj >> 1) * 4;
    }
    const int mshift = (dj & 1) * 16 + 4 * g;
    float st_s[4] = {0.f, 0.f, 0.f, 0.f}, st_q[4] = {0.f, 0.f, 0.f, 0.f};

    // ---- wgrad: wave owns dW rows 32 wv .. + 31 (2 fragments) x all CI columns (4 fragments);
    // operand fragments by transposed reads: lane reads 4 columns of row 8 g + q (+ 4)
    const int q4 = (lane >> 2) & 3, pq = lane & 3;
    uint32_t wa[2][2], wb[4][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = 8 * g + q4 + 4 * h;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int col = 32 * wv + 16 * i + 4 * pq;
            wa[i][h] = r * (CO * 2) + (((col >> 3) ^ (r & 15)) << 4) + (pq & 1) * 8;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = 16 * j + 4 * pq;
            wb[j][h] = r * (CI * 2) + (((col >> 3) ^ (r & 7)) << 4) + (pq & 1) * 8;
        }
    }
    f32x4 wacc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) wacc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    int buf = 0;
    for (int t = t0; t < t1; ++t) {
        // tile t landed: what this wave issued after its DMA -- the stores of up to NBUF - 1 earlier
        // tiles and the DMA of up to NBUF - 2 later ones -- may stay in flight
        wait_vm(min(NBUF - 1, t - t0) * SPT + min(NBUF - 2, t1 - 1 - t) * DPT);
        __builtin_amdgcn_s_barrier();
        // into the image tile t - 1 used (every wave is past its last read of it); none after the
        // last tile: LDS-DMA still landing when the workgroup exits would write into the LDS of
        // the next workgroup on this CU
        if (t + NBUF - 1 < t1) prefetch(t + NBUF - 1, buf == 0 ? NBUF - 1 : buf - 1);
        const uint32_t img = lds0 + WBYTES + buf * BUFB;
        const long m0 = (long)t * TM;

        // ---- dx3 over the dz image
        {
            const bf16x8 z0 = ds_read16(img + O_DZ + toff), z1 = ds_read16(img + O_DZ + toff + 16 * CO * 2);
            const bf16x8 x0 = ds_read16(img + O_X3 + toff), x1 = ds_read16(img + O_X3 + toff + 16 * CO * 2);
            LGKM0();
            __builtin_amdgcn_sched_barrier(0);
            ds_write16(img + O_DZ + toff, bn_apply8(z0, x0, cA, cB, cD, m0 + tr < p.M));
            ds_write16(img + O_DZ + toff + 16 * CO * 2, bn_apply8(z1, x1, cA, cB, cD, m0 + tr + 16 < p.M));
            LGKM0();
            __builtin_amdgcn_s_barrier();
        }

        // ---- dgrad (waves 0-3): 32 x 16 outputs per wave over K = CO
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if (dgw) {
#pragma unroll
            for (int k2 = 0; k2 < CO / 32; k2 += 4) {
                bf16x8 af[2][4], bfr[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    af[0][u] = ds_read16(img + O_DZ + aoff[0][k2 + u]);
                    af[1][u] = ds_read16(img + O_DZ + aoff[1][k2 + u]);
                    bfr[u] = ds_read16(boff[k2 + u]);
                }
                LGKM0();
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[u], af[0][u], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[u], af[1][u], acc[1], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // wgrad fragments, the mask word and the BN input of this lane's outputs
        s16x4 fal[2][2], fbl[4][2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int i = 0; i < 2; ++i) fal[i][h] = ds_read_tr8(img + O_DZ + wa[i][h]);
#pragma unroll
            for (int j = 0; j < 4; ++j) fbl[j][h] = ds_read_tr8(img + O_A2 + wb[j][h]);
        }
        uint32_t mword[2] = {~0u, ~0u};
        uint2 ev[2] = {make_uint2(0u, 0u), make_uint2(0u, 0u)};
        if (dgw) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (p.mask2) mword[i] = ds_read32(img + O_MK + moff[i]);
                ev[i] = ds_read8(img + O_X2 + coff[i]);
            }
        }
        LGKM0();
        __builtin_amdgcn_sched_barrier(0);
        {
            typedef short s16x8 __attribute__((ext_vector_type(8)));
            bf16x8 fa[2], fb[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const s16x8 r = {fal[i][0][0], fal[i][0][1], fal[i][0][2], fal[i][0][3],
                                 fal[i][1][0], fal[i][1][1], fal[i][1][2], fal[i][1][3]};
                fa[i] = __builtin_bit_cast(bf16x8, r);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const s16x8 r = {fbl[j][0][0], fbl[j][0][1], fbl[j][0][2], fbl[j][0][3],
                                 fbl[j][1][0], fbl[j][1][1], fbl[j][1][2], fbl[j][1][3]};
                fb[j] = __builtin_bit_cast(bf16x8, r);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    wacc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], wacc[i][j], 0, 0, 0);
        }
        // ---- dgrad epilogue: ReLU mask, bf16 into the x2 image, the BN-backward sums
        if (dgw) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float v[4] = {acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
                const float xv[4] = {lo_f(ev[i].x), hi_f(ev[i].x), lo_f(ev[i].y), hi_f(ev[i].y)};
                const uint32_t bits = mword[i] >> mshift;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = ((bits >> e) & 1u) ? v[e] : 0.f;
                const uint32_t lo = pack2bf(v[0], v[1]), hi = pack2bf(v[2], v[3]);
                ds_write8(img + O_X2 + coff[i], make_uint2(lo, hi));
                if (m0 + 16 * i + r16 < p.M) {
                    const float tq[4] = {lo_f(lo), hi_f(lo), lo_f(hi), hi_f(hi)};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        st_s[e] += tq[e];
                        st_q[e] = __builtin_fmaf(tq[e], xv[e], st_q[e]);
                    }
                }
            }
        }
        LGKM0();
        __builtin_amdgcn_s_barrier();
        // ---- the dz2 tile leaves as whole rows: 4 rows (512 B) per wave, one store instruction
        {
            const int row = 4 * wv + (lane >> 4), pc = lane & 15;
            const uint2 d = ds_read8(img + O_X2 + row * (CI * 2) + (((pc >> 1) ^ (row & 7)) << 4) + (pc & 1) * 8);
            LGKM0();
            __builtin_amdgcn_sched_barrier(0);
            const long grow = m0 + row;
            const uint32_t off = grow < p.M ? (uint32_t)((grow * CI + pc * 4) * 2) : 0x80000000u;
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, d), crs, (int)off, 0, 0);
        }
        buf = buf + 1 == NBUF ? 0 : buf + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- this workgroup's dW partial, bf16 as stream_wgrad_k writes it: lane holds
    // dW[32 wv + 16 i + r16][16 j + 4 g .. + 3]
    bf16_t* wout = p.wpart + (long)blockIdx.x * CO * CI;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<uint2*>(wout + (long)(32 * wv + 16 * i + r16) * CI + 16 * j + 4 * g) =
                make_uint2(pack2bf(wacc[i][j][0], wacc[i][j][1]), pack2bf(wacc[i][j][2], wacc[i][j][3]));

    // ---- statistics row: a wave owns its columns, lanes r16 == 0 hold the sums after the row reduction
    if (dgw) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = row16_sum(st_s[e]), b = row16_sum(st_q[e]);
            if (r16 == 0) {
                const int col = 16 * dj + 4 * g + e;
                p.colstats[(long)blockIdx.x * 2 * CI + col] = a;
                p.colstats[(long)blockIdx.x * 2 * CI + CI + col] =
                    __builtin_fmaf(-p.mean2[col], a, b) * p.istd2[col];                     // sum dz2 * xhat2
            }
        }
    }
}

}  // namespace

// Workgroups (= statistics rows = dW partials) ddl_conv3_bwd launches for M rows (grid <= 0: default)
DDL_API int ddl_conv3_bwd_grid(long M, int grid) {
    // the row chunks of skinny_gemm_k (whole 64-row tiles per workgroup): with the per-lane order of
    // the sums this makes the statistics rows bitwise what the unfused dgrad writes, at every M
    const int tiles64 = (int)((M + 63) / 64);
    const int g = std::min(grid > 0 ? std::min(grid, 256) : 256, tiles64);
    const int chunk64 = (tiles64 + g - 1) / g;
    return (tiles64 + chunk64 - 1) / chunk64;
}

// The fused conv3 / bn3 backward (see the top of this file).  dz, x3: [M][Cout]; coef3: bn3's
// backward coefficients (ddl_bn_bwd_coef_from_partials); a2, x2, dz2: [M][Cin]; mask2 (nullable),
// mean2, istd2: bn2's; wt: [Cin][Cout]; colstats: G rows of [sum dz2 | sum dz2 * xhat2]; wpart:
// >= G * Cout * Cin bf16 elements; dW: [Cout][Cin] bf16 or fp32 (dw_f32), += with accumulate.  bf16,
// row-major contiguous, 16-byte aligned (dW bf16: 8).  Returns G, -1 when not covered (nothing launched),
// -2 - hipError.
DDL_API int ddl_conv3_bwd(const void* dz, const void* x3, const float* mean3, const float* istd3, const float* coef3,
                          const void* a2, const void* x2, const uint8_t* mask2, const float* mean2, const float* istd2,
                          const void* wt, void* dz2, float* colstats, void* wpart, long wpart_elems, void* dW,
                          int dw_f32, int accumulate, long M, int Cout, int Cin, int grid, hipStream_t st) {
    if (Cout != 256 || Cin != 64 || M < 1 || M * (long)Cout * 2 >= (1l << 31)) return -1;
    if (!dz || !x3 || !mean3 || !istd3 || !coef3 || !a2 || !x2 || !mean2 || !istd2 || !wt || !dz2 || !colstats ||
        !wpart || !dW)
        return -1;
    for (const void* q : {dz, x3, a2, x2, wt, (const void*)dz2, (const void*)wpart})
        if ((uintptr_t)q & 15) return -1;
    if ((uintptr_t)dW & (dw_f32 ? 15 : 7)) return -1;
    C3Params p{};
    p.dz = (const bf16_t*)dz;
    p.x3 = (const bf16_t*)x3;
    p.mean3 = mean3;
    p.istd3 = istd3;
    p.coef3 = coef3;
    p.a2 = (const bf16_t*)a2;
    p.x2 = (const bf16_t*)x2;
    p.mask2 = mask2;
    p.mean2 = mean2;
    p.istd2 = istd2;
    p.wt = (const bf16_t*)wt;
    p.dz2 = (bf16_t*)dz2;
    p.colstats = colstats;
    p.wpart = (bf16_t*)wpart;
    p.M = M;
    p.tiles = (int)((M + TM - 1) / TM);
    const int G = ddl_conv3_bwd_grid(M, grid);
    p.chunk = 2 * (((int)((M + 63) / 64) + G - 1) / G);     // 32-row tiles per workgroup: whole 64-row tiles
    p.dz2_bytes = (uint32_t)(M * Cin * 2);
    if (wpart_elems < (long)G * Cout * Cin) return -1;
    hipLaunchKernelGGL((conv3_bwd_k<256, 64, 3>), dim3(G), dim3(NTH), 0, st, p);
    // the reduce of stream_wgrad_k (stream_gemm.hip): the same partials give the same bits
    ddl_wgrad_reduce(p.wpart, G, Cout, Cin, dW, Cin, accumulate, dw_f32, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return -2 - (int)e;
    return G;
}
