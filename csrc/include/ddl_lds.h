// The kernels' LDS and LDS-DMA vocabulary: one definition of each primitive the MFMA kernels stage
// and read their operands with (gemm*.hip, stream_gemm.hip, skinny_gemm.hip, conv3*.hip,
// stem_conv.hip, attention.hip).  Small inline functions only -- layouts that belong to one kernel
// (its own swizzle, its issue_* loops, its parameter structs) stay in that kernel's file.
//
// Naming rule.  ds_*(uint32_t addr, ...) is UNTRACKED: an `asm volatile` LDS instruction on a 32-bit
// LDS byte address that the compiler knows nothing about.  It inserts no wait for it, so the caller
// places the `s_waitcnt lgkmcnt` (LGKM0()) before the first use of a result, and nothing may touch
// the result before that wait.  lds_*(pointer) is TRACKED: a builtin or plain access the compiler
// orders and waits for itself.
#pragma once
#include "ddl_common.h"

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) s16x4 lds_v4;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- waits and barriers
#define BARRIER() __builtin_amdgcn_s_barrier()
#define LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define VMN(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")

// s_waitcnt vmcnt(n) for a workgroup-uniform run-time n (the counts conv3_bwd.hip's ring produces)
__device__ __forceinline__ void wait_vm(int n) {
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}

// ---------------------------------------------------------------- untracked LDS access
__device__ __forceinline__ bf16x8 ds_read16(uint32_t addr) {
    bf16x8 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
    return v;
}
// ... with a compile-time offset: a per-lane base + immediates keeps a tile's many fragment addresses
// out of the register file
template <int OFF>
__device__ __forceinline__ bf16x8 ds_read16_off(uint32_t addr) {
    bf16x8 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
    return v;
}
__device__ __forceinline__ uint2 ds_read8(uint32_t addr) {
    uint2 v;
    asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"(addr));
    return v;
}
__device__ __forceinline__ uint32_t ds_read32(uint32_t addr) {
    uint32_t v;
    asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(addr));
    return v;
}
__device__ __forceinline__ void ds_write8(uint32_t addr, uint2 v) {
    asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void ds_write16(uint32_t addr, u32x4 v) {
    asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
// Transposing read (ds_read_b64_tr_b16), untracked: tracked ones drew lgkmcnt(0) waits in the
// middle of the MFMA stream.
__device__ __forceinline__ s16x4 ds_read_tr8(uint32_t addr) {
    s16x4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr));
    return v;
}
// k-major fragment (rows = the image's columns) from the two transposing reads at LDS addresses a, b
__device__ __forceinline__ bf16x8 tr_frag(uint32_t a, uint32_t b) {
    const s16x4 lo = ds_read_tr8(a), hi = ds_read_tr8(b);
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, r);
}

// ---------------------------------------------------------------- tracked transposing read
// Transposed LDS read through a restrict-qualified parameter: inlined, the read
// carries alias-scope metadata, which is what keeps the compiler's LDS-DMA tracking
// from putting an `s_waitcnt vmcnt(0)` in front of every ds_read_b64_tr_b16 (a bare
// builtin read has no alias info, so it waited out ALL in-flight operand DMA -- the
// whole 3-half-tile prefetch of the reduction-outer (NN / TN) kernels, every phase).
// The schedule's own counted vmcnt waits + barriers order DMA and reads.
__device__ __forceinline__ s16x4 lds_read_tr(lds_v4* __restrict__ p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16(p);
}

// ---------------------------------------------------------------- LDS-DMA
// One wave instruction: each lane's 16 (4) bytes at g land at dst + 16 (4) * lane, dst wave-uniform.
// glds16 has the default cache policy, glds16_nt the non-temporal one; which one a kernel wants is
// a fact about how often it re-reads the source, stated at its call sites.
__device__ __forceinline__ void glds16(const void* g, char* dst) {
    __builtin_amdgcn_global_load_lds(g, (lds_void*)dst, 16, 0, 0);
}
__device__ __forceinline__ void glds16_nt(const void* g, char* dst) {
    __builtin_amdgcn_global_load_lds(g, (lds_void*)dst, 16, 0, 2);
}
__device__ __forceinline__ void glds4(const void* g, char* dst) {
    __builtin_amdgcn_global_load_lds(g, (lds_void*)dst, 4, 0, 0);
}
// buffer resource over [p, p + bytes): raw buffer accesses past the end are dropped
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}

// ---------------------------------------------------------------- GEMM operand images
// k-contiguous 16-row x 32-k subtile (1 KB, 64-byte rows): the st_16x32 swizzle of a byte offset
__device__ __forceinline__ int swz_kc(int b) { return b ^ (((b >> 9) & 1) << 5); }
// k-outer image (256-byte rows of 128 columns): 16-byte chunk c of k-row r sits at chunk c ^ swz_ko(r)
__device__ __forceinline__ int swz_ko(int r) { return 2 * ((r & 3) | (((r >> 3) & 1) << 2)); }
// 16 columns (col_base .. + 15) x 32 k-rows of a k-outer image as an MFMA operand fragment: lane holds
// column col_base + (lane & 15), k = 8 (lane >> 4) .. + 7 (two tracked transposing reads of 4 rows)
__device__ __forceinline__ bf16x8 frag_ko(const char* img, int col_base, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, pq = lane & 3;
    const int chunk = (col_base + 4 * pq) >> 3;
    const int ra = 8 * g + q, rb = ra + 4;
    const s16x4 lo = lds_read_tr((lds_v4*)(img + ra * 256 + ((chunk ^ swz_ko(ra)) << 4) + (pq & 1) * 8));
    const s16x4 hi = lds_read_tr((lds_v4*)(img + rb * 256 + ((chunk ^ swz_ko(rb)) << 4) + (pq & 1) * 8));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, r);
}

// ---------------------------------------------------------------- swizzled row images
// [rows][W] bf16 image: 16-byte chunk c of row r sits at chunk c ^ (r & swm<W>()): the 16 rows a
// ds_read_b128 lane group touches land on 16 distinct 16-byte slots of the bank row
template <int W>
constexpr int swm() { return W / 8 >= 16 ? 15 : W / 8 - 1; }

// NROWS rows of W bf16 columns (row stride LD elements) into a swizzled [NROWS][W] LDS image by
// non-temporal LDS-DMA from the NWAVES waves of the workgroup (this one is wv): a fixed
// (compile-time) number of 1 KB instructions per wave, so the waits can count them
template <int NWAVES, int W, int NROWS, long LD = W>
__device__ __forceinline__ void dma_rows(const bf16_t* src, long row0, long rows_valid, char* dst, int wv, int lane) {
    constexpr int CPR = W / 8;                    // 16-byte chunks per row
    constexpr int RPI = CPR >= 64 ? 1 : 64 / CPR; // rows per 1 KB wave instruction
    constexpr int IPR = CPR >= 64 ? CPR / 64 : 1; // instructions per row (W > 512)
    constexpr int NINST = NROWS * IPR / RPI;
    static_assert(NINST % NWAVES == 0, "instructions split evenly over the waves");
#pragma unroll
    for (int qq = 0; qq < NINST / NWAVES; ++qq) {
        const int q = qq * NWAVES + wv;
        const int r = (q / IPR) * RPI + (CPR >= 64 ? 0 : lane / CPR);
        const int cl = CPR >= 64 ? (q % IPR) * 64 + lane : lane % CPR;
        const int c = cl ^ (r & swm<W>());
        const long gr = min(row0 + r, rows_valid - 1);   // rows past the end: any valid row
        glds16_nt(src + gr * LD + c * 8, dst + q * 1024);
    }
}
