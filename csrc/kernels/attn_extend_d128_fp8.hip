// Rotary grouped-query chunk (extend) attention at HEAD DIM 128 over an FP8 KV CACHE: T new tokens per sequence
// attend to the dequantised cached keys and, causally, to the chunk's own keys as bf16; the chunk's queries and keys
// are rotated inside the launch and its rotated keys / values are quantised and appended.  The contract is
// attn_extend_d128.hip's (qkv_new, the rotary table, lens / new_lens / max_len, the zero rows, the dead-row rule) with
// attn_decode_d128_fp8.hip's cache format: kcache / vcache [B, Hkv, C, 128] e4m3 bytes, kscale / vscale [B, Hkv, C]
// fp32, element = value(byte) * scale[row]; a row is quantised as ops.quantize_fp8_rows defines it (scale = amax / 448
// as a true fp32 division, 1.0 for an all-zero row; byte = e4m3_rne(clamp(x / scale))).  Inside this launch the
// chunk is seen UNQUANTISED; every later call sees the appended rows quantised.  No cache row >= n, no scale >= n, no
// chunk row >= t and no table row past max_len + T - 1 is loaded: a staged row past the end of its part is a copy
// of the last valid row WITH THAT ROW'S SCALE, and its scores are replaced by -inf with a select.  With n = 0 no
// cache tile is staged.
//
// What is decided here (not attn_extend_d128.hip with a cast in front):
//
//   Two tile bodies, one LDS budget.  Cache tiles are walked first, in their own loop, chunk tiles after them.  A
//   cache tile is 64 keys landed AS BYTES by LDS-DMA, one tile ahead: 64 x 128 B = 8 KB per image, exactly the 8 KB
//   of a 32-key bf16 chunk tile, so both kinds share the 4 x 8 KB double buffer and a cached key costs half the
//   barriers and half the DMA instructions of the bf16 kernel.  The arithmetic of a cache tile runs as two halves
//   of 32 keys (two score blocks, one 32-deep P V step; the second half only if n reaches into it).  Scoring all 64
//   at once (16 score registers, half the rescales too) was built first: with the byte fragments' addresses it
//   spilled in eight of the eleven instances (8 - 58 scratch instructions), and the 8-wave instances have no
//   register to give at 128.  The alternative of 32-key byte tiles in a smaller buffer buys nothing: the chunk body
//   sizes the buffer at 32 KB either way.  The two loops keep only their own fragment addresses live, and the
//   FIRST chunk K tile is rotated on arrival (after the last cache tile's arithmetic: one exposed load per
//   workgroup) so that the cache loop carries no rotation units in flight; that is what brought every instance
//   under its budget without scratch.
//
//   Bytes become bf16 in registers, exactly.  K: the 8 consecutive bytes of a key row per lane (ds_read_b64),
//   widened by four v_cvt_scalef32_pk_bf16_fp8 at scale 1.0.  V: ONE ds_read_b64_tr_b8 per fragment -- the
//   transposing byte read was built, not the register transpose.  Measured on the device: within a row of 16
//   lanes, lane i's byte e is byte i & 7 of the 8 bytes addressed by lane 2 e + (i >> 3).  Every source lane gives
//   its own address, so the eight key rows of a fragment need not be adjacent: source lane j points at key row
//   16 (e >> 2) + 4 g + (e & 3), e = j >> 1, which is the accumulator's k order (a lane of S^T holds keys
//   16 blk + 4 g + r), and P goes from the score registers into the B operand without a shuffle.  The MFMA is the
//   bf16 16x16x32 one; Q is not quantised.
//
//   Swizzle of the byte images.  A 128-byte row is half a bank line: line L holds key rows 2 L and 2 L + 1 as 16
//   sixteen-byte slots, slot ((r & 1) << 3 | c) ^ bswz(L), bswz(L) = (L & 7) ^ ((L >> 1) & 4), for chunk c of row r.
//   K row reads (16 rows x one chunk per 32-lane pass): L & 7 runs over 0 .. 7 and r & 1 over both halves, 16
//   distinct slots.  V transposing reads (a pass is rows 4 g .. + 3 and 16 + 4 g .. + 3 for two g, one chunk): the
//   low rows give L & 7 in 0 .. 3 (or 4 .. 7), the rows 16 further the same XOR 4, again 16 distinct slots.  The DMA
//   lands linearly, each 16-byte slot of four lines written once per instruction; the permutation is on the global
//   side, within the 1 KB of eight consecutive cache rows.  All three were enumerated on the host.  The chunk tiles
//   keep attn_extend_d128.hip's patterns (xswz).
//
//   Scales.  A tile's 64 key scales and 64 value scales are one 4-byte-per-lane LDS-DMA instruction each, issued
//   with the tile into LDS beside the images (512 B per buffer; holding them in the registers of the lanes that own
//   the score rows would be 32 registers a tile ahead), and read back as one ds_read_b128 per score block, the same
//   address across a lane group.  The key scale times scale log2(e) multiplies the FINISHED fp32 score once; the
//   value scale is folded into p before p's one rounding to bf16; the softmax sum takes the unscaled p.
//
//   Work split: attn_extend_d128.hip's, all of it still paying -- grid (query tiles, Hkv, B), G x NS waves so a tile
//   is staged once for the G heads of its group, longest workgroups first, only a tile (half) that n or the
//   diagonal cuts pays the compare, and the "maxima did not move" rescale skip.
//
//   Append.  Once per KV head, by the workgroup that owns the chunk positions: a DPP row of 16 lanes per position
//   rotates the key again with the same function (the bits that were scored), takes the row's amax with the decode
//   kernel's four DPP max steps, quantises with its expressions (so the same bytes and scale as the native fill and
//   decode write for that row), and stores 8 bytes per lane and the scale from lane 0; the value row likewise.
//
// One launch; the grid and the instance follow from B, Hkv, G and T alone; no sync, no atomics, no scratch, no
// workspace; nothing this launch stores is read by it; bitwise repeatable.
//
// Registers.  VGPRs per instance <G, NS>, no scratch in any, 33 KB of LDS each (32 KB of images + 1 KB of scales);
// the launch bounds ask for 4 waves per SIMD from the 8-wave instances, 3 from 4 waves up, 2 from 2, 1 from <1,1>:
//   <1,1> 260  <1,2> 208  <1,4> 152  <2,1> 208  <2,2> 152  <2,4> 128  <3,1> 200  <3,2> 152  <4,1> 152  <4,2> 128
//   <8,1> 128.
// So a CU holds two workgroups of the 512-thread instances, three of the 256-thread ones, and of the narrow ones the
// four that 33 KB of LDS allows (the bf16 kernel: five): <1,1> is one wave per workgroup, so its 260 registers (one
// wave per SIMD) still fit those four.
#include "ddl_lds.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int ZD = 128;          // head dim
constexpr int ZH = ZD / 2;       // rotation distance
constexpr int ZTC = 64;          // cached keys per (byte) tile
constexpr int ZTK = 32;          // chunk keys per (bf16) tile
constexpr int ZROWB = 256;       // bytes per LDS line: one bf16 row, or two byte rows
constexpr int ZIMG = 8192;       // one image: 64 byte rows or 32 bf16 rows
constexpr int ZSCL = 4 * ZIMG;   // the scales: per buffer 64 key scales, then 64 value scales
constexpr int ZSMEM = ZSCL + 2 * 2 * ZTC * 4;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float E4M3_MAX = 448.f;

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) i32x2 lds_i2;

__device__ __forceinline__ uint4 ld16(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void st8(uint8_t* p, const uint2& u) { *reinterpret_cast<uint2*>(p) = u; }

// ---------------------------------------------------------------- byte images (cache tiles)
// slot permutation of line L (key rows 2 L, 2 L + 1) of a byte image (see the header)
__device__ __forceinline__ int bswz(int L) { return (L & 7) ^ ((L >> 1) & 4); }
// byte offset of 16-byte chunk c (0 .. 7) of key row r (0 .. 63)
__device__ __forceinline__ int bpos(int r, int c) {
    const int L = r >> 1;
    return L * ZROWB + ((((r & 1) << 3) | (c ^ bswz(L))) << 4);
}

// rows row0 .. row0 + 63 of a [rows][128] byte matrix into a swizzled byte image; rows >= rows_valid (>= 1) are
// copies of the last valid one.  8 one-KB instructions (4 lines = 8 rows each) dealt round-robin to the NW waves.
// The landing is linear (lane l at line 4 q + l / 16, slot l & 15); the permutation is on the global side.
template <int NW>
__device__ __forceinline__ void dma_bytes(const uint8_t* src, int row0, int rows_valid, char* dst, int wv, int lane) {
#pragma unroll
    for (int qq = 0; qq < (8 + NW - 1) / NW; ++qq) {
        const int q = qq * NW + wv;
        if (8 % NW == 0 || q < 8) {
            const int L = q * 4 + (lane >> 4), s = lane & 15;
            const int r = 2 * L + (s >> 3), c = (s & 7) ^ bswz(L);
            const long gr = min(row0 + r, rows_valid - 1);
            glds16(src + gr * ZD + c * 16, dst + q * 1024);     // default policy: every query tile re-reads it
        }
    }
}

// 8 e4m3 bytes (byte i = element i) -> 8 bf16, exactly: four packed converts at scale 1
__device__ __forceinline__ bf16x8 e4m3x8_to_bf16(uint32_t lo, uint32_t hi) {
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
    const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
    const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
    return (bf16x8){a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// fragment: key rows rbase .. +15 (lane & 15), k = 32 kk + 8 (lane >> 4) + 0..7, from the byte K image
__device__ __forceinline__ bf16x8 frag_kb(const char* img, int rbase, int kk, int lane) {
    const int r = rbase + (lane & 15), g = lane >> 4;
    const uint2 u = *reinterpret_cast<const uint2*>(img + bpos(r, 2 * kk + (g >> 1)) + 8 * (g & 1));
    return e4m3x8_to_bf16(u.x, u.y);
}

// (through a restrict-qualified parameter, as ddl_lds.h's lds_read_tr: the read then carries alias-scope metadata
// and draws no vmcnt(0) against the LDS-DMA in flight)
__device__ __forceinline__ i32x2 lds_read_tr_b8(lds_i2* __restrict__ p) {
    return __builtin_amdgcn_ds_read_tr8_b64_v2i32(p);
}

// transposed fragment of the byte V image in the accumulator's k order: lane gets column 16 db + (lane & 15) of
// key rows 32 t + 16 hh + 4 g + {0..3}, hh = 0, 1.  ONE ds_read_b64_tr_b8: within a row of 16 lanes, lane i's
// byte e comes from byte i & 7 of the 8 bytes that lane 2 e + (i >> 3) addresses (measured), so source lane j
// points at key row e = j >> 1 of the eight and at columns 16 db + 8 (j & 1) ..
__device__ __forceinline__ bf16x8 frag_vtb(const char* img, int t, int db, int lane) {
    const int g = lane >> 4, e = (lane >> 1) & 7;
    const int r = 32 * t + 16 * (e >> 2) + 4 * g + (e & 3);
    const i32x2 u = lds_read_tr_b8((lds_i2*)(img + bpos(r, db) + 8 * (lane & 1)));
    return e4m3x8_to_bf16((uint32_t)u[0], (uint32_t)u[1]);
}

// ---------------------------------------------------------------- bf16 images (chunk tiles): attn_extend_d128.hip's
// slot permutation of row r of a bf16 image
__device__ __forceinline__ int xswz(int r) { return ((r & 7) << 1) | ((r >> 3) & 1); }

// rows row0 .. row0 + 31 of a [rows][ld] bf16 matrix (128 columns used) into a swizzled image; rows >= rows_valid
// (>= 1) are copies of the last valid one.  8 one-KB instructions (4 rows each) dealt round-robin to the waves.
template <int NW>
__device__ __forceinline__ void dma_tile(const bf16_t* src, long ld, int row0, int rows_valid, char* dst, int wv,
                                         int lane) {
#pragma unroll
    for (int qq = 0; qq < (8 + NW - 1) / NW; ++qq) {
        const int q = qq * NW + wv;
        if (8 % NW == 0 || q < 8) {
            const int r = q * 4 + (lane >> 4);
            const int c = (lane & 15) ^ xswz(r);
            const long gr = min(row0 + r, rows_valid - 1);
            glds16(src + gr * ld + c * 8, dst + q * 1024);
        }
    }
}

// One rotation unit: columns W cw .. + W - 1 and 64 + W cw .. + W - 1 of one head of one token (W = 8: a pair of
// 16-byte pieces; W = 4: half of one, 8-byte pieces), with the W cos and W sin values of its table row.
template <int W>
struct RotIn {
    uint32_t a[W / 2], b[W / 2];
    float c[W], sn[W];
};
template <int W>
__device__ __forceinline__ void ldw(const bf16_t* p, uint32_t* u) {
    if constexpr (W == 8) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        u[0] = v.x; u[1] = v.y; u[2] = v.z; u[3] = v.w;
    } else {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        u[0] = v.x; u[1] = v.y;
    }
}
template <int W, typename P>
__device__ __forceinline__ void stw(P* p, const uint32_t* u) {
    if constexpr (W == 8) *reinterpret_cast<uint4*>(p) = make_uint4(u[0], u[1], u[2], u[3]);
    else *reinterpret_cast<uint2*>(p) = make_uint2(u[0], u[1]);
}
template <int W>
__device__ __forceinline__ RotIn<W> rot_load(const bf16_t* head, const float* tabrow, int cw) {
    RotIn<W> r;
    ldw<W>(head + W * cw, r.a);
    ldw<W>(head + ZH + W * cw, r.b);
    if constexpr (W == 8) {
        load8(tabrow + W * cw, r.c);
        load8(tabrow + ZH + W * cw, r.sn);
    } else {
        load4(tabrow + W * cw, r.c);
        load4(tabrow + ZH + W * cw, r.sn);
    }
    return r;
}
// rope_qkv_fwd_k's expressions, operand order included; each half rounded once
template <int W>
__device__ __forceinline__ void rot_apply(const RotIn<W>& r, uint32_t* lo, uint32_t* hi) {
#pragma unroll
    for (int e = 0; e < W / 2; ++e) {
        const float x1[2] = {lo_f(r.a[e]), hi_f(r.a[e])}, x2[2] = {lo_f(r.b[e]), hi_f(r.b[e])};
        float o1[2], o2[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            o1[k] = x1[k] * r.c[2 * e + k] - x2[k] * r.sn[2 * e + k];
            o2[k] = x2[k] * r.c[2 * e + k] + x1[k] * r.sn[2 * e + k];
        }
        lo[e] = pack2bf(o1[0], o1[1]);
        hi[e] = pack2bf(o2[0], o2[1]);
    }
}

// fragment: key rows rbase .. +15 (lane & 15), k = 32 kk + 8 (lane >> 4) + 0..7, from the bf16 K image
__device__ __forceinline__ bf16x8 frag_k(const char* img, int rbase, int kk, int lane) {
    const int r = rbase + (lane & 15);
    return *reinterpret_cast<const bf16x8*>(img + r * ZROWB + (((kk * 4 + (lane >> 4)) ^ xswz(r)) << 4));
}

// transposed fragment of the bf16 V image in the accumulator k order: lane gets column cbase + (lane & 15) of rows
// 16 hh + 4 g + {0..3}, hh = 0, 1
__device__ __forceinline__ bf16x8 frag_vt(const char* img, int cbase, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int chunk = (cbase + 4 * p) >> 3;
    const int ra = 4 * g + q, rb = ra + 16;
    const s16x4 lo = lds_read_tr((lds_v4*)(img + ra * ZROWB + ((chunk ^ xswz(ra)) << 4) + (p & 1) * 8));
    const s16x4 hi = lds_read_tr((lds_v4*)(img + rb * ZROWB + ((chunk ^ xswz(rb)) << 4) + (p & 1) * 8));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, r);
}

__device__ __forceinline__ bf16x8 pack_p(const f32x4& a, const f32x4& b) {
    bf16x8 r;
    r[0] = (__bf16)a[0]; r[1] = (__bf16)a[1]; r[2] = (__bf16)a[2]; r[3] = (__bf16)a[3];
    r[4] = (__bf16)b[0]; r[5] = (__bf16)b[1]; r[6] = (__bf16)b[2]; r[7] = (__bf16)b[3];
    return r;
}

// ---------------------------------------------------------------- the append's quantiser: attn_decode_d128_fp8.hip's
// Max over the 16 lanes of a DPP row (every lane of the row gets it).
template <int CTRL>
__device__ __forceinline__ float dpp_max(float v) {
    return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF,
                                                                          0xF, false)));
}
__device__ __forceinline__ float row16_max(float v) {
    v = dpp_max<0xB1>(v);    // quad_perm [1,0,3,2]
    v = dpp_max<0x4E>(v);    // quad_perm [2,3,0,1]
    v = dpp_max<0x141>(v);   // row_half_mirror
    return dpp_max<0x140>(v);   // row_mirror
}
// This lane's 8 bf16 elements (four packed words) of a 128-wide row held by the 16 lanes of a DPP row -> its 8
// bytes and the row's scale (the same bits in every lane): ops.quantize_fp8_rows on that row.
__device__ __forceinline__ uint2 quant_row8(const uint32_t* w, float& sc) {
    float x[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        x[2 * e] = lo_f(w[e]);
        x[2 * e + 1] = hi_f(w[e]);
    }
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) a = fmaxf(a, fabsf(x[i]));
    a = row16_max(a);
    sc = a > 0.f ? a / E4M3_MAX : 1.f;
    float y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = fminf(fmaxf(x[i] / sc, -E4M3_MAX), E4M3_MAX);
    uint2 u;
    u.x = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
    u.x = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], (int)u.x, true);
    u.y = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
    u.y = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], (int)u.y, true);
    return u;
}

template <int G, int NS>
__global__ __launch_bounds__(64 * G * NS, (G * NS >= 8 ? 4 : (G * NS >= 4 ? 3 : (G * NS >= 2 ? 2 : 1))))
void attn_extend_d128_fp8_k(
    const bf16_t* __restrict__ qkv, const float* __restrict__ tab, uint8_t* __restrict__ kcache,
    uint8_t* __restrict__ vcache, float* __restrict__ kscale, float* __restrict__ vscale,
    const int* __restrict__ lens, const int* __restrict__ new_lens, bf16_t* __restrict__ out, int T, int Hkv, int C,
    int max_len, float scale) {
    constexpr int NW = G * NS, NT = 64 * NW, TQ = 16 * NS;
    // a chunk K tile's rotation units, as in attn_extend_d128.hip: 256 pairs (W = 8), or 512 half-pairs (W = 4)
    // in the 512-thread instances; NU per thread; the 64-thread instance rotates on arrival
    constexpr int W = NT >= 512 ? 4 : 8, UPR = ZH / W, UNITS = ZTK * UPR;
    constexpr int NU = (UNITS + NT - 1) / NT;
    constexpr bool ARRIVE = NU > 2;
    __shared__ __attribute__((aligned(16))) char smem[ZSMEM];   // K0 V0 K1 V1, then the scales of the two buffers
    const int qt = (int)(gridDim.x - 1 - blockIdx.x), hkv = blockIdx.y, b = blockIdx.z;   // longest loop first
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4;
    const int hg = wv / NS, sub = wv % NS;      // this wave's query head of the group and its 16-query sub-tile
    const int H = Hkv * G, h = hkv * G + hg;
    // a lens beyond the host's bound, or a new_lens outside 1 .. T, would index past the cache, the table or the
    // chunk: clamp (the result is then the caller's problem, every access stays in bounds)
    const int n = min(max(lens[b], 0), max_len);
    const int tl = new_lens ? min(max(new_lens[b], 1), T) : T;

    const long HD = (long)H * ZD, rs = (long)(H + 2 * Hkv) * ZD;
    const bf16_t* rowb = qkv + (long)b * T * rs;
    const bf16_t* qb = rowb + (long)h * ZD;
    const bf16_t* kb = rowb + (long)(H + hkv) * ZD;
    const bf16_t* vb = rowb + (long)(H + Hkv + hkv) * ZD;
    const float* tb = tab + (long)n * ZD;                       // the table row of chunk position 0
    const long hrow = ((long)b * Hkv + hkv) * C;                // this head's first cache row (and scale)
    uint8_t* ck = kcache + hrow * ZD;
    uint8_t* cv = vcache + hrow * ZD;
    float* sk = kscale + hrow;
    float* sv = vscale + hrow;
    const int q0 = qt * TQ, q0w = q0 + 16 * sub, myq = q0w + (lane & 15);
    bf16_t* orow = out + ((long)b * T + myq) * HD + (long)h * ZD + 4 * g;

    if (q0 >= tl) {     // padded queries only: zeros, nothing to append
        if (myq < T) {
#pragma unroll
            for (int db = 0; db < 8; ++db) *reinterpret_cast<uint2*>(orow + 16 * db) = make_uint2(0u, 0u);
        }
        return;
    }

    // append, once per KV head: this workgroup's chunk positions q0 .. q0 + TQ - 1 (those < tl).  A DPP row of 16
    // lanes owns a position: lane s rotates pair s & 7 once more (the same function, so the bits that are scored)
    // and keeps its low (s < 8) or high half, 8 columns 8 s ..; the key row and the value row are then quantised
    // as the decode kernel does (amax over the row of lanes, a true division, the packed convert) and stored as
    // 8 bytes per lane, the two scales by lane 0.  (16 TQ is a multiple of 64 and so is NT: a row of lanes is
    // inside or outside as a whole, and the DPP reads stay inside active lanes.)
#pragma unroll
    for (int i = 0; i < (16 * TQ + NT - 1) / NT; ++i) {
        const int unit = tid + i * NT;
        if ((16 * TQ) % NT == 0 || unit < 16 * TQ) {
            const int j = q0 + (unit >> 4), jc = min(j, tl - 1), s16 = unit & 15;
            const RotIn<8> ri = rot_load<8>(kb + (long)jc * rs, tb + (long)jc * ZD, s16 & 7);
            uint32_t lo[4], hi[4], kw[4];
            rot_apply<8>(ri, lo, hi);
#pragma unroll
            for (int e = 0; e < 4; ++e) kw[e] = s16 < 8 ? lo[e] : hi[e];
            const uint4 vraw = ld16(vb + (long)jc * rs + s16 * 8);
            const uint32_t vw[4] = {vraw.x, vraw.y, vraw.z, vraw.w};
            float ksc, vsc;
            const uint2 kq = quant_row8(kw, ksc), vq = quant_row8(vw, vsc);
            if (j < tl) {
                st8(ck + (long)(n + j) * ZD + s16 * 8, kq);
                st8(cv + (long)(n + j) * ZD + s16 * 8, vq);
                if (s16 == 0) {
                    sk[n + j] = ksc;
                    sv[n + j] = vsc;
                }
            }
        }
    }

    // Q fragments (B operand of S^T = K Q^T): lane holds Q[myq][32 kk + 8 g + 0..7], rotated: fragments kk and
    // kk + 2 are the two halves of a pair
    bf16x8 qf[4];
    {
        const int jq = min(myq, tl - 1);
        const bf16_t* qr = qb + (long)jq * rs;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const RotIn<8> ri = rot_load<8>(qr, tb + (long)jq * ZD, 4 * kk + g);
            uint32_t lo[4], hi[4];
            rot_apply<8>(ri, lo, hi);
            qf[kk] = __builtin_bit_cast(bf16x8, make_uint4(lo[0], lo[1], lo[2], lo[3]));
            qf[kk + 2] = __builtin_bit_cast(bf16x8, make_uint4(hi[0], hi[1], hi[2], hi[3]));
        }
    }

    const int nc = (n + ZTC - 1) / ZTC;                         // cache tiles (64 keys, bytes)
    const int nd = min(q0 + TQ - 1, tl - 1) / ZTK + 1;           // chunk tiles (32 keys, bf16), through the last diagonal one
    const int ntot = nc + nd;
    RotIn<W> kin[ARRIVE ? 1 : NU];                               // the next chunk K tile's units, in flight
    auto unit_load = [&](int row0, int unit) __attribute__((always_inline)) {
        const int jc = min(row0 + unit / UPR, tl - 1);
        return rot_load<W>(kb + (long)jc * rs, tb + (long)jc * ZD, unit % UPR);
    };
    // issue tile i: DMA for everything but a chunk K tile, whose units go to registers.  A cache tile's 64 key
    // scales and 64 value scales are one 4-byte-per-lane DMA instruction each (wave 0, and wave 1 where there is
    // one), clamped like the rows, so a staged copy of the last valid row has that row's scale
    auto stage = [&](auto holdc, int i, int buf) __attribute__((always_inline)) {
        char* sK = smem + buf * 2 * ZIMG;
        if (i < nc) {
            dma_bytes<NW>(ck, i * ZTC, n, sK, wv, lane);
            dma_bytes<NW>(cv, i * ZTC, n, sK + ZIMG, wv, lane);
            char* sS = smem + ZSCL + buf * (2 * ZTC * 4);
            const int jr = min(i * ZTC + lane, n - 1);
            if (wv == 0) glds4(sk + jr, sS);
            if (wv == (NW > 1 ? 1 : 0)) glds4(sv + jr, sS + ZTC * 4);
        } else {
            const int row0 = (i - nc) * ZTK;
            dma_tile<NW>(vb, rs, row0, tl, sK + ZIMG, wv, lane);
            if constexpr (decltype(holdc)::value) {
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int unit = tid + u * NT;
                    if (UNITS % NT == 0 || unit < UNITS) kin[u] = unit_load(row0, unit);
                }
            }
        }
    };
    // rotate a chunk K tile's units and write them into the swizzled bf16 K image: the low piece first on even
    // rows, the high piece first on odd rows
    auto land = [&](auto holdc, int i, int buf) __attribute__((always_inline)) {
        if (i < nc) return;
        char* sK = smem + buf * 2 * ZIMG;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int unit = tid + u * NT;
            if (UNITS % NT == 0 || unit < UNITS) {
                const int r = unit / UPR, cw = unit % UPR;
                const bool odd = r & 1;
                uint32_t lo[W / 2], hi[W / 2], first[W / 2], second[W / 2];
                if constexpr (!decltype(holdc)::value) rot_apply<W>(unit_load((i - nc) * ZTK, unit), lo, hi);
                else rot_apply<W>(kin[u], lo, hi);
#pragma unroll
                for (int e = 0; e < W / 2; ++e) {
                    first[e] = odd ? hi[e] : lo[e];
                    second[e] = odd ? lo[e] : hi[e];
                }
                char* rowp = sK + r * ZROWB + ((2 * W * cw) & 15);
                const int ch = (W * cw) >> 3, sw = xswz(r);
                stw<W>(rowp + (((ch + (odd ? 8 : 0)) ^ sw) << 4), first);
                stw<W>(rowp + (((ch + (odd ? 0 : 8)) ^ sw) << 4), second);
            }
        }
    };

    const float c2 = scale * LOG2E;                              // scores in the exp2 domain
    const bool active = q0w < tl;                                // per wave: it has a valid query
    float m = -INFINITY, lsum = 0.f;
    f32x4 o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // The arithmetic of 32 keys: half hf of cache tile i (FP8), or chunk tile i.  Two score blocks of 16 keys and
    // one 32-deep P V step; lane holds s[blk][r] = score(q = myq, key0 + 16 blk + 4 g + r).
    auto body = [&](auto fp8c, int i, int hf) __attribute__((always_inline)) {
        constexpr bool FP8 = decltype(fp8c)::value;
        constexpr int NB = 2;
        const char* sK = smem + (i & 1) * 2 * ZIMG;
        const char* sV = sK + ZIMG;
        const float* sS = reinterpret_cast<const float*>(smem + ZSCL + (i & 1) * (2 * ZTC * 4)) + 32 * hf + 4 * g;
        const int key0 = FP8 ? i * ZTC + 32 * hf : (i - nc) * ZTK;
        // keys key0 + j of this part are visible to this lane's query while key0 + j < limit
        const int limit = FP8 ? n : myq + 1;
        const bool cut = FP8 ? key0 + ZTK > n : key0 + ZTK - 1 > q0w;     // per wave
        f32x4 s[NB];
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) {
            s[blk] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                bf16x8 kf;
                if constexpr (FP8) kf = frag_kb(sK, 32 * hf + 16 * blk, kk, lane);
                else kf = frag_k(sK, 16 * blk, kk, lane);
                s[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], s[blk], 0, 0, 0);
            }
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) {
            const int k0 = key0 + 16 * blk + 4 * g;
            // the key's scale meets its finished score once, together with 1 / sqrt(D) and log2(e)
            f32x4 kc = (f32x4){c2, c2, c2, c2};
            if constexpr (FP8) kc = *reinterpret_cast<const f32x4*>(sS + 16 * blk) * c2;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = s[blk][r] * kc[r];
                if (cut && k0 + r >= limit) v = -INFINITY;
                s[blk][r] = v;
                tmax = fmaxf(tmax, v);
            }
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mnew = fmaxf(m, tmax);
        const float alpha = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - mnew);
        m = mnew;
        float psum = 0.f;
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = __builtin_amdgcn_exp2f(s[blk][r] - mnew);
                psum += pv;                         // (the sum takes the unscaled p)
                s[blk][r] = pv;
            }
        }
        lsum = lsum * alpha + psum;
        // (wave-uniform: no lane's maximum moved, every alpha is exactly 1)
        if (__builtin_amdgcn_ballot_w64(alpha != 1.f)) {
#pragma unroll
            for (int db = 0; db < 8; ++db) o[db] *= alpha;
        }
        // ---- O^T[d][q] += V^T[d][k] P^T[k][q]: a 32-deep step per 16-column block; the value's scale goes into p
        // before p's one rounding
        if constexpr (FP8) {
            s[0] *= *reinterpret_cast<const f32x4*>(sS + ZTC);
            s[1] *= *reinterpret_cast<const f32x4*>(sS + ZTC + 16);
        }
        const bf16x8 pf = pack_p(s[0], s[1]);
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            bf16x8 vf;
            if constexpr (FP8) vf = frag_vtb(sV, hf, db, lane);
            else vf = frag_vt(sV, 16 * db, lane);
            o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[db], 0, 0, 0);
        }
    };

    // Cache tiles first, chunk tiles after them: two loops, so each keeps only its own fragment addresses live.
    // The first chunk K tile is rotated on arrival (loaded, rotated and stored after the last cache tile's
    // arithmetic: one exposed load per workgroup), so the cache loop carries no rotation units in flight; the
    // later ones are held in registers a tile ahead, as in attn_extend_d128.hip.
    constexpr std::false_type arrive{};
    constexpr std::integral_constant<bool, !ARRIVE> hold{};
    stage(arrive, 0, 0);
    land(arrive, 0, 0);
    for (int i = 0; i < nc; ++i) {
        // tile i has landed (this wave's DMA, then everyone's); everyone is done with the other image pair
        LGKM0();
        VMN(0);
        BARRIER();
        stage(arrive, i + 1, (i + 1) & 1);                      // (there is always a chunk tile after the cache)
        if (active) {
            // the tile's first key is live; its second half is scored only if n reaches into it
            const int nh = i * ZTC + ZTK < n ? 2 : 1;
#pragma unroll 1
            for (int hf = 0; hf < nh; ++hf) body(std::true_type{}, i, hf);
        }
        land(arrive, i + 1, (i + 1) & 1);
    }
    for (int i = nc; i < ntot; ++i) {
        // ... and this wave's LDS stores of rotated keys
        LGKM0();
        VMN(0);
        BARRIER();
        // (none after the last tile: LDS-DMA must not be landing when the workgroup exits)
        if (i + 1 < ntot) stage(hold, i + 1, (i + 1) & 1);
        // a chunk tile that starts past this wave's last query holds nothing for it (it still stages and keeps the
        // barriers); every query of a scoring wave sees the tile's first key
        if (active && (i - nc) * ZTK <= q0w) body(std::false_type{}, i, 0);
        if (i + 1 < ntot) land(hold, i + 1, (i + 1) & 1);
    }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    if (myq >= T) return;
    const bool qok = myq < tl;                                   // (then lsum >= 1: its own key)
    const float inv = qok ? 1.f / lsum : 0.f;
#pragma unroll
    for (int db = 0; db < 8; ++db) {
        const float v[4] = {qok ? o[db][0] * inv : 0.f, qok ? o[db][1] * inv : 0.f, qok ? o[db][2] * inv : 0.f,
                            qok ? o[db][3] * inv : 0.f};
        store4(orow + 16 * db, v);
    }
}

inline bool z_group_ok(int H, int Hkv) {
    if (Hkv < 1 || H < Hkv || H % Hkv) return false;
    const int G = H / Hkv;
    return G == 1 || G == 2 || G == 3 || G == 4 || G == 8;
}

// 16-query sub-tiles per workgroup: attn_extend_d128.hip's rule (1 / 2 / 4, capped so that G NS <= 8 waves), so
// ddl_attn_extend_gqa_d128_tile answers for this kernel too
inline int z_subtiles(int T, int G) {
    const int want = T <= 16 ? 1 : (T <= 32 ? 2 : 4);
    const int cap = G >= 8 ? 1 : (G >= 3 ? 2 : 4);
    return std::min(want, cap);
}

}  // namespace

// 1 when the head-dim-128 extend kernel on an FP8 cache has an instance for this group size
DDL_API int ddl_attn_extend_gqa_d128_fp8_supported(int H, int Hkv) { return z_group_ok(H, Hkv) ? 1 : 0; }

// kcache / vcache: e4m3 bytes [B, Hkv, C, 128], 16-byte aligned; kscale / vscale: fp32 [B, Hkv, C]
DDL_API int ddl_attn_extend_gqa_d128_fp8(const void* qkv_new, const float* tab, void* kcache, void* vcache,
                                         void* kscale, void* vscale, const void* lens, const void* new_lens,
                                         void* out, int B, int T, int H, int Hkv, int C, int max_len, long n_pos,
                                         float scale, hipStream_t st) {
    if (!z_group_ok(H, Hkv)) return (int)hipErrorInvalidValue;
    if (B <= 0 || T <= 0) return 0;
    if (max_len < 0 || (long)max_len + T > C || (long)max_len + T > n_pos || Hkv > 65535 || B > 65535 ||
        ((uintptr_t)kcache | (uintptr_t)vcache) % 16)
        return (int)hipErrorInvalidValue;
    const int G = H / Hkv;
#define Z_LAUNCH(G_, NS_)                                                                                              \
    attn_extend_d128_fp8_k<G_, NS_><<<dim3((T + 16 * NS_ - 1) / (16 * NS_), Hkv, B), 64 * G_ * NS_, 0, st>>>(          \
        (const bf16_t*)qkv_new, tab, (uint8_t*)kcache, (uint8_t*)vcache, (float*)kscale, (float*)vscale,              \
        (const int*)lens, (const int*)new_lens, (bf16_t*)out, T, Hkv, C, max_len, scale)
    switch (G * 8 + z_subtiles(T, G)) {
        case 1 * 8 + 1: Z_LAUNCH(1, 1); break;
        case 1 * 8 + 2: Z_LAUNCH(1, 2); break;
        case 1 * 8 + 4: Z_LAUNCH(1, 4); break;
        case 2 * 8 + 1: Z_LAUNCH(2, 1); break;
        case 2 * 8 + 2: Z_LAUNCH(2, 2); break;
        case 2 * 8 + 4: Z_LAUNCH(2, 4); break;
        case 3 * 8 + 1: Z_LAUNCH(3, 1); break;
        case 3 * 8 + 2: Z_LAUNCH(3, 2); break;
        case 4 * 8 + 1: Z_LAUNCH(4, 1); break;
        case 4 * 8 + 2: Z_LAUNCH(4, 2); break;
        case 8 * 8 + 1: Z_LAUNCH(8, 1); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef Z_LAUNCH
    DDL_RETURN_LAUNCH();
}
