// Rotary grouped-query chunk (extend) attention over a KV cache at HEAD DIM 128: T new tokens per sequence attend
// to the cached keys and, causally, to the chunk's own keys; the chunk's queries and keys are rotated inside the
// launch and its rotated keys / bit-copied values are appended.  Llama-2-7B (32 / 32 heads), Llama-3-8B and
// Mistral-7B (32 / 8).  Forward only, bf16.  The contract is attn_extend.hip's rotary one with D = 128:
//
// qkv_new [B, T, (H + 2 Hkv) 128] is the chunk's fused, UNROTATED projection [q heads | k heads | v heads]
// (G = H / Hkv in {1, 2, 3, 4, 8}); kcache / vcache [B, Hkv, C, 128] hold ROTATED keys; tab [n_pos, 128] is the fp32
// rotary table (row s = [cos 0..63 | sin 0..63]); lens [B] and the optional new_lens [B] are int32 on the device.
// For batch row b with n = lens[b] (clamped to 0 .. max_len) and t = new_lens[b] (clamped to 1 .. T; T without
// new_lens), chunk token i < t has its query and key heads rotated by table row n + i (HF half-split pairs
// i / i + 64 in fp32, the expressions and operand order of llama.hip's rope_qkv_fwd_k, rounded ONCE to bf16);
// query i of head h attends to cached keys 0 .. n-1 of KV head h / G and to the rotated chunk keys 0 .. i of that
// head; out [B, T, H 128] rows i >= t are zero bits.  The rotated key and the value of chunk positions i < t are
// stored to cache[b, :, n + i]; nothing else in the cache changes and lens / new_lens are not written.  No cache
// row >= n, no chunk row >= t and no table row past max_len + T - 1 is loaded: a staged row past the end of its
// part is a copy of that part's last valid row and its scores are replaced by -inf with a select.
//
// What is decided here (not the D = 64 file with a constant doubled):
//
//   Tile shape and LDS.  Keys come in tiles of 32, not 64: a K + V double buffer is 4 x 8 KB = 32 KB.  The
//   choice follows from occupancy.  The 8-wave instances (below) need 2 waves per SIMD per workgroup and at their
//   register counts a CU holds two of them with either tile, so 64-key tiles (64 KB, 128 KB for the two) would
//   buy the wide instances only half the barriers; but the narrow ones -- G waves per workgroup at T <= 16, the
//   chunk sizes of prefix reuse and speculative verification -- would drop from 5 workgroups per CU to 2 (one
//   or two waves on a four-SIMD CU).  A 32-key score block is also 8 accumulator registers per lane, not 16, and
//   a chunk K tile is 32 rows x 8 = 256 rotation pairs, not 512.  Per wave the fixed state is 32 registers of O^T
//   (8 x f32x4), 16 of Q fragments, 8 of scores.  The price, 32 accumulator rescales per 32 keys, is taken back
//   where it can be: a wave whose running maxima did not move in a tile (alpha = 1 in every lane: the common
//   case deep in a long cache) skips the rescale, which changes no bit.
//
//   Work split.  Grid (query tiles, Hkv, B); a workgroup's G NS waves are (query head of the group) x (16-query
//   sub-tile), so every K / V tile is staged ONCE for all G heads of its group.  NS = 1 / 2 / 4 for T <= 16 /
//   <= 32 / more, capped at 8 waves: 4 for G <= 2, 2 for G = 3 or 4, 1 for G = 8.  The query tile (up to 64) can
//   be wider than the key tile, so a sub-tile whose queries all lie in front of a chunk tile sits that tile's
//   arithmetic out (it still stages and keeps the barriers); every tile a wave does score holds a visible key for
//   each of its queries.  Only a tile that n or the diagonal cuts pays the per-score compare.  The longest
//   workgroups (last query tiles) launch first.
//
//   One swizzle for 256-byte rows.  A row is one whole 64-bank line of 16 sixteen-byte slots, so a swizzle can
//   only permute slots within the row: chunk c of row r sits at slot c ^ xswz(r), xswz(r) = 2 (r & 7) | (r >> 3 & 1).
//   The K image is read as rows by ds_read_b128 (16 key rows x 4 lane groups, lane group g at chunk 4 kk + g):
//   xswz is a bijection of r & 15, so 16 lanes hit 16 slots, and xswz >> 1 is distinct over 8 rows, so the
//   pairing lanes 0-7 + 16-23 (rows 0-7 at two adjacent chunks) is clean as well.  The V image is read
//   transposed by ds_read_b64_tr_b16 in the accumulator's k order (rows 4 g + q and 16 + 4 g + q, 32 bytes per
//   row): a 32-lane pass is 8 aligned rows x 2 adjacent chunks, clean because xswz >> 1 is distinct over them.
//   So the same function serves both images.  The LDS-DMA lands linearly (16 lanes per row, four rows per 1-KB
//   instruction; the permutation is on the global side, within a row's 256 contiguous bytes), and the plain
//   stores of rotated keys go low-piece-first on even rows and high-piece-first on odd rows, so the two rows of
//   a 16-lane pass hit the two halves of the line.  All four patterns were enumerated on the host.
//
//   Staging.  Cache tiles and the chunk's V tiles come by LDS-DMA (glds16), one tile ahead, 8 one-KB
//   instructions per image dealt round-robin to the waves (short last round with 3 or 6).  Chunk K tiles come
//   through registers: when a tile's DMA is issued a thread loads both halves of its rotation pairs (row,
//   columns 8 c .. and 64 + 8 c ..) and their 8 cos + 8 sin values; after the current tile's arithmetic it rotates
//   them and writes the two pieces into the same swizzled image; the wave waits its own stores out (lgkmcnt)
//   in front of the barrier that publishes the tile, as it does its DMA (vmcnt).  With 32-key tiles a tile is 256
//   pairs: 2 per thread in flight at 128 / 192 threads (48 registers), 1 at 256 / 384.  The 512-thread instances
//   deal 512 HALF-pairs instead (4 columns and their partners, 8-byte pieces, 12 registers in flight): with pairs
//   half their waves would hold nothing and all would pay 24 registers, which their 128-register budget (two
//   workgroups per CU) does not have.  The 64-thread instance (G = 1, T <= 16) would hold 4 pairs = 96 registers:
//   it rotates on arrival instead (loads, rotates and stores after the current tile's arithmetic) -- with
//   T <= 16 it has exactly one chunk tile, so the exposed load is paid once per workgroup.
//
//   Q rotation is lane-local.  In the 16x16x32 B-operand layout a lane's fragment kk holds columns
//   32 kk + 8 g .. + 7 of its query: fragments 0 / 2 and 1 / 3 are rotation pairs.
//
//   Append.  Once per KV head, by the workgroup that owns the chunk positions: 8 pairs per position rotated
//   again with the same function (the same bits as were scored), values as 16-byte copies.
//
// One launch; the grid and the instance follow from B, Hkv, G and T alone; no sync, no atomics, no scratch;
// nothing this launch stores is read by it; bitwise repeatable.  Not here: a non-rotary D = 128 instance.
//
//   Key split (ddl_attn_extend_gqa_d128_split; the SPLIT instances of the same kernel, then a merge launch).  The
//   one launch has ceil(T / TQ) Hkv B workgroups, 8 at B = 1, (32, 8), T = 16, each walking every key tile in turn;
//   the split form folds a split index into blockIdx.z (b nsplit + s) and gives split s the cache tiles of keys
//   [s chunk, min((s + 1) chunk, n)), chunk = ceil(max_len / nsplit) rounded up to the tile, so the grid is static
//   (from max_len) and n = lens[b] is read on the device as before.  A split whose range starts at or past n
//   returns before it stages anything.  The LAST split is the one that also scores the chunk's own tiles (the
//   diagonal) and appends, with the code of the one launch, so the appended bits are its bits.  Last, not first:
//   the first split has a full range of cache keys whenever n >= chunk, and the chunk work on top would make it
//   the longest workgroup of every row; the last split's range is the shortest (what the rounding of chunk
//   leaves) and is empty whenever lens[b] is far below max_len, which is exactly when the other splits finish
//   early too.  It is also the one split that always has a key for every live query (its own), so every live
//   row has at least one partial.  Staging is unchanged: one tile ahead, same swizzle, chunk K through registers.
//   Partials: ws is [B, T, H, nsplit][128] fp32 unnormalised accumulators, stored as 16-byte pieces straight from
//   the MFMA accumulator layout (lane group g owns columns 16 db + 4 g .. + 3 of its query), followed by
//   [B, T, H, nsplit][2] (running maximum in the exp2 domain, sum).  Only queries i < t of live splits are
//   written.  Uninitialised workspace cannot reach the result because the merge DERIVES the live splits instead
//   of reading flags: split s < nsplit - 1 is live iff s chunk < n, the last split always is; it reads those
//   partials and no others, combines them in split order (M = max m_s, w_s = exp2(m_s - M) with a select to 0 at
//   m_s = -inf, out = sum w_s O_s / sum w_s l_s, one rounding to bf16) and writes zero bits to rows i >= t.  No
//   atomics; both launches are bitwise repeatable.  The plan (y_nsplit) is host arithmetic on B, T, H, Hkv and
//   max_len.
//
// Registers.  VGPRs per instance <G, NS>, no scratch in any, 32 KB of LDS each; the launch bounds ask for 4 waves
// per SIMD from the 8-wave instances (two workgroups per CU), 3 from 4 waves up, 2 below:
//   <1,1> 212  <1,2> 240  <1,4> 160  <2,1> 240  <2,2> 160  <2,4> 126  <3,1> 216  <3,2> 160  <4,1> 160  <4,2> 126
//   <8,1> 126
// and the SPLIT instances (scripts/check_spills.py --all-kernels: no scratch in any of the 23 kernels):
//   <1,1> 211  <1,2> 239  <1,4> 161  <2,1> 239  <2,2> 161  <2,4> 126  <3,1> 216  <3,2> 161  <4,1> 161  <4,2> 126
//   <8,1> 126; the merge 26, no LDS.
// So a CU holds two workgroups of the 512-thread instances (<2,4>, <4,2>, <8,1>), of <3,2> and of <3,1>, three of
// the 256-thread ones, four of <2,1> and <1,2>, and of <1,1> the five that 32 KB of LDS allows; the SPLIT
// instances have the occupancy of their one-launch twins.
#include "ddl_lds.h"

#include <algorithm>

namespace {

constexpr int YD = 128;          // head dim
constexpr int YH = YD / 2;       // rotation distance
constexpr int YTK = 32;          // keys per tile
constexpr int YROWB = 256;       // bytes per LDS row (128 bf16): one bank line
constexpr int YIMG = YTK * YROWB;
constexpr int YPAIRS = YTK * 8;  // rotation pairs of a chunk K tile
constexpr float LOG2E = 1.4426950408889634f;

// slot permutation of row r of either image (see the header)
__device__ __forceinline__ int xswz(int r) { return ((r & 7) << 1) | ((r >> 3) & 1); }

__device__ __forceinline__ uint4 ld16(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void st16(bf16_t* p, const uint4& u) { *reinterpret_cast<uint4*>(p) = u; }

// rows row0 .. row0 + 31 of a [rows][ld] bf16 matrix (128 columns used) into a swizzled image; rows >= rows_valid
// (>= 1) are copies of the last valid one.  8 one-KB instructions (4 rows each) dealt round-robin to the NW waves
// (wv wave-uniform); with NW = 3 or 6 the last round is short.
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
            glds16(src + gr * ld + c * 8, dst + q * 1024);     // default policy: every query tile re-reads it
        }
    }
}

// One rotation unit: columns W cw .. + W - 1 and 64 + W cw .. + W - 1 of one head of one token (W = 8: a pair of
// 16-byte pieces; W = 4: half of one, 8-byte pieces), with the W cos and W sin values of its table row.  Loaded in
// one place, rotated in another (a tile later for K tiles).
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
    ldw<W>(head + YH + W * cw, r.b);
    if constexpr (W == 8) {
        load8(tabrow + W * cw, r.c);
        load8(tabrow + YH + W * cw, r.sn);
    } else {
        load4(tabrow + W * cw, r.c);
        load4(tabrow + YH + W * cw, r.sn);
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

// fragment: key rows rbase .. +15 (lane & 15), k = 32 kk + 8 (lane >> 4) + 0..7, from the K image
__device__ __forceinline__ bf16x8 frag_k(const char* img, int rbase, int kk, int lane) {
    const int r = rbase + (lane & 15);
    return *reinterpret_cast<const bf16x8*>(img + r * YROWB + (((kk * 4 + (lane >> 4)) ^ xswz(r)) << 4));
}

// transposed fragment of the V image in the accumulator k order: lane gets column cbase + (lane & 15) of rows
// 16 hh + 4 g + {0..3}, hh = 0, 1
__device__ __forceinline__ bf16x8 frag_vt(const char* img, int cbase, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int chunk = (cbase + 4 * p) >> 3;
    const int ra = 4 * g + q, rb = ra + 16;
    const s16x4 lo = lds_read_tr((lds_v4*)(img + ra * YROWB + ((chunk ^ xswz(ra)) << 4) + (p & 1) * 8));
    const s16x4 hi = lds_read_tr((lds_v4*)(img + rb * YROWB + ((chunk ^ xswz(rb)) << 4) + (p & 1) * 8));
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

// SPLIT: the key-split form (see the header).  blockIdx.z is b nsplit + s; split s walks the cache tiles of keys
// [s chunk, min((s + 1) chunk, n)), the last split also the chunk's own tiles and the append; every split stores
// fp32 partials to ws instead of rows of out.  Without SPLIT the three last arguments are not read.
template <int G, int NS, bool SPLIT>
__global__ __launch_bounds__(64 * G * NS, (G * NS >= 8 ? 4 : (G * NS >= 4 ? 3 : 2))) void attn_extend_d128_k(
    const bf16_t* __restrict__ qkv, const float* __restrict__ tab, bf16_t* __restrict__ kcache,
    bf16_t* __restrict__ vcache, const int* __restrict__ lens, const int* __restrict__ new_lens,
    bf16_t* __restrict__ out, int T, int Hkv, int C, int max_len, float scale, float* __restrict__ ws, int nsplit,
    int chunk) {
    constexpr int NW = G * NS, NT = 64 * NW, TQ = 16 * NS;
    // a chunk K tile is rotated in units of W columns and their partners: 256 pairs (W = 8), or 512 half-pairs
    // (W = 4) in the 512-thread instances, where pairs would leave half the waves idle and cost all of them 24
    // registers; NU units per thread.  The 64-thread instance (NU = 4) rotates on arrival instead of holding 96
    // registers in flight: it serves T <= 16, so it has one chunk tile.
    constexpr int W = NT >= 512 ? 4 : 8, UPR = YH / W, UNITS = YTK * UPR;
    constexpr int NU = (UNITS + NT - 1) / NT;
    constexpr bool ARRIVE = NU > 2;
    __shared__ __attribute__((aligned(16))) char smem[4 * YIMG];   // K0 V0 K1 V1
    const int qt = (int)(gridDim.x - 1 - blockIdx.x), hkv = blockIdx.y;                   // longest loop first
    const int b = SPLIT ? (int)blockIdx.z / nsplit : (int)blockIdx.z, sp = SPLIT ? (int)blockIdx.z % nsplit : 0;
    const bool last = !SPLIT || sp == nsplit - 1;               // the split with the chunk's own keys and the append
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4;
    const int hg = wv / NS, sub = wv % NS;      // this wave's query head of the group and its 16-query sub-tile
    const int H = Hkv * G, h = hkv * G + hg;
    // a lens beyond the host's bound, or a new_lens outside 1 .. T, would index past the cache, the table or the
    // chunk: clamp (the result is then the caller's problem, every access stays in bounds)
    const int n = min(max(lens[b], 0), max_len);
    const int tl = new_lens ? min(max(new_lens[b], 1), T) : T;

    const long HD = (long)H * YD, rs = (long)(H + 2 * Hkv) * YD;
    const bf16_t* rowb = qkv + (long)b * T * rs;
    const bf16_t* qb = rowb + (long)h * YD;
    const bf16_t* kb = rowb + (long)(H + hkv) * YD;
    const bf16_t* vb = rowb + (long)(H + Hkv + hkv) * YD;
    const float* tb = tab + (long)n * YD;                       // the table row of chunk position 0
    bf16_t* ck = kcache + ((long)b * Hkv + hkv) * C * YD;
    bf16_t* cv = vcache + ((long)b * Hkv + hkv) * C * YD;
    const int q0 = qt * TQ, q0w = q0 + 16 * sub, myq = q0w + (lane & 15);
    bf16_t* orow = out + ((long)b * T + myq) * HD + (long)h * YD + 4 * g;

    // this split's cache tiles ct0 .. ct0 + nc - 1 (chunk is a multiple of the tile, so only n cuts a tile)
    const int ct0 = SPLIT ? sp * (chunk / YTK) : 0;
    const int nc = SPLIT ? max(0, (min((sp + 1) * chunk, n) + YTK - 1) / YTK - ct0) : (n + YTK - 1) / YTK;
    if constexpr (SPLIT) {
        // a split past n stages nothing and stores nothing (the merge knows it from lens[b]); rows >= tl are the
        // merge's zeros
        if ((!last && nc == 0) || q0 >= tl) return;
    }
    if (!SPLIT && q0 >= tl) {     // padded queries only: zeros, nothing to append
        if (myq < T) {
#pragma unroll
            for (int db = 0; db < 8; ++db) *reinterpret_cast<uint2*>(orow + 16 * db) = make_uint2(0u, 0u);
        }
        return;
    }

    // append, once per KV head: this workgroup's chunk positions q0 .. q0 + TQ - 1 (those < tl).  The keys: 8
    // pairs per position, rotated once more instead of read back from LDS (the same function, so the same
    // bits); the values: 16-byte bit copies, 16 per position
    if (last) {
#pragma unroll
        for (int i = 0; i < (8 * TQ + NT - 1) / NT; ++i) {
            const int unit = tid + i * NT;
            if ((8 * TQ) % NT == 0 || unit < 8 * TQ) {
                const int j = q0 + (unit >> 3), jc = min(j, tl - 1), c8 = unit & 7;
                const RotIn<8> ri = rot_load<8>(kb + (long)jc * rs, tb + (long)jc * YD, c8);
                uint32_t lo[4], hi[4];
                rot_apply<8>(ri, lo, hi);
                if (j < tl) {
                    stw<8>(ck + (long)(n + j) * YD + 8 * c8, lo);
                    stw<8>(ck + (long)(n + j) * YD + YH + 8 * c8, hi);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < (16 * TQ + NT - 1) / NT; ++i) {
            const int piece = tid + i * NT;
            const int j = q0 + (piece >> 4), s16 = piece & 15;
            if (piece < 16 * TQ && j < tl) st16(cv + (long)(n + j) * YD + s16 * 8, ld16(vb + (long)j * rs + s16 * 8));
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
            const RotIn<8> ri = rot_load<8>(qr, tb + (long)jq * YD, 4 * kk + g);
            uint32_t lo[4], hi[4];
            rot_apply<8>(ri, lo, hi);
            qf[kk] = __builtin_bit_cast(bf16x8, make_uint4(lo[0], lo[1], lo[2], lo[3]));
            qf[kk + 2] = __builtin_bit_cast(bf16x8, make_uint4(hi[0], hi[1], hi[2], hi[3]));
        }
    }

    // chunk tiles, through the workgroup's last diagonal one (none in a split that is not the last)
    const int nd = last ? min(q0 + TQ - 1, tl - 1) / YTK + 1 : 0;
    const int ntot = nc + nd;
    RotIn<W> kin[ARRIVE ? 1 : NU];                               // the next chunk K tile's units, in flight
    // unit -> its chunk row (clamped: a clamped row rotates by its clamped position) and its loads
    auto unit_load = [&](int row0, int unit) __attribute__((always_inline)) {
        const int jc = min(row0 + unit / UPR, tl - 1);
        return rot_load<W>(kb + (long)jc * rs, tb + (long)jc * YD, unit % UPR);
    };
    // issue tile i: DMA for everything but a chunk K tile, whose units go to registers
    auto stage = [&](int i, int buf) __attribute__((always_inline)) {
        char* sK = smem + buf * 2 * YIMG;
        if (i < nc) {
            dma_tile<NW>(ck, YD, (ct0 + i) * YTK, n, sK, wv, lane);
            dma_tile<NW>(cv, YD, (ct0 + i) * YTK, n, sK + YIMG, wv, lane);
        } else {
            const int row0 = (i - nc) * YTK;
            dma_tile<NW>(vb, rs, row0, tl, sK + YIMG, wv, lane);
            if constexpr (!ARRIVE) {
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int unit = tid + u * NT;
                    if (UNITS % NT == 0 || unit < UNITS) kin[u] = unit_load(row0, unit);
                }
            }
        }
    };
    // rotate a chunk K tile's units and write them into the swizzled K image: the low piece first on even rows,
    // the high piece first on odd rows (the rows of one pass of the store then fill the bank line's two halves)
    auto land = [&](int i, int buf) __attribute__((always_inline)) {
        if (i < nc) return;
        char* sK = smem + buf * 2 * YIMG;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int unit = tid + u * NT;
            if (UNITS % NT == 0 || unit < UNITS) {
                const int r = unit / UPR, cw = unit % UPR;
                const bool odd = r & 1;
                uint32_t lo[W / 2], hi[W / 2], first[W / 2], second[W / 2];
                if constexpr (ARRIVE) rot_apply<W>(unit_load((i - nc) * YTK, unit), lo, hi);
                else rot_apply<W>(kin[u], lo, hi);
#pragma unroll
                for (int e = 0; e < W / 2; ++e) {
                    first[e] = odd ? hi[e] : lo[e];
                    second[e] = odd ? lo[e] : hi[e];
                }
                // columns W cw ..: chunk W cw / 8 (+ 8 for the high piece), byte 2 W cw & 15 within it
                char* rowp = sK + r * YROWB + ((2 * W * cw) & 15);
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

    stage(0, 0);
    land(0, 0);
    for (int i = 0; i < ntot; ++i) {
        // tile i has landed (this wave's LDS stores and DMA, then everyone's); everyone is done with the other
        // image pair
        LGKM0();
        VMN(0);
        BARRIER();
        // (none after the last tile: LDS-DMA must not be landing when the workgroup exits)
        if (i + 1 < ntot) stage(i + 1, (i + 1) & 1);
        const bool cache = i < nc;
        const int key0 = (cache ? ct0 + i : i - nc) * YTK;
        // a chunk tile that starts past this wave's last query holds nothing for it (key0 and q0w are multiples
        // of 16, so key0 <= q0w + 15 is key0 <= q0w: every query of a scoring wave sees key key0)
        if (active && (cache || key0 <= q0w)) {
            const char* sK = smem + (i & 1) * 2 * YIMG;
            const char* sV = sK + YIMG;
            // keys key0 + j of this part are visible to this lane's query while key0 + j < limit
            const int limit = cache ? n : myq + 1;
            const bool cut = cache ? key0 + YTK > n : key0 + YTK - 1 > q0w;     // per wave
            // ---- S^T block: lane holds s[blk][r] = score(q = myq, key = key0 + 16 blk + 4 g + r)
            f32x4 s[2];
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                s[blk] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    s[blk] =
                        __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_k(sK, 16 * blk, kk, lane), qf[kk], s[blk], 0, 0, 0);
            }
            float tmax = -INFINITY;
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const int k0 = key0 + 16 * blk + 4 * g;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = s[blk][r] * c2;
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
            for (int blk = 0; blk < 2; ++blk) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(s[blk][r] - mnew);
                    psum += pv;
                    s[blk][r] = pv;
                }
            }
            lsum = lsum * alpha + psum;
            // (wave-uniform: no lane's maximum moved, every alpha is exactly 1)
            if (__builtin_amdgcn_ballot_w64(alpha != 1.f)) {
#pragma unroll
                for (int db = 0; db < 8; ++db) o[db] *= alpha;
            }
            // ---- O^T[d][q] += V^T[d][k] P^T[k][q]: one 32-deep step per 16-column block
            const bf16x8 pf = pack_p(s[0], s[1]);
#pragma unroll
            for (int db = 0; db < 8; ++db)
                o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_vt(sV, 16 * db, lane), pf, o[db], 0, 0, 0);
        }
        if (i + 1 < ntot) land(i + 1, (i + 1) & 1);
    }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    if constexpr (SPLIT) {
        // the partial of (b, myq, h, sp), straight from the accumulator layout: lane group g holds columns
        // 16 db + 4 g .. + 3.  ws is [rows][128] accumulators, then [rows][2] (maximum, sum), rows = B T H nsplit.
        // Every query < tl of a split that gets here has scored a key (a cache tile of its range, or its diagonal)
        if (myq >= tl) return;
        const long row = (((long)b * T + myq) * H + h) * nsplit + sp;
        float* po = ws + row * YD + 4 * g;
#pragma unroll
        for (int db = 0; db < 8; ++db) *reinterpret_cast<f32x4*>(po + 16 * db) = o[db];
        if (g == 0) *reinterpret_cast<float2*>(ws + (long)gridDim.z * T * H * YD + row * 2) = make_float2(m, lsum);
        return;
    }
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

// The merge of a split launch: 32 threads per (b, query i, head h), 4 columns each, 8 rows per workgroup.  The live
// splits of a row follow from lens[b] and chunk (cache splits 0 .. ceil(n / chunk) - 1 below the last, and the
// last); they are combined in split order, nothing else of ws is read.  Rows i >= t are zero bits.
__global__ __launch_bounds__(256) void attn_extend_d128_merge_k(const float* __restrict__ ws,
                                                                const int* __restrict__ lens,
                                                                const int* __restrict__ new_lens,
                                                                bf16_t* __restrict__ out, long rows, int T, int H,
                                                                int nsplit, int chunk, int max_len) {
    const long row = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (row >= rows) return;
    const int c = threadIdx.x & 31, b = (int)(row / ((long)T * H)), i = (int)(row / H % T);
    const int n = min(max(lens[b], 0), max_len);
    const int tl = new_lens ? min(max(new_lens[b], 1), T) : T;
    bf16_t* po = out + row * YD + 4 * c;
    if (i >= tl) {
        *reinterpret_cast<uint2*>(po) = make_uint2(0u, 0u);
        return;
    }
    const int nlive = min(nsplit - 1, (n + chunk - 1) / chunk);
    const float2* ml = reinterpret_cast<const float2*>(ws + rows * nsplit * YD) + row * nsplit;
    const float* acc = ws + row * nsplit * YD + 4 * c;
    float M = ml[nsplit - 1].x;
    for (int s = 0; s < nlive; ++s) M = fmaxf(M, ml[s].x);
    float l = 0.f, o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < nsplit; ++s) {
        if (s >= nlive && s != nsplit - 1) continue;
        const float2 p = ml[s];
        const float w = p.x == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(p.x - M);    // (never -inf - -inf)
        float v[4];
        load4(acc + (long)s * YD, v);
        l += w * p.y;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] += w * v[k];
    }
    const float inv = 1.f / l;
    const float r[4] = {o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv};
    store4(po, r);
}

inline bool y_group_ok(int H, int Hkv) {
    if (Hkv < 1 || H < Hkv || H % Hkv) return false;
    const int G = H / Hkv;
    return G == 1 || G == 2 || G == 3 || G == 4 || G == 8;
}

// 16-query sub-tiles per workgroup for a chunk of T tokens and a group of G heads: 1 / 2 / 4, capped so that
// G NS <= 8 waves
inline int y_subtiles(int T, int G) {
    const int want = T <= 16 ? 1 : (T <= 32 ? 2 : 4);
    const int cap = G >= 8 ? 1 : (G >= 3 ? 2 : 4);
    return std::min(want, cap);
}

// Keys per split of a launch of nsplit splits over a bound of max_len keys: a multiple of the key tile
inline int y_chunk(int max_len, int nsplit) {
    const int per = (std::max(max_len, 1) + nsplit - 1) / nsplit;
    return (per + YTK - 1) / YTK * YTK;
}

// The plan: key splits of the launch, from the shapes and max_len alone.  Enough splits that there are two
// workgroups per CU, at most Y_MAX_SPLIT, each of at least Y_MIN_KEYS keys (7 tiles; so max_len below 448 is
// always the one launch).  The two per CU, the cap (the largest value tried) and the minimum are read off the
// sweep in profiles/llama_d128_extend_split.log
constexpr int Y_MAX_SPLIT = 32, Y_MIN_KEYS = 224;
inline int y_nsplit(int B, int T, int H, int Hkv, int max_len) {
    if (!y_group_ok(H, Hkv) || B < 1 || T < 1) return 1;
    const int tq = 16 * y_subtiles(T, H / Hkv);
    const long wgs = (long)((T + tq - 1) / tq) * Hkv * B;
    const long want = std::min<long>({Y_MAX_SPLIT, (2 * num_cus() + wgs - 1) / wgs, max_len / Y_MIN_KEYS});
    if (want < 2) return 1;
    const int chunk = y_chunk(max_len, (int)want);
    return std::max(1, (max_len + chunk - 1) / chunk);          // (no split that max_len leaves empty)
}

}  // namespace

// 1 when the head-dim-128 rotary extend kernel has an instance for this group size
DDL_API int ddl_attn_extend_gqa_d128_supported(int H, int Hkv) { return y_group_ok(H, Hkv) ? 1 : 0; }
// queries per workgroup for this (T, H, Hkv): what the launch will use (0 without an instance)
DDL_API int ddl_attn_extend_gqa_d128_tile(int T, int H, int Hkv) {
    return y_group_ok(H, Hkv) ? 16 * y_subtiles(T, H / Hkv) : 0;
}

DDL_API int ddl_attn_extend_gqa_d128(const void* qkv_new, const float* tab, void* kcache, void* vcache,
                                     const void* lens, const void* new_lens, void* out, int B, int T, int H, int Hkv,
                                     int C, int max_len, long n_pos, float scale, hipStream_t st) {
    if (!y_group_ok(H, Hkv)) return (int)hipErrorInvalidValue;
    if (B <= 0 || T <= 0) return 0;
    if (max_len < 0 || (long)max_len + T > C || (long)max_len + T > n_pos || Hkv > 65535 || B > 65535)
        return (int)hipErrorInvalidValue;
    const int G = H / Hkv;
#define Y_LAUNCH(G_, NS_)                                                                                              \
    attn_extend_d128_k<G_, NS_, false><<<dim3((T + 16 * NS_ - 1) / (16 * NS_), Hkv, B), 64 * G_ * NS_, 0, st>>>(       \
        (const bf16_t*)qkv_new, tab, (bf16_t*)kcache, (bf16_t*)vcache, (const int*)lens, (const int*)new_lens,         \
        (bf16_t*)out, T, Hkv, C, max_len, scale, nullptr, 1, 0)
    switch (G * 8 + y_subtiles(T, G)) {
        case 1 * 8 + 1: Y_LAUNCH(1, 1); break;
        case 1 * 8 + 2: Y_LAUNCH(1, 2); break;
        case 1 * 8 + 4: Y_LAUNCH(1, 4); break;
        case 2 * 8 + 1: Y_LAUNCH(2, 1); break;
        case 2 * 8 + 2: Y_LAUNCH(2, 2); break;
        case 2 * 8 + 4: Y_LAUNCH(2, 4); break;
        case 3 * 8 + 1: Y_LAUNCH(3, 1); break;
        case 3 * 8 + 2: Y_LAUNCH(3, 2); break;
        case 4 * 8 + 1: Y_LAUNCH(4, 1); break;
        case 4 * 8 + 2: Y_LAUNCH(4, 2); break;
        case 8 * 8 + 1: Y_LAUNCH(8, 1); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef Y_LAUNCH
    DDL_RETURN_LAUNCH();
}

// key splits the plan gives this shape (1: the one launch above)
DDL_API int ddl_attn_extend_gqa_d128_nsplit(int B, int T, int H, int Hkv, int max_len) {
    return y_nsplit(B, T, H, Hkv, max_len);
}
// floats of workspace a launch of nsplit splits needs
DDL_API long ddl_attn_extend_gqa_d128_ws(int B, int T, int H, int nsplit) {
    return (long)B * T * H * nsplit * (2 + YD);
}

// The key-split form: nsplit >= 2 splits of y_chunk(max_len, nsplit) keys, then the merge; ws holds
// ddl_attn_extend_gqa_d128_ws(B, T, H, nsplit) floats and need not be initialised.
DDL_API int ddl_attn_extend_gqa_d128_split(const void* qkv_new, const float* tab, void* kcache, void* vcache,
                                           const void* lens, const void* new_lens, void* out, void* ws, int nsplit,
                                           int B, int T, int H, int Hkv, int C, int max_len, long n_pos, float scale,
                                           hipStream_t st) {
    if (!y_group_ok(H, Hkv)) return (int)hipErrorInvalidValue;
    if (B <= 0 || T <= 0) return 0;
    if (max_len < 0 || (long)max_len + T > C || (long)max_len + T > n_pos || Hkv > 65535 || nsplit < 2 || !ws ||
        (long)B * nsplit > 65535)
        return (int)hipErrorInvalidValue;
    const int G = H / Hkv, chunk = y_chunk(max_len, nsplit);
#define Y_LAUNCH(G_, NS_)                                                                                              \
    attn_extend_d128_k<G_, NS_, true><<<dim3((T + 16 * NS_ - 1) / (16 * NS_), Hkv, B * nsplit), 64 * G_ * NS_, 0,      \
                                        st>>>((const bf16_t*)qkv_new, tab, (bf16_t*)kcache, (bf16_t*)vcache,           \
                                              (const int*)lens, (const int*)new_lens, (bf16_t*)out, T, Hkv, C,         \
                                              max_len, scale, (float*)ws, nsplit, chunk)
    switch (G * 8 + y_subtiles(T, G)) {
        case 1 * 8 + 1: Y_LAUNCH(1, 1); break;
        case 1 * 8 + 2: Y_LAUNCH(1, 2); break;
        case 1 * 8 + 4: Y_LAUNCH(1, 4); break;
        case 2 * 8 + 1: Y_LAUNCH(2, 1); break;
        case 2 * 8 + 2: Y_LAUNCH(2, 2); break;
        case 2 * 8 + 4: Y_LAUNCH(2, 4); break;
        case 3 * 8 + 1: Y_LAUNCH(3, 1); break;
        case 3 * 8 + 2: Y_LAUNCH(3, 2); break;
        case 4 * 8 + 1: Y_LAUNCH(4, 1); break;
        case 4 * 8 + 2: Y_LAUNCH(4, 2); break;
        case 8 * 8 + 1: Y_LAUNCH(8, 1); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef Y_LAUNCH
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    const long rows = (long)B * T * H;
    attn_extend_d128_merge_k<<<(unsigned)((rows + 7) / 8), 256, 0, st>>>(
        (const float*)ws, (const int*)lens, (const int*)new_lens, (bf16_t*)out, rows, T, H, nsplit, chunk, max_len);
    DDL_RETURN_LAUNCH();
}
