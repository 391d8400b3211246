// Chunk (extend) attention for grouped queries over a ROTATED key/value cache: T new tokens per sequence
// are rotated, attend to the cached keys and, causally, to the chunk's own rotated keys, and the chunk's
// rotated keys / values are appended.  Forward only, head dim 64, bf16, G = H / Hkv in {1, 2, 3, 4, 8}.
// ONE launch, no scratch buffer: the rotation of the chunk's queries and keys happens inside it.
//
// Inputs: qkv_new [B, T, (H + 2 Hkv) 64], the chunk's fused UNROTATED projection [q heads | k heads | v
// heads]; tab [n_pos, 64], the fp32 rotary table (row s = [cos 0..31 | sin 0..31]); kcache / vcache
// [B, Hkv, C, 64]; lens [B] int32 and the optional new_lens [B] int32 on the device.  For batch row b with
// n = lens[b] (clamped to 0 .. max_len) and t = new_lens[b] (clamped to 1 .. T; T without new_lens), chunk
// token i < t has its H query heads and Hkv key heads rotated by table row n + i (HF half-split pairs
// i / i+32 in fp32, the expressions and operand order of llama.hip's rope_qkv_fwd_k, rounded ONCE to bf16:
// the bits rope_qkv hands a full forward).  Query i of head h attends to cached keys 0 .. n-1 of KV head
// h / G and to rotated chunk keys 0 .. i of that head; out [B, T, H 64] rows i >= t are zeros.  The rotated
// key and the value (a bit copy) of chunk positions i < t are stored to cache[b, :, n + i]; lens and
// new_lens are not written.  No cache row >= n and no table row past max_len + T - 1 is loaded.
//
// The structure is attn_extend.hip's: S^T = K Q^T on v_mfma_f32_16x16x32_bf16, P fed from the accumulators
// into O^T += V^T P^T, fp32 online softmax on exp2, 64-key tiles one ahead in two swizzled [64][64] image
// pairs, the compare only on a tile that n or the diagonal cuts, clamped copies plus selects for rows past
// the end of a part, the longest workgroups first, a grid that follows from B, Hkv, T and G alone, no
// atomics, no sync, the same bits on every run.  What differs:
//   - the grid is (query tiles, Hkv, B).  A workgroup's G NS waves are (query head of the group) x
//     (16-query sub-tile): every K / V tile is staged ONCE and scored by all G heads of its group, so a
//     call reads the cache bytes of Hkv heads, not of H.  NS (1 / 2 / 4 sub-tiles for T <= 16 / <= 32 /
//     more) is capped so that a workgroup has at most 8 waves: 4 for G <= 2, 2 for G = 3 or 4, 1 for G = 8;
//   - a lane's Q fragments hold columns 8g .. and 32 + 8g .. of its query, a rotation pair: the Q rotation
//     is lane-local, with 8 cos and 8 sin values of table row n + myq;
//   - cache tiles and the chunk's V tiles arrive by LDS-DMA.  The chunk's K tiles cannot (they are not
//     rotated in memory): a thread loads both halves of a (row, 8-column) pair and its 16 table values a
//     tile ahead, when the DMA of that tile is issued, and after the current tile's arithmetic rotates
//     them and writes the two 16-byte pieces into the same swizzled image with plain LDS stores.  Those
//     stores are waited for (lgkmcnt) by the wave that made them in front of the barrier that publishes
//     the tile, as the DMA is (vmcnt); the image they go to was last read before the previous barrier;
//   - the append rotates the workgroup's own chunk keys once more (one pair per thread of the first NS
//     waves) instead of reading them back from LDS: the same function, so the same bits.
#include "ddl_lds.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int YD = 64;           // head dim
constexpr int YTK = 64;          // keys per tile
constexpr int YROWB = 128;       // bytes per LDS row (64 bf16)
constexpr int YIMG = YTK * YROWB;
constexpr float LOG2E = 1.4426950408889634f;

// chunk swizzles of the two images (attn_extend.hip's): K is read as rows (ds_read_b128), V transposed
__device__ __forceinline__ int yswz_k(int r, int c) { return c ^ ((r >> 1) & 7); }
__device__ __forceinline__ int yswz_v(int r, int c) { return c ^ (2 * ((r >> 1) & 3)); }

__device__ __forceinline__ void unpack8(const uint4& u, float* v) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = lo_f(w[i]);
        v[2 * i + 1] = hi_f(w[i]);
    }
}
__device__ __forceinline__ uint4 pack8(const float* v) {
    return make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
}
__device__ __forceinline__ uint4 ld16(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void st16(bf16_t* p, const uint4& u) { *reinterpret_cast<uint4*>(p) = u; }

// rows row0 .. row0 + 63 of a [rows][ld] bf16 matrix (64 columns used) into a swizzled image; rows
// >= rows_valid (>= 1) are copies of the last valid one.  8 one-KB instructions dealt round-robin to the
// NW waves (wv wave-uniform); with NW = 3 or 6 the last round is short.
template <int NW, bool V>
__device__ __forceinline__ void dma_tile(const bf16_t* src, long ld, int row0, int rows_valid, char* dst, int wv,
                                         int lane) {
#pragma unroll
    for (int qq = 0; qq < (8 + NW - 1) / NW; ++qq) {
        const int q = qq * NW + wv;
        if (8 % NW == 0 || q < 8) {
            const int r = q * 8 + (lane >> 3), cl = lane & 7;
            const int c = V ? yswz_v(r, cl) : yswz_k(r, cl);
            const long gr = min(row0 + r, rows_valid - 1);
            glds16(src + gr * ld + c * 8, dst + q * 1024);     // default policy: every query tile re-reads it
        }
    }
}

// One rotation pair: columns 8 c4 .. + 7 and 32 + 8 c4 .. + 7 of one head of one token, with the 8 cos
// and 8 sin values of its table row.  Loaded in one place, rotated in another (a tile later for K tiles).
struct RotIn {
    uint4 a, b;
    float c[8], sn[8];
};
__device__ __forceinline__ RotIn rot_load(const bf16_t* head, const float* tabrow, int c4) {
    RotIn r;
    r.a = ld16(head + 8 * c4);
    r.b = ld16(head + 32 + 8 * c4);
    load8(tabrow + 8 * c4, r.c);
    load8(tabrow + 32 + 8 * c4, r.sn);
    return r;
}
// rope_qkv_fwd_k's expressions, operand order included; each half rounded once
__device__ __forceinline__ void rot_apply(const RotIn& r, uint4& lo, uint4& hi) {
    float x1[8], x2[8], o1[8], o2[8];
    unpack8(r.a, x1);
    unpack8(r.b, x2);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o1[e] = x1[e] * r.c[e] - x2[e] * r.sn[e];
        o2[e] = x2[e] * r.c[e] + x1[e] * r.sn[e];
    }
    lo = pack8(o1);
    hi = pack8(o2);
}

// fragment: key rows rbase .. +15 (lane & 15), k = 32 kk + 8 (lane >> 4) + 0..7, from the K image
__device__ __forceinline__ bf16x8 frag_k(const char* img, int rbase, int kk, int lane) {
    const int r = rbase + (lane & 15);
    return *reinterpret_cast<const bf16x8*>(img + r * YROWB + (yswz_k(r, kk * 4 + (lane >> 4)) << 4));
}

// transposed fragment of the V image in the accumulator k order: lane gets column cbase + (lane & 15)
// of rows kb + 16 hh + 4 g + {0..3}, hh = 0, 1
__device__ __forceinline__ bf16x8 frag_vt(const char* img, int kb, int cbase, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int col = cbase + 4 * p;
    const int ra = kb + 4 * g + q, rb = ra + 16;
    const s16x4 lo = lds_read_tr((lds_v4*)(img + ra * YROWB + (yswz_v(ra, col >> 3) << 4) + (p & 1) * 8));
    const s16x4 hi = lds_read_tr((lds_v4*)(img + rb * YROWB + (yswz_v(rb, col >> 3) << 4) + (p & 1) * 8));
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

template <int G, int NS>
__global__ __launch_bounds__(64 * G * NS) void attn_extend_gqa_k(
    const bf16_t* __restrict__ qkv, const float* __restrict__ tab, bf16_t* __restrict__ kcache,
    bf16_t* __restrict__ vcache, const int* __restrict__ lens, const int* __restrict__ new_lens,
    bf16_t* __restrict__ out, int T, int Hkv, int C, int max_len, float scale) {
    constexpr int NW = G * NS, NT = 64 * NW, TQ = 16 * NS;
    constexpr int NU = (256 + NT - 1) / NT;     // rotation pairs of a K tile (64 rows x 4) per thread
    __shared__ __attribute__((aligned(16))) char smem[4 * YIMG];   // K0 V0 K1 V1
    const int qt = (int)(gridDim.x - 1 - blockIdx.x), hkv = blockIdx.y, b = blockIdx.z;   // longest loop first
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4;
    const int hg = wv / NS, sub = wv % NS;      // this wave's query head of the group, its 16-query sub-tile
    const int H = Hkv * G, h = hkv * G + hg;
    // a lens beyond the host's bound, or a new_lens outside 1 .. T, would index past the cache, the table
    // or the chunk: clamp (the result is then the caller's problem, every access stays in bounds)
    const int n = min(max(lens[b], 0), max_len);
    const int tl = new_lens ? min(max(new_lens[b], 1), T) : T;

    const long HD = (long)H * YD, rs = (long)(H + 2 * Hkv) * YD;
    const bf16_t* rowb = qkv + (long)b * T * rs;
    const bf16_t* qb = rowb + (long)h * YD;
    const bf16_t* kb = rowb + (long)(H + hkv) * YD;
    const bf16_t* vb = rowb + (long)(H + Hkv + hkv) * YD;
    const float* tb = tab + (long)n * YD;       // the table row of chunk position 0
    bf16_t* ck = kcache + ((long)b * Hkv + hkv) * C * YD;
    bf16_t* cv = vcache + ((long)b * Hkv + hkv) * C * YD;
    const int q0 = qt * TQ, q0w = q0 + 16 * sub, myq = q0w + (lane & 15);
    bf16_t* orow = out + ((long)b * T + myq) * HD + (long)h * YD + 4 * g;

    if (q0 >= tl) {     // padded queries only: zeros, nothing to append
        if (myq < T) {
#pragma unroll
            for (int db = 0; db < 4; ++db) *reinterpret_cast<uint2*>(orow + 16 * db) = make_uint2(0u, 0u);
        }
        return;
    }

    // append, once per KV head: this workgroup's chunk positions q0 .. q0 + TQ - 1 (those < tl).  The
    // rotated keys: one pair per thread of the first NS waves; the values: 16-byte bit copies.
    if (tid < 4 * TQ) {
        const int j = q0 + (tid >> 2), jc = min(j, tl - 1), c4 = tid & 3;
        const RotIn ri = rot_load(kb + (long)jc * rs, tb + (long)jc * YD, c4);
        uint4 lo, hi;
        rot_apply(ri, lo, hi);
        if (j < tl) {
            st16(ck + (long)(n + j) * YD + 8 * c4, lo);
            st16(ck + (long)(n + j) * YD + 32 + 8 * c4, hi);
        }
    }
#pragma unroll
    for (int i = 0; i < (8 * TQ + NT - 1) / NT; ++i) {
        const int piece = tid + i * NT;
        const int j = q0 + (piece >> 3), s8 = piece & 7;
        if (piece < 8 * TQ && j < tl) st16(cv + (long)(n + j) * YD + s8 * 8, ld16(vb + (long)j * rs + s8 * 8));
    }

    // Q fragments (B operand of S^T = K Q^T): lane holds the rotated Q[myq][32 kk + 8 g + 0..7]
    bf16x8 qf[2];
    {
        const int jq = min(myq, tl - 1);
        const RotIn ri = rot_load(qb + (long)jq * rs, tb + (long)jq * YD, g);
        uint4 lo, hi;
        rot_apply(ri, lo, hi);
        qf[0] = __builtin_bit_cast(bf16x8, lo);
        qf[1] = __builtin_bit_cast(bf16x8, hi);
    }

    const int nc = (n + YTK - 1) / YTK;                         // cache tiles
    const int nd = min(q0 + TQ - 1, tl - 1) / YTK + 1;           // chunk tiles, through the diagonal one
    const int ntot = nc + nd;
    RotIn kin[NU];                                               // the next chunk K tile's pairs, in flight
    // issue tile i: DMA for everything but a chunk K tile, whose pairs go to registers
    auto stage = [&](int i, int buf) __attribute__((always_inline)) {
        char* sK = smem + buf * 2 * YIMG;
        if (i < nc) {
            dma_tile<NW, false>(ck, YD, i * YTK, n, sK, wv, lane);
            dma_tile<NW, true>(cv, YD, i * YTK, n, sK + YIMG, wv, lane);
        } else {
            const int row0 = (i - nc) * YTK;
            dma_tile<NW, true>(vb, rs, row0, tl, sK + YIMG, wv, lane);
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int unit = tid + u * NT;
                if (256 % NT == 0 || unit < 256) {
                    const int jc = min(row0 + (unit >> 2), tl - 1);  // a clamped row rotates by its clamped position
                    kin[u] = rot_load(kb + (long)jc * rs, tb + (long)jc * YD, unit & 3);
                }
            }
        }
    };
    // rotate a chunk K tile's pairs and write them into the swizzled K image
    auto land = [&](int i, int buf) __attribute__((always_inline)) {
        if (i < nc) return;
        char* sK = smem + buf * 2 * YIMG;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int unit = tid + u * NT;
            if (256 % NT == 0 || unit < 256) {
                const int r = unit >> 2, c4 = unit & 3;
                uint4 lo, hi;
                rot_apply(kin[u], lo, hi);
                *reinterpret_cast<uint4*>(sK + r * YROWB + (yswz_k(r, c4) << 4)) = lo;
                *reinterpret_cast<uint4*>(sK + r * YROWB + (yswz_k(r, c4 + 4) << 4)) = hi;
            }
        }
    };

    const float c2 = scale * LOG2E;                              // scores in the exp2 domain
    const bool active = q0w < tl;                                // per wave: it has a valid query
    float m = -INFINITY, lsum = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    stage(0, 0);
    land(0, 0);
    for (int i = 0; i < ntot; ++i) {
        // tile i has landed (this wave's LDS stores and DMA, then everyone's); everyone is done with the
        // other image pair
        LGKM0();
        VMN(0);
        BARRIER();
        // (none after the last tile: LDS-DMA must not be landing when the workgroup exits)
        if (i + 1 < ntot) stage(i + 1, (i + 1) & 1);
        if (active) {
            const char* sK = smem + (i & 1) * 2 * YIMG;
            const char* sV = sK + YIMG;
            // keys key0 + j of this part are visible to this lane's query while key0 + j < limit
            const bool cache = i < nc;
            const int key0 = (cache ? i : i - nc) * YTK;
            const int limit = cache ? n : myq + 1;
            const bool cut = cache ? key0 + YTK > n : key0 + YTK - 1 > q0w;     // per wave
            // ---- S^T block: lane holds s[blk][r] = score(q = myq, key = key0 + 16 blk + 4 g + r)
            f32x4 s[4];
#pragma unroll
            for (int blk = 0; blk < 4; ++blk) {
                s[blk] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
                    s[blk] =
                        __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_k(sK, 16 * blk, kk, lane), qf[kk], s[blk], 0, 0, 0);
            }
            float tmax = -INFINITY;
#pragma unroll
            for (int blk = 0; blk < 4; ++blk) {
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
            // (every tile holds a visible key for every query: key 64 (nc - 1) < n, chunk key key0 <= q0)
            const float mnew = fmaxf(m, tmax);
            const float alpha = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - mnew);
            m = mnew;
            float psum = 0.f;
#pragma unroll
            for (int blk = 0; blk < 4; ++blk) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(s[blk][r] - mnew);
                    psum += pv;
                    s[blk][r] = pv;
                }
            }
            lsum = lsum * alpha + psum;
#pragma unroll
            for (int db = 0; db < 4; ++db) o[db] *= alpha;
            // ---- O^T[d][q] += V^T[d][k] P^T[k][q]
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const bf16x8 pf = pack_p(s[2 * st], s[2 * st + 1]);
#pragma unroll
                for (int db = 0; db < 4; ++db)
                    o[db] =
                        __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_vt(sV, 32 * st, 16 * db, lane), pf, o[db], 0, 0, 0);
            }
        }
        if (i + 1 < ntot) land(i + 1, (i + 1) & 1);
    }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    if (myq >= T) return;
    const bool qok = myq < tl;                                   // (then lsum >= 1: its own key)
    const float inv = qok ? 1.f / lsum : 0.f;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
        const float v[4] = {qok ? o[db][0] * inv : 0.f, qok ? o[db][1] * inv : 0.f, qok ? o[db][2] * inv : 0.f,
                            qok ? o[db][3] * inv : 0.f};
        store4(orow + 16 * db, v);
    }
}

inline bool xg_group_ok(int H, int Hkv) {
    if (Hkv < 1 || H < Hkv || H % Hkv) return false;
    const int G = H / Hkv;
    return G == 1 || G == 2 || G == 3 || G == 4 || G == 8;
}

// 16-query sub-tiles per workgroup for a chunk of T tokens and a group of G heads: attn_extend.hip's
// 1 / 2 / 4, capped so that G NS <= 8 waves
inline int xg_subtiles(int T, int G) {
    const int want = T <= 16 ? 1 : (T <= 32 ? 2 : 4);
    const int cap = G >= 8 ? 1 : (G >= 3 ? 2 : 4);
    return std::min(want, cap);
}

}  // namespace

// 1 when the extend kernel has an instance for this group size (the decode kernel's set)
DDL_API int ddl_attn_extend_gqa_supported(int H, int Hkv) { return xg_group_ok(H, Hkv) ? 1 : 0; }
// queries per workgroup for this (T, H, Hkv): what the launch will use (0 without an instance)
DDL_API int ddl_attn_extend_gqa_tile(int T, int H, int Hkv) {
    return xg_group_ok(H, Hkv) ? 16 * xg_subtiles(T, H / Hkv) : 0;
}

DDL_API int ddl_attn_extend_gqa(const void* qkv_new, const float* tab, void* kcache, void* vcache, const void* lens,
                                const void* new_lens, void* out, int B, int T, int H, int Hkv, int C, int max_len,
                                long n_pos, float scale, hipStream_t st) {
    if (!xg_group_ok(H, Hkv)) return (int)hipErrorInvalidValue;
    if (B <= 0 || T <= 0) return 0;
    if (max_len < 0 || (long)max_len + T > C || (long)max_len + T > n_pos || Hkv > 65535 || B > 65535)
        return (int)hipErrorInvalidValue;
    const int G = H / Hkv, ns = xg_subtiles(T, G);
    const dim3 grid((T + 16 * ns - 1) / (16 * ns), Hkv, B);
#define XG_LAUNCH(G_, NS_)                                                                                             \
    attn_extend_gqa_k<G_, NS_><<<grid, 64 * G_ * NS_, 0, st>>>(                                                        \
        (const bf16_t*)qkv_new, tab, (bf16_t*)kcache, (bf16_t*)vcache, (const int*)lens, (const int*)new_lens,         \
        (bf16_t*)out, T, Hkv, C, max_len, scale)
    switch (G * 8 + ns) {
        case 1 * 8 + 1: XG_LAUNCH(1, 1); break;
        case 1 * 8 + 2: XG_LAUNCH(1, 2); break;
        case 1 * 8 + 4: XG_LAUNCH(1, 4); break;
        case 2 * 8 + 1: XG_LAUNCH(2, 1); break;
        case 2 * 8 + 2: XG_LAUNCH(2, 2); break;
        case 2 * 8 + 4: XG_LAUNCH(2, 4); break;
        case 3 * 8 + 1: XG_LAUNCH(3, 1); break;
        case 3 * 8 + 2: XG_LAUNCH(3, 2); break;
        case 4 * 8 + 1: XG_LAUNCH(4, 1); break;
        case 4 * 8 + 2: XG_LAUNCH(4, 2); break;
        case 8 * 8 + 1: XG_LAUNCH(8, 1); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef XG_LAUNCH
    DDL_RETURN_LAUNCH();
}
