// Chunk (extend) attention over a key/value cache: T new tokens per sequence attend to the cached keys and,
// causally, to the chunk's own keys; the chunk's keys / values are appended.  For the rotary (Llama) family the
// chunk's queries and keys are rotated inside the same launch.  Forward only, head dim 64, bf16.
//
// Inputs: qkv_new [B, T, (H + 2 Hkv) 64], the chunk's fused projection [q heads | k heads | v heads] (G = H / Hkv
// query heads share a KV head); kcache / vcache [B, Hkv, C, 64]; lens [B] int32 and the optional new_lens [B]
// int32 on the device.  For batch row b with n = lens[b] (clamped to 0 .. max_len) and t = new_lens[b] (clamped
// to 1 .. T; T without new_lens), query i < t of head h attends to cached keys 0 .. n-1 of KV head h / G and to
// chunk keys 0 .. i of that head; out [B, T, H 64] rows i >= t are zeros.  The K / V rows of chunk positions
// i < t are stored to cache[b, :, n + i]; lens and new_lens are not written (all layers share them).
//
// One kernel, attn_extend_k<G, NS, ROPE>, serves both families:
//   - ROPE = false (GPT-2: ddl_attn_extend, G = 1): the packed [B, T, 3 H 64] projection is the layout above
//     with Hkv = H; queries and keys are used as they are, and no table is read.
//   - ROPE = true (ddl_attn_extend_gqa, G in {1, 2, 3, 4, 8}): the cache holds ROTATED keys and qkv_new is
//     UNROTATED.  tab [n_pos, 64] is the fp32 rotary table (row s = [cos 0..31 | sin 0..31]); chunk token i < t
//     has its query and key heads rotated by table row n + i (HF half-split pairs i / i+32 in fp32, the
//     expressions and operand order of llama.hip's rope_qkv_fwd_k, rounded ONCE to bf16: the bits rope_qkv
//     hands a full forward), and the rotated key is what is appended.  The value is a bit copy.  No table row
//     past max_len + T - 1 is loaded.
//
// The grid is (query tiles, Hkv, B).  A workgroup's G NS waves are (query head of the group) x (16-query
// sub-tile): every K / V tile is staged ONCE and scored by all G heads of its group, so a call reads the cache
// bytes of Hkv heads, not of H.  NS (1 / 2 / 4 sub-tiles for T <= 16 / <= 32 / more) is capped so that a
// workgroup has at most 8 waves: 4 for G <= 2, 2 for G = 3 or 4, 1 for G = 8.  A wave works as attention.hip's
// forward does: S^T = K Q^T on v_mfma_f32_16x16x32_bf16 (query on the lane, a 64-key tile's scores in the
// accumulators), fp32 online softmax on exp2, P rounded to bf16 and fed from the accumulator registers as the B
// operand of O^T += V^T P^T.  The key loop runs over ceil(n / 64) cache tiles (the bound a scalar read of lens)
// and then over the chunk tiles up to the one that holds the workgroup's last query.  Only a tile that n or
// the diagonal cuts pays the per-score compare.  The longest workgroups come first.
//
// K / V tiles come in one tile ahead, into two swizzled [64][64] images each.  Cache tiles and the chunk's V
// tiles (and, unrotated, its K tiles) arrive by LDS-DMA (glds16).  Chunk keys / values are read from qkv_new,
// never from the cache, and no cache row >= n is read: a staged row past the end of its part (>= n in the
// cache, >= t in the chunk) is a copy of that part's last valid row, and its scores are replaced by -inf (a
// select), so the probabilities there are exact zeros against finite values.  With ROPE the chunk's K tiles
// cannot come by DMA (they are not rotated in memory): a thread loads both halves of a (row, 8-column) pair and
// its 16 table values a tile ahead, when the DMA of that tile is issued, and after the current tile's
// arithmetic rotates them and writes the two 16-byte pieces into the same swizzled image with plain LDS stores.
// Those stores are waited for (lgkmcnt) by the wave that made them in front of the barrier that publishes the
// tile, as the DMA is (vmcnt); the image they go to was last read before the previous barrier.  Likewise a
// lane's Q fragments hold columns 8g .. and 32 + 8g .. of its query, a rotation pair: the Q rotation is
// lane-local, with 8 cos and 8 sin values of table row n + myq.
//
// Nothing this launch stores (rows n .. n+t-1) is read by it: no sync, no atomics, no second launch; plain
// vector stores; the same bits on every run.  The grid and the instance follow from B, Hkv, G and T alone;
// max_len, the host's bound on lens, only guards the capacity (max_len + T <= C, and the table's rows) and
// clamps a lens beyond it, so that every access stays in bounds.
#include "ddl_lds.h"

#include <algorithm>

namespace {

constexpr int XD = 64;           // head dim
constexpr int XTK = 64;          // keys per tile
constexpr int XROWB = 128;       // bytes per LDS row (64 bf16)
constexpr int XIMG = XTK * XROWB;
constexpr float LOG2E = 1.4426950408889634f;

// chunk swizzles of the two images (attention.hip's): K is read as rows (ds_read_b128), V transposed
__device__ __forceinline__ int xswz_k(int r, int c) { return c ^ ((r >> 1) & 7); }
__device__ __forceinline__ int xswz_v(int r, int c) { return c ^ (2 * ((r >> 1) & 3)); }

__device__ __forceinline__ void unpack8(const uint4& u, float* v) {
    v[0] = lo_f(u.x); v[1] = hi_f(u.x); v[2] = lo_f(u.y); v[3] = hi_f(u.y);
    v[4] = lo_f(u.z); v[5] = hi_f(u.z); v[6] = lo_f(u.w); v[7] = hi_f(u.w);
}
__device__ __forceinline__ uint4 pack8(const float* v) {
    return make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
}
__device__ __forceinline__ uint4 ld16(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void st16(bf16_t* p, const uint4& u) { *reinterpret_cast<uint4*>(p) = u; }

// rows row0 .. row0 + 63 of a [rows][ld] bf16 matrix (64 columns used) into a swizzled image; rows
// >= rows_valid (>= 1) are copies of the last valid one.  8 one-KB instructions dealt round-robin to the
// NW waves (wv wave-uniform); with NW = 3 or 6 the last round is short.
// (ddl_lds.h's dma_rows takes the row stride at compile time; the chunk's is (H + 2 Hkv) 64.)
template <int NW, bool V>
__device__ __forceinline__ void dma_tile(const bf16_t* src, long ld, int row0, int rows_valid, char* dst, int wv,
                                         int lane) {
#pragma unroll
    for (int qq = 0; qq < (8 + NW - 1) / NW; ++qq) {
        const int q = qq * NW + wv;
        if (8 % NW == 0 || q < 8) {
            const int r = q * 8 + (lane >> 3), cl = lane & 7;
            const int c = V ? xswz_v(r, cl) : xswz_k(r, cl);
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
    return *reinterpret_cast<const bf16x8*>(img + r * XROWB + (xswz_k(r, kk * 4 + (lane >> 4)) << 4));
}

// transposed fragment of the V image in the accumulator k order: lane gets column cbase + (lane & 15)
// of rows kb + 16 hh + 4 g + {0..3}, hh = 0, 1
__device__ __forceinline__ bf16x8 frag_vt(const char* img, int kb, int cbase, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int col = cbase + 4 * p;
    const int ra = kb + 4 * g + q, rb = ra + 16;
    const s16x4 lo = lds_read_tr((lds_v4*)(img + ra * XROWB + (xswz_v(ra, col >> 3) << 4) + (p & 1) * 8));
    const s16x4 hi = lds_read_tr((lds_v4*)(img + rb * XROWB + (xswz_v(rb, col >> 3) << 4) + (p & 1) * 8));
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

template <int G, int NS, bool ROPE>
__global__ __launch_bounds__(64 * G * NS) void attn_extend_k(
    const bf16_t* __restrict__ qkv, const float* __restrict__ tab, bf16_t* __restrict__ kcache,
    bf16_t* __restrict__ vcache, const int* __restrict__ lens, const int* __restrict__ new_lens,
    bf16_t* __restrict__ out, int T, int Hkv, int C, int max_len, float scale) {
    static_assert(ROPE || G == 1, "the unrotated append below deals a workgroup's 16 TQ pieces to 64 NS threads");
    constexpr int NW = G * NS, NT = 64 * NW, TQ = 16 * NS;
    constexpr int NU = (256 + NT - 1) / NT;     // rotation pairs of a K tile (64 rows x 4) per thread
    __shared__ __attribute__((aligned(16))) char smem[4 * XIMG];   // K0 V0 K1 V1
    const int qt = (int)(gridDim.x - 1 - blockIdx.x), hkv = blockIdx.y, b = blockIdx.z;   // longest loop first
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4;
    // this wave's query head of the group and its 16-query sub-tile (ROPE = false is G = 1: no division)
    const int hg = ROPE ? wv / NS : 0, sub = ROPE ? wv % NS : wv;
    const int H = Hkv * G, h = hkv * G + hg;
    // a lens beyond the host's bound, or a new_lens outside 1 .. T, would index past the cache, the table
    // or the chunk: clamp (the result is then the caller's problem, every access stays in bounds)
    const int n = min(max(lens[b], 0), max_len);
    const int tl = new_lens ? min(max(new_lens[b], 1), T) : T;

    // (ROPE = false is G = 1, Hkv = H, h = hkv: the layout's offsets are then multiples of HD from the query's)
    const long HD = (long)H * XD, rs = ROPE ? (long)(H + 2 * Hkv) * XD : 3 * HD;
    const bf16_t* rowb = qkv + (long)b * T * rs;
    const bf16_t* qb = rowb + (long)h * XD;
    const bf16_t* kb = ROPE ? rowb + (long)(H + hkv) * XD : qb + HD;
    const bf16_t* vb = ROPE ? rowb + (long)(H + Hkv + hkv) * XD : qb + 2 * HD;
    const float* tb = ROPE ? tab + (long)n * XD : nullptr;      // the table row of chunk position 0
    bf16_t* ck = kcache + ((long)b * Hkv + hkv) * C * XD;
    bf16_t* cv = vcache + ((long)b * Hkv + hkv) * C * XD;
    const int q0 = qt * TQ, q0w = q0 + 16 * sub, myq = q0w + (lane & 15);
    bf16_t* orow = out + ((long)b * T + myq) * HD + (long)h * XD + 4 * g;

    if (q0 >= tl) {     // padded queries only: zeros, nothing to append
        if (myq < T) {
#pragma unroll
            for (int db = 0; db < 4; ++db) *reinterpret_cast<uint2*>(orow + 16 * db) = make_uint2(0u, 0u);
        }
        return;
    }

    // append, once per KV head: this workgroup's chunk positions q0 .. q0 + TQ - 1 (those < tl)
    if constexpr (ROPE) {
        // the rotated keys: one pair per thread of the first NS waves, rotated once more instead of read back
        // from LDS (the same function, so the same bits); the values: 16-byte bit copies
        if (tid < 4 * TQ) {
            const int j = q0 + (tid >> 2), jc = min(j, tl - 1), c4 = tid & 3;
            const RotIn ri = rot_load(kb + (long)jc * rs, tb + (long)jc * XD, c4);
            uint4 lo, hi;
            rot_apply(ri, lo, hi);
            if (j < tl) {
                st16(ck + (long)(n + j) * XD + 8 * c4, lo);
                st16(ck + (long)(n + j) * XD + 32 + 8 * c4, hi);
            }
        }
#pragma unroll
        for (int i = 0; i < (8 * TQ + NT - 1) / NT; ++i) {
            const int piece = tid + i * NT;
            const int j = q0 + (piece >> 3), s8 = piece & 7;
            if (piece < 8 * TQ && j < tl) st16(cv + (long)(n + j) * XD + s8 * 8, ld16(vb + (long)j * rs + s8 * 8));
        }
    } else {
        // keys and values are 16-byte bit copies, four per thread; the four loads first, then the four stores
        // (a store behind each load waited out each round trip in turn)
        uint4 u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = tid + i * NT;
            const int s8 = piece & 7, kv = (piece >> 3) & 1, j = min(q0 + (piece >> 4), tl - 1);
            u[i] = ld16((kv ? vb : kb) + (long)j * rs + s8 * 8);
        }
        // (opaque here, or the compiler sinks each load back under its store's predicate)
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(u[i].x), "+v"(u[i].y), "+v"(u[i].z), "+v"(u[i].w));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = tid + i * NT;
            const int s8 = piece & 7, kv = (piece >> 3) & 1, j = q0 + (piece >> 4);
            if (j < tl) st16((kv ? cv : ck) + (long)(n + j) * XD + s8 * 8, u[i]);
        }
    }

    // Q fragments (B operand of S^T = K Q^T): lane holds Q[myq][32 kk + 8 g + 0..7], rotated with ROPE
    bf16x8 qf[2];
    {
        const int jq = min(myq, tl - 1);
        const bf16_t* qr = qb + (long)jq * rs;
        if constexpr (ROPE) {
            const RotIn ri = rot_load(qr, tb + (long)jq * XD, g);
            uint4 lo, hi;
            rot_apply(ri, lo, hi);
            qf[0] = __builtin_bit_cast(bf16x8, lo);
            qf[1] = __builtin_bit_cast(bf16x8, hi);
        } else {
            qf[0] = *reinterpret_cast<const bf16x8*>(qr + 8 * g);
            qf[1] = *reinterpret_cast<const bf16x8*>(qr + 32 + 8 * g);
        }
    }

    const int nc = (n + XTK - 1) / XTK;                         // cache tiles
    const int nd = min(q0 + TQ - 1, tl - 1) / XTK + 1;           // chunk tiles, through the diagonal one
    const int ntot = nc + nd;
    RotIn kin[NU];                                               // ROPE: the next chunk K tile's pairs, in flight
    // issue tile i: DMA for everything but a chunk K tile under ROPE, whose pairs go to registers
    auto stage = [&](int i, int buf) __attribute__((always_inline)) {
        char* sK = smem + buf * 2 * XIMG;
        if (i < nc) {
            dma_tile<NW, false>(ck, XD, i * XTK, n, sK, wv, lane);
            dma_tile<NW, true>(cv, XD, i * XTK, n, sK + XIMG, wv, lane);
        } else {
            const int row0 = (i - nc) * XTK;
            if constexpr (!ROPE) dma_tile<NW, false>(kb, rs, row0, tl, sK, wv, lane);
            dma_tile<NW, true>(vb, rs, row0, tl, sK + XIMG, wv, lane);
            if constexpr (ROPE) {
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int unit = tid + u * NT;
                    if (256 % NT == 0 || unit < 256) {
                        const int jc = min(row0 + (unit >> 2), tl - 1);  // a clamped row rotates by its clamped position
                        kin[u] = rot_load(kb + (long)jc * rs, tb + (long)jc * XD, unit & 3);
                    }
                }
            }
        }
    };
    // ROPE: rotate a chunk K tile's pairs and write them into the swizzled K image
    auto land = [&](int i, int buf) __attribute__((always_inline)) {
        if constexpr (ROPE) {
            if (i < nc) return;
            char* sK = smem + buf * 2 * XIMG;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int unit = tid + u * NT;
                if (256 % NT == 0 || unit < 256) {
                    const int r = unit >> 2, c4 = unit & 3;
                    uint4 lo, hi;
                    rot_apply(kin[u], lo, hi);
                    *reinterpret_cast<uint4*>(sK + r * XROWB + (xswz_k(r, c4) << 4)) = lo;
                    *reinterpret_cast<uint4*>(sK + r * XROWB + (xswz_k(r, c4 + 4) << 4)) = hi;
                }
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
        if constexpr (ROPE) LGKM0();
        VMN(0);
        BARRIER();
        // (none after the last tile: LDS-DMA must not be landing when the workgroup exits)
        if (i + 1 < ntot) stage(i + 1, (i + 1) & 1);
        if (active) {
            const char* sK = smem + (i & 1) * 2 * XIMG;
            const char* sV = sK + XIMG;
            // keys key0 + j of this part are visible to this lane's query while key0 + j < limit
            const bool cache = i < nc;
            const int key0 = (cache ? i : i - nc) * XTK;
            const int limit = cache ? n : myq + 1;
            const bool cut = cache ? key0 + XTK > n : key0 + XTK - 1 > q0w;     // per wave
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

inline bool ext_group_ok(int H, int Hkv) {
    if (Hkv < 1 || H < Hkv || H % Hkv) return false;
    const int G = H / Hkv;
    return G == 1 || G == 2 || G == 3 || G == 4 || G == 8;
}

// 16-query sub-tiles per workgroup for a chunk of T tokens and a group of G heads: 1 / 2 / 4, capped so
// that G NS <= 8 waves
inline int ext_subtiles(int T, int G) {
    const int want = T <= 16 ? 1 : (T <= 32 ? 2 : 4);
    const int cap = G >= 8 ? 1 : (G >= 3 ? 2 : 4);
    return std::min(want, cap);
}

}  // namespace

#define EXT_LAUNCH(G_, NS_, ROPE_, tab_, Hkv_)                                                                         \
    attn_extend_k<G_, NS_, ROPE_><<<dim3((T + 16 * NS_ - 1) / (16 * NS_), Hkv_, B), 64 * G_ * NS_, 0, st>>>(           \
        (const bf16_t*)qkv_new, tab_, (bf16_t*)kcache, (bf16_t*)vcache, (const int*)lens, (const int*)new_lens,        \
        (bf16_t*)out, T, Hkv_, C, max_len, scale)

DDL_API int ddl_attn_extend(const void* qkv_new, void* kcache, void* vcache, const void* lens, const void* new_lens,
                            void* out, int B, int T, int H, int C, int max_len, float scale, hipStream_t st) {
    if (B <= 0 || T <= 0 || H <= 0) return 0;
    if (max_len < 0 || (long)max_len + T > C || H > 65535 || B > 65535) return (int)hipErrorInvalidValue;
    switch (ext_subtiles(T, 1)) {
        case 1: EXT_LAUNCH(1, 1, false, nullptr, H); break;
        case 2: EXT_LAUNCH(1, 2, false, nullptr, H); break;
        default: EXT_LAUNCH(1, 4, false, nullptr, H); break;
    }
    DDL_RETURN_LAUNCH();
}

// 1 when the rotary extend kernel has an instance for this group size (the decode kernel's set)
DDL_API int ddl_attn_extend_gqa_supported(int H, int Hkv) { return ext_group_ok(H, Hkv) ? 1 : 0; }
// queries per workgroup for this (T, H, Hkv): what the launch will use (0 without an instance)
DDL_API int ddl_attn_extend_gqa_tile(int T, int H, int Hkv) {
    return ext_group_ok(H, Hkv) ? 16 * ext_subtiles(T, H / Hkv) : 0;
}

DDL_API int ddl_attn_extend_gqa(const void* qkv_new, const float* tab, void* kcache, void* vcache, const void* lens,
                                const void* new_lens, void* out, int B, int T, int H, int Hkv, int C, int max_len,
                                long n_pos, float scale, hipStream_t st) {
    if (!ext_group_ok(H, Hkv)) return (int)hipErrorInvalidValue;
    if (B <= 0 || T <= 0) return 0;
    if (max_len < 0 || (long)max_len + T > C || (long)max_len + T > n_pos || Hkv > 65535 || B > 65535)
        return (int)hipErrorInvalidValue;
    const int G = H / Hkv;
    switch (G * 8 + ext_subtiles(T, G)) {
        case 1 * 8 + 1: EXT_LAUNCH(1, 1, true, tab, Hkv); break;
        case 1 * 8 + 2: EXT_LAUNCH(1, 2, true, tab, Hkv); break;
        case 1 * 8 + 4: EXT_LAUNCH(1, 4, true, tab, Hkv); break;
        case 2 * 8 + 1: EXT_LAUNCH(2, 1, true, tab, Hkv); break;
        case 2 * 8 + 2: EXT_LAUNCH(2, 2, true, tab, Hkv); break;
        case 2 * 8 + 4: EXT_LAUNCH(2, 4, true, tab, Hkv); break;
        case 3 * 8 + 1: EXT_LAUNCH(3, 1, true, tab, Hkv); break;
        case 3 * 8 + 2: EXT_LAUNCH(3, 2, true, tab, Hkv); break;
        case 4 * 8 + 1: EXT_LAUNCH(4, 1, true, tab, Hkv); break;
        case 4 * 8 + 2: EXT_LAUNCH(4, 2, true, tab, Hkv); break;
        case 8 * 8 + 1: EXT_LAUNCH(8, 1, true, tab, Hkv); break;
        default: return (int)hipErrorInvalidValue;
    }
    DDL_RETURN_LAUNCH();
}
#undef EXT_LAUNCH
