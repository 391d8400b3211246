// Chunk (extend) attention over a key/value cache: T new tokens per sequence attend to the cached
// keys and, causally, to the chunk's own keys; the chunk's keys / values are appended.  Forward only,
// head dim 64, bf16, one query row per KV head (MHA).
//
// Inputs: qkv_new [B, T, 3 H 64] (the chunk's packed projection), kcache / vcache [B, H, C, 64],
// lens [B] int32 and the optional new_lens [B] int32 on the device.  For batch row b with n = lens[b]
// and t = new_lens[b] (T without new_lens; 1 <= t <= T), query i < t attends to cached keys 0 .. n-1
// and to chunk keys 0 .. i; out [B, T, H 64] rows i >= t are zeros.  The K / V rows of chunk
// positions i < t are stored to cache[b, h, n + i]; lens is not modified (all layers share it).
//
// One workgroup = NW waves = 16 NW consecutive queries of one (b, h): the structure of attention.hip's
// forward -- S^T = K Q^T on v_mfma_f32_16x16x32_bf16 (query on the lane, a 64-key tile's scores in
// the accumulators), fp32 online softmax on exp2, P rounded to bf16 and fed from the accumulator
// registers as the B operand of O^T += V^T P^T.  The key loop runs over ceil(n / 64) cache tiles (the
// bound a scalar read of lens) and then over the chunk tiles up to the one that holds the
// workgroup's last query.  Only a tile that n or the diagonal cuts pays the per-score compare.
//
// K / V tiles come in by LDS-DMA (glds16), one tile ahead, into two swizzled [64][64] images each.
// Chunk keys / values are read from qkv_new, never from the cache, and no cache row >= n is read: a
// staged row past the end of its part (>= n in the cache, >= t in the chunk) is a copy of that part's
// last valid row, and its scores are replaced by -inf (a select), so the probabilities there are exact
// zeros against finite values.  Nothing this launch stores (rows n .. n+t-1) is read by it: no sync,
// no atomics, no second launch; plain vector stores; the same bits on every run.
//
// The grid (query tiles, H, B) and NW (1 / 2 / 4 waves for T <= 16 / <= 32 / more) follow from B, H
// and T alone; max_len, the host's bound on lens, only guards the capacity (max_len + T <= C) and
// clamps a lens beyond it, so that every store stays inside the cache.
#include "ddl_lds.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int XD = 64;           // head dim
constexpr int XTK = 64;          // keys per tile
constexpr int XROWB = 128;       // bytes per LDS row (64 bf16)
constexpr int XIMG = XTK * XROWB;
constexpr float LOG2E = 1.4426950408889634f;

// chunk swizzles of the two images (attention.hip's): K is read as rows (ds_read_b128), V transposed
__device__ __forceinline__ int xswz_k(int r, int c) { return c ^ ((r >> 1) & 7); }
__device__ __forceinline__ int xswz_v(int r, int c) { return c ^ (2 * ((r >> 1) & 3)); }

// rows row0 .. row0 + 63 of a [rows][ld] bf16 matrix (64 columns used) into a swizzled image; rows
// >= rows_valid (>= 1) are copies of the last valid one.  8 one-KB instructions, split over the waves.
// (ddl_lds.h's dma_rows takes the row stride at compile time; the chunk's is 3 H 64.)
template <int NW, bool V>
__device__ __forceinline__ void dma_tile(const bf16_t* src, long ld, int row0, int rows_valid, char* dst, int wv,
                                         int lane) {
#pragma unroll
    for (int qq = 0; qq < 8 / NW; ++qq) {
        const int q = qq * NW + wv;
        const int r = q * 8 + (lane >> 3), cl = lane & 7;
        const int c = V ? xswz_v(r, cl) : xswz_k(r, cl);
        const long gr = min(row0 + r, rows_valid - 1);
        glds16(src + gr * ld + c * 8, dst + q * 1024);     // default policy: every query tile re-reads it
    }
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

template <int NW>
__global__ __launch_bounds__(64 * NW) void attn_extend_k(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kcache,
                                                         bf16_t* __restrict__ vcache, const int* __restrict__ lens,
                                                         const int* __restrict__ new_lens, bf16_t* __restrict__ out,
                                                         int T, int H, int C, int max_len, float scale) {
    constexpr int TQ = 16 * NW, NT = 64 * NW;
    __shared__ __attribute__((aligned(16))) char smem[4 * XIMG];   // K0 V0 K1 V1
    const int qt = (int)(gridDim.x - 1 - blockIdx.x), h = blockIdx.y, b = blockIdx.z;   // longest loop first
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4;
    // a lens beyond the host's bound, or a new_lens outside 1 .. T, would index past the cache or the
    // chunk: clamp (the result is then the caller's problem, every access stays in bounds)
    const int n = min(max(lens[b], 0), max_len);
    const int tl = new_lens ? min(max(new_lens[b], 1), T) : T;

    const long HD = (long)H * XD, rs = 3 * HD;
    const bf16_t* qb = qkv + (long)b * T * rs + (long)h * XD;
    const bf16_t* kb = qb + HD;
    const bf16_t* vb = qb + 2 * HD;
    bf16_t* ck = kcache + ((long)b * H + h) * C * XD;
    bf16_t* cv = vcache + ((long)b * H + h) * C * XD;
    const int q0 = qt * TQ, q0w = q0 + 16 * wv, myq = q0w + (lane & 15);
    bf16_t* orow = out + ((long)b * T + myq) * HD + (long)h * XD + 4 * g;

    if (q0 >= tl) {     // padded queries only: zeros, nothing to append
        if (myq < T) {
#pragma unroll
            for (int db = 0; db < 4; ++db) *reinterpret_cast<uint2*>(orow + 16 * db) = make_uint2(0u, 0u);
        }
        return;
    }

    // append: this workgroup's chunk positions q0 .. q0 + TQ - 1 (those < tl), 16-byte pieces; the four
    // loads first, then the four stores (a store behind each load waited out each round trip in turn)
    {
        uint4 u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = tid + i * NT;
            const int sub = piece & 7, kv = (piece >> 3) & 1, j = min(q0 + (piece >> 4), tl - 1);
            u[i] = *reinterpret_cast<const uint4*>((kv ? vb : kb) + (long)j * rs + sub * 8);
        }
        // (opaque here, or the compiler sinks each load back under its store's predicate)
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(u[i].x), "+v"(u[i].y), "+v"(u[i].z), "+v"(u[i].w));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = tid + i * NT;
            const int sub = piece & 7, kv = (piece >> 3) & 1, j = q0 + (piece >> 4);
            if (j < tl) *reinterpret_cast<uint4*>((kv ? cv : ck) + (long)(n + j) * XD + sub * 8) = u[i];
        }
    }

    // Q fragments (B operand of S^T = K Q^T): lane holds Q[myq][32 kk + 8 g + 0..7]
    bf16x8 qf[2];
    {
        const bf16_t* qr = qb + (long)min(myq, tl - 1) * rs + 8 * g;
        qf[0] = *reinterpret_cast<const bf16x8*>(qr);
        qf[1] = *reinterpret_cast<const bf16x8*>(qr + 32);
    }

    const int nc = (n + XTK - 1) / XTK;                         // cache tiles
    const int nd = min(q0 + TQ - 1, tl - 1) / XTK + 1;           // chunk tiles, through the diagonal one
    const int ntot = nc + nd;
    auto stage = [&](int i, int buf) __attribute__((always_inline)) {
        char* sK = smem + buf * 2 * XIMG;
        if (i < nc) {
            dma_tile<NW, false>(ck, XD, i * XTK, n, sK, wv, lane);
            dma_tile<NW, true>(cv, XD, i * XTK, n, sK + XIMG, wv, lane);
        } else {
            dma_tile<NW, false>(kb, rs, (i - nc) * XTK, tl, sK, wv, lane);
            dma_tile<NW, true>(vb, rs, (i - nc) * XTK, tl, sK + XIMG, wv, lane);
        }
    };

    const float c2 = scale * LOG2E;                              // scores in the exp2 domain
    const bool active = q0w < tl;                                // per wave: it has a valid query
    float m = -INFINITY, lsum = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    stage(0, 0);
    for (int i = 0; i < ntot; ++i) {
        // tile i has landed (this wave's DMA, then everyone's); everyone is done with the other image
        VMN(0);
        BARRIER();
        // (none after the last tile: LDS-DMA must not be landing when the workgroup exits)
        if (i + 1 < ntot) stage(i + 1, (i + 1) & 1);
        if (!active) continue;
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
                s[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_k(sK, 16 * blk, kk, lane), qf[kk], s[blk], 0, 0, 0);
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
                o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_vt(sV, 32 * st, 16 * db, lane), pf, o[db], 0, 0, 0);
        }
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

// waves per workgroup (16 queries each) for a chunk of T tokens
inline int ext_waves(int T) { return T <= 16 ? 1 : (T <= 32 ? 2 : 4); }

}  // namespace

DDL_API int ddl_attn_extend(const void* qkv_new, void* kcache, void* vcache, const void* lens, const void* new_lens,
                            void* out, int B, int T, int H, int C, int max_len, float scale, hipStream_t st) {
    if (B <= 0 || T <= 0 || H <= 0) return 0;
    if (max_len < 0 || (long)max_len + T > C || H > 65535 || B > 65535) return (int)hipErrorInvalidValue;
    const int nw = ext_waves(T);
    const dim3 grid((T + 16 * nw - 1) / (16 * nw), H, B);
    auto launch = [&](auto nwc) {
        constexpr int NW = decltype(nwc)::value;
        attn_extend_k<NW><<<grid, 64 * NW, 0, st>>>((const bf16_t*)qkv_new, (bf16_t*)kcache, (bf16_t*)vcache,
                                                    (const int*)lens, (const int*)new_lens, (bf16_t*)out, T, H, C,
                                                    max_len, scale);
    };
    if (nw == 1) launch(std::integral_constant<int, 1>{});
    else if (nw == 2) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, 4>{});
    DDL_RETURN_LAUNCH();
}
