// Single-query (decode) attention over a key/value cache, with the new token's append and, for the rotary
// (Llama) family, its rotation; and the cache fill after a prefill.  Head dim 64, bf16.
//
// Cache: per layer kcache / vcache [B, Hkv, C, 64] bf16 (a head's keys are contiguous 128-byte rows), lens [B]
// int32 on the device.  qkv_new [B, (H + 2 Hkv) 64] is the new token's fused projection [q heads | k heads |
// v heads]; G = H / Hkv query heads share a KV head.  For batch row b with n = lens[b] the queries attend to
// cached keys 0 .. n-1 and to the new key, which is read from qkv_new, never from the cache; the lane group
// that owns position n also stores the new K / V rows to cache[b, hkv, n] (plain 16-byte vector stores).  No
// workgroup reads a row another one writes in the same launch, and lens is not modified (all layers of a step
// share it).
//
// One kernel, attn_decode_k<G, U, ROPE>, serves both families:
//   - ROPE = false (GPT-2: ddl_attn_decode, G = 1): the packed [B, 3 H 64] projection is the layout above with
//     Hkv = H; queries and the new key are used as they are, and no table is read.
//   - ROPE = true (ddl_attn_decode_gqa, G in {1, 2, 3, 4, 8}): the cache holds ROTATED keys and qkv_new is
//     UNROTATED.  tab [n_pos, 64] is the fp32 rotary table (row s = [cos 0..31 | sin 0..31]); the G queries of
//     a KV head and the new key are rotated by table row n (HF half-split pairs i / i+32, fp32, the expression
//     of llama.hip's rope_qkv_fwd_k, rounded ONCE to bf16: the operand bits a full forward sees after
//     rope_qkv), and the rotated key is what is appended.  The value is a bit copy.
//
// Memory / latency bound, so VALU, no MFMA, no LDS staging of K / V: a key row is 8 x 16 bytes, 8 lanes (one
// "group") own a key, each lane the 8 head-dim elements of its 16-byte piece for both the score (8 FMAs + a
// 3-step reduce over the group) and the P V accumulation.  A 256-thread workgroup is 32 groups; each takes U
// keys per round (2 U 16-byte loads in flight per lane).  Every K / V row is loaded ONCE and scored against
// all G queries of its KV head -- G online-softmax states (m, l, acc[8], exp2 domain) per lane -- so a step
// reads the cache bytes of Hkv heads, not of H.  The 32 group states of up to 4 query heads merge through LDS
// at a time, in group order (33 KB at G >= 4); G = 8 takes two passes over the same buffer and U = 2.
//
// Split-KV: grid (nsplit, Hkv, B); split s covers positions [s chunk, (s+1) chunk), clipped to n+1.  nsplit and
// chunk come from B Hkv and max_len (the host's upper bound on n+1) alone, so the grid never depends on device
// data; the two entry points differ only in the cap on nsplit (16 and 32: fewer workgroups per split with
// grouped heads, so more splits).  A split whose range is empty writes an empty partial (m = -inf, l = 0) and
// touches no cache row.  Partials go to ws ([B H nsplit] x (m, l) then x 64 fp32) and a second launch merges
// them in split order: no float atomics, no in-launch hand-off; nsplit = 1 writes out directly.  Positions
// past n are never loaded (selects, not multiplies, keep them out), so whatever bit patterns the unwritten
// part of the cache holds cannot reach the output.
#include "ddl_common.h"

namespace {

constexpr int DEC_D = 64;
constexpr int DEC_NT = 256;                 // threads per workgroup
constexpr int DEC_GRPS = DEC_NT / 8;        // key groups per workgroup
constexpr int DEC_MAX_SPLIT = 16;           // ddl_attn_decode
constexpr int DEC_MAX_SPLIT_GQA = 32;       // ddl_attn_decode_gqa
constexpr int DEC_MIN_CHUNK = 64;           // positions per split, at least (and a multiple of DEC_GRPS)
constexpr float LOG2E = 1.4426950408889634f;

struct DecPlan {
    int nsplit, chunk;
};

// From max_len alone: enough splits (max_split at most) that B Hkv nsplit covers the chip, each at least
// DEC_MIN_CHUNK positions, chunk a multiple of DEC_GRPS.
inline DecPlan dec_plan(int B, int Hkv, int max_len, int max_split) {
    const int bh = std::max(1, B * Hkv);
    int want = std::min(max_split, (num_cus() + bh - 1) / bh);
    want = std::max(1, std::min(want, (max_len + DEC_MIN_CHUNK - 1) / DEC_MIN_CHUNK));
    int chunk = (max_len + want - 1) / want;
    chunk = (chunk + DEC_GRPS - 1) / DEC_GRPS * DEC_GRPS;
    return {(max_len + chunk - 1) / chunk, chunk};
}

__device__ __forceinline__ void unpack8(const uint4& u, float* v) {
    v[0] = lo_f(u.x); v[1] = hi_f(u.x); v[2] = lo_f(u.y); v[3] = hi_f(u.y);
    v[4] = lo_f(u.z); v[5] = hi_f(u.z); v[6] = lo_f(u.w); v[7] = hi_f(u.w);
}
__device__ __forceinline__ uint4 pack8(const float* v) {
    return make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
}
__device__ __forceinline__ uint4 ld16(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void st16(bf16_t* p, const uint4& u) { *reinterpret_cast<uint4*>(p) = u; }

// sum over the 8 lanes of a group (lanes 8 g .. 8 g + 7): xor 1, 2 inside the quad, then xor 4
__device__ __forceinline__ float group8_sum(float v) {
    v = dpp_add<0xB1>(v);
    v = dpp_add<0x4E>(v);
    return v + __shfl_xor(v, 4, 64);
}

// This lane's 8 columns (sub * 8 ..) of one head rotated by (c, sn), the table's entries for columns
// 8 (sub & 3) .. of the low half.  Both halves are formed by rope_qkv_fwd_k's expressions, operand order
// included, and the lane keeps its own: lanes 0-3 of a group own the low half, lanes 4-7 the high one.
__device__ __forceinline__ uint4 rotate8(const bf16_t* head, int sub, const float* c, const float* sn) {
    float x1[8], x2[8], o1[8], o2[8];
    unpack8(ld16(head + 8 * (sub & 3)), x1);
    unpack8(ld16(head + 32 + 8 * (sub & 3)), x2);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o1[e] = x1[e] * c[e] - x2[e] * sn[e];
        o2[e] = x2[e] * c[e] + x1[e] * sn[e];
    }
    const uint4 lo = pack8(o1), hi = pack8(o2);
    return sub < 4 ? lo : hi;
}

template <int G, int U, bool ROPE>
__global__ __launch_bounds__(DEC_NT) void attn_decode_k(const bf16_t* __restrict__ qkv_new, const float* __restrict__ tab,
                                                        bf16_t* __restrict__ kcache, bf16_t* __restrict__ vcache,
                                                        const int* __restrict__ lens, bf16_t* __restrict__ out,
                                                        float* __restrict__ ws, int Hkv, int C, int max_len, int chunk,
                                                        float scale) {
    constexpr int NH = G < 4 ? G : 4;       // query heads merged through LDS at a time
    __shared__ float s_ml[NH][DEC_GRPS][2];
    __shared__ float s_acc[NH][DEC_GRPS][DEC_D];
    const int split = blockIdx.x, nsplit = gridDim.x, hkv = blockIdx.y, b = blockIdx.z, B = gridDim.z;
    const int tid = threadIdx.x, grp = tid >> 3, sub = tid & 7;
    const int H = Hkv * G;
    // lens beyond the host's bound would index past the cache and the table: clamp (the result is
    // then the caller's problem, the accesses stay inside)
    const int n = std::min(std::max(lens[b], 0), max_len - 1);
    const int start = split * chunk, end = std::min(start + chunk, n + 1);

    const bf16_t* row = qkv_new + (long)b * (H + 2 * Hkv) * DEC_D;
    const bf16_t* knew = row + (long)(H + hkv) * DEC_D;
    const bf16_t* vnew = row + (long)(H + Hkv + hkv) * DEC_D + sub * 8;
    const long cbase = ((long)b * Hkv + hkv) * C * DEC_D + sub * 8;
    const bf16_t* kbase = kcache + cbase;
    const bf16_t* vbase = vcache + cbase;

    // this lane's 16-byte piece of one head of the projection as the attention sees it: rotated by table row n,
    // or as it is
    float c[8], sn[8];
    if constexpr (ROPE) {
        load8(tab + (long)n * DEC_D + 8 * (sub & 3), c);
        load8(tab + (long)n * DEC_D + 32 + 8 * (sub & 3), sn);
    }
    auto head8 = [&](const bf16_t* head) __attribute__((always_inline)) {
        if constexpr (ROPE) return rotate8(head, sub, c, sn);
        else return ld16(head + sub * 8);
    };

    float q[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        unpack8(head8(row + (long)(hkv * G + g) * DEC_D), q[g]);
#pragma unroll
        for (int i = 0; i < 8; ++i) q[g][i] *= scale * LOG2E;       // scores in the exp2 domain
    }

    float m[G], l[G], acc[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        m[g] = -INFINITY;
        l[g] = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] = 0.f;
    }
    for (int jb = start; jb < end; jb += DEC_GRPS * U) {      // trip count uniform over the workgroup
        const int j0 = jb + grp;
        uint4 ku[U], vu[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * DEC_GRPS;
            ku[u] = make_uint4(0, 0, 0, 0);
            vu[u] = make_uint4(0, 0, 0, 0);
            if (j < end) {
                // the new key / value come from the projection, cached rows from the cache; the group that
                // owns position n appends
                if constexpr (ROPE) {
                    if (j == n) {
                        ku[u] = head8(knew);
                        vu[u] = ld16(vnew);
                        st16(kcache + cbase + (long)n * DEC_D, ku[u]);
                        st16(vcache + cbase + (long)n * DEC_D, vu[u]);
                    } else {
                        ku[u] = ld16(kbase + (long)j * DEC_D);
                        vu[u] = ld16(vbase + (long)j * DEC_D);
                    }
                } else {    // both are plain rows: a pointer select and one load each
                    ku[u] = ld16(j == n ? knew + sub * 8 : kbase + (long)j * DEC_D);
                    vu[u] = ld16(j == n ? vnew : vbase + (long)j * DEC_D);
                    if (j == n) {
                        st16(kcache + cbase + (long)n * DEC_D, ku[u]);
                        st16(vcache + cbase + (long)n * DEC_D, vu[u]);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool live = j0 + u * DEC_GRPS < end;
            float kf[8], vf[8];
            unpack8(ku[u], kf);
            unpack8(vu[u], vf);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float d = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) d = __builtin_fmaf(q[g][i], kf[i], d);
                d = group8_sum(d);
                const float s = live ? d : -INFINITY;
                const float mn = fmaxf(m[g], s);
                const float corr = m[g] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m[g] - mn);
                const float p = live ? __builtin_amdgcn_exp2f(s - mn) : 0.f;
                l[g] = __builtin_fmaf(l[g], corr, p);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[g][i] = __builtin_fmaf(acc[g][i], corr, p * vf[i]);
                m[g] = mn;
            }
        }
    }

    // merge the 32 group states in group order, NH query heads at a time: thread tid takes column
    // tid & 63 of head h0 + (tid >> 6)
    const int hh = tid >> 6, col = tid & 63;
#pragma unroll
    for (int h0 = 0; h0 < G; h0 += NH) {
        if (h0 > 0) __syncthreads();
#pragma unroll
        for (int g = 0; g < NH; ++g) {
            if (sub == 0) {
                s_ml[g][grp][0] = m[h0 + g];
                s_ml[g][grp][1] = l[h0 + g];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) s_acc[g][grp][sub * 8 + i] = acc[h0 + g][i];
        }
        __syncthreads();
        if (hh < NH) {
            float mm = -INFINITY;
#pragma unroll 8
            for (int g = 0; g < DEC_GRPS; ++g) mm = fmaxf(mm, s_ml[hh][g][0]);
            float ll = 0.f, o = 0.f;
#pragma unroll 8
            for (int g = 0; g < DEC_GRPS; ++g) {
                const float mg = s_ml[hh][g][0];
                const float w = mg == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mg - mm);
                ll = __builtin_fmaf(s_ml[hh][g][1], w, ll);
                o = __builtin_fmaf(s_acc[hh][g][col], w, o);
            }
            const int h = hkv * G + h0 + hh;
            if (nsplit == 1) {
                out[((long)b * H + h) * DEC_D + col] = f2bf(o / ll);    // ll >= 1: the new key is live
            } else {
                const long pi = ((long)b * H + h) * nsplit + split;
                float* ws_ml = ws;
                float* ws_acc = ws + (long)B * H * nsplit * 2;
                if (col == 0) {
                    ws_ml[pi * 2] = mm;
                    ws_ml[pi * 2 + 1] = ll;
                }
                ws_acc[pi * DEC_D + col] = o;
            }
        }
    }
}

// out[b, h, :] from the nsplit partials, in split order; one wave per (b, h)
__global__ __launch_bounds__(DEC_D) void attn_decode_merge_k(const float* __restrict__ ws, bf16_t* __restrict__ out, int H,
                                                             int nsplit) {
    const int h = blockIdx.x, b = blockIdx.y, B = gridDim.y, tid = threadIdx.x;
    const long p0 = ((long)b * H + h) * nsplit;
    const float* ws_ml = ws + p0 * 2;
    const float* ws_acc = ws + (long)B * H * nsplit * 2 + p0 * DEC_D;
    float mm = -INFINITY;
    for (int s = 0; s < nsplit; ++s) mm = fmaxf(mm, ws_ml[2 * s]);
    float ll = 0.f, o = 0.f;
    for (int s = 0; s < nsplit; ++s) {
        const float ms = ws_ml[2 * s];
        const float w = ms == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(ms - mm);
        ll = __builtin_fmaf(ws_ml[2 * s + 1], w, ll);
        o = __builtin_fmaf(ws_acc[(long)s * DEC_D + tid], w, o);
    }
    out[((long)b * H + h) * DEC_D + tid] = f2bf(o / ll);
}

// Slot hkv G of the K and V thirds of a packed [B, S, 3, Hkv G, 64] projection -> cache positions 0 .. S-1 of
// [B, Hkv, C, 64]; one thread per 16 bytes.  G = 1: GPT-2's projection, every head.  G > 1: rope_qkv's output
// (keys already rotated, every KV head repeated to G slots).
__global__ __launch_bounds__(256) void kv_cache_fill_k(const bf16_t* __restrict__ packed, bf16_t* __restrict__ kcache,
                                                       bf16_t* __restrict__ vcache, int S, int Hkv, int G, int C,
                                                       long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int sub = (int)(i & 7);
    long r = i >> 3;
    const int hkv = (int)(r % Hkv);
    r /= Hkv;
    const int kv = (int)(r & 1);
    r >>= 1;
    const int s = (int)(r % S);
    const long b = r / S;
    const long HD = (long)Hkv * G * DEC_D;
    const uint4 u = ld16(packed + (b * S + s) * 3 * HD + (1 + kv) * HD + (long)hkv * G * DEC_D + sub * 8);
    st16((kv ? vcache : kcache) + ((b * Hkv + hkv) * C + s) * DEC_D + sub * 8, u);
}

inline bool gqa_group_ok(int H, int Hkv) {
    if (Hkv < 1 || H < Hkv || H % Hkv) return false;
    const int G = H / Hkv;
    return G == 1 || G == 2 || G == 3 || G == 4 || G == 8;
}

// the decode launch and, with more than one split, the merge
template <int G, int U, bool ROPE>
inline void dec_launch(const DecPlan& pl, const void* qkv_new, const float* tab, void* kcache, void* vcache,
                       const void* lens, void* out, void* ws, int B, int Hkv, int C, int max_len, float scale,
                       hipStream_t st) {
    attn_decode_k<G, U, ROPE><<<dim3(pl.nsplit, Hkv, B), DEC_NT, 0, st>>>(
        (const bf16_t*)qkv_new, tab, (bf16_t*)kcache, (bf16_t*)vcache, (const int*)lens, (bf16_t*)out, (float*)ws, Hkv, C,
        max_len, pl.chunk, scale);
    if (pl.nsplit > 1)
        attn_decode_merge_k<<<dim3(Hkv * G, B), DEC_D, 0, st>>>((const float*)ws, (bf16_t*)out, Hkv * G, pl.nsplit);
}

inline int fill_launch(const void* packed, void* kcache, void* vcache, int B, int S, int Hkv, int G, int C,
                       hipStream_t st) {
    const long total = (long)B * S * 2 * Hkv * 8;
    kv_cache_fill_k<<<(unsigned)((total + 255) / 256), 256, 0, st>>>((const bf16_t*)packed, (bf16_t*)kcache,
                                                                    (bf16_t*)vcache, S, Hkv, G, C, total);
    DDL_RETURN_LAUNCH();
}

}  // namespace

// number of key splits for this (B, H, max_len): what the launch will use
DDL_API int ddl_attn_decode_nsplit(int B, int H, int max_len) {
    return dec_plan(B, H, std::max(1, max_len), DEC_MAX_SPLIT).nsplit;
}
// positions per split
DDL_API int ddl_attn_decode_chunk(int B, int H, int max_len) {
    return dec_plan(B, H, std::max(1, max_len), DEC_MAX_SPLIT).chunk;
}
// floats of workspace the launch needs (0 with one split)
DDL_API long ddl_attn_decode_ws(int B, int H, int max_len) {
    const int ns = dec_plan(B, H, std::max(1, max_len), DEC_MAX_SPLIT).nsplit;
    return ns == 1 ? 0 : (long)B * H * ns * (2 + DEC_D);
}

DDL_API int ddl_attn_decode(const void* qkv_new, void* kcache, void* vcache, const void* lens, void* out, void* ws, int B,
                            int H, int C, int max_len, float scale, hipStream_t st) {
    if (B <= 0 || H <= 0) return 0;
    if (max_len < 1 || max_len > C || H > 65535 || B > 65535) return (int)hipErrorInvalidValue;
    const DecPlan pl = dec_plan(B, H, max_len, DEC_MAX_SPLIT);
    if (pl.nsplit > 1 && !ws) return (int)hipErrorInvalidValue;
    dec_launch<1, 4, false>(pl, qkv_new, nullptr, kcache, vcache, lens, out, ws, B, H, C, max_len, scale, st);
    DDL_RETURN_LAUNCH();
}

DDL_API int ddl_kv_cache_fill(const void* qkv, void* kcache, void* vcache, int B, int S, int H, int C, hipStream_t st) {
    if (B <= 0 || S <= 0 || H <= 0) return 0;
    if (S > C) return (int)hipErrorInvalidValue;
    return fill_launch(qkv, kcache, vcache, B, S, H, 1, C, st);
}

// 1 when the rotary decode kernel has an instance for this group size
DDL_API int ddl_attn_decode_gqa_supported(int H, int Hkv) { return gqa_group_ok(H, Hkv) ? 1 : 0; }
// number of key splits for this (B, Hkv, max_len): what the launch will use
DDL_API int ddl_attn_decode_gqa_nsplit(int B, int Hkv, int max_len) {
    return dec_plan(B, Hkv, std::max(1, max_len), DEC_MAX_SPLIT_GQA).nsplit;
}
// positions per split
DDL_API int ddl_attn_decode_gqa_chunk(int B, int Hkv, int max_len) {
    return dec_plan(B, Hkv, std::max(1, max_len), DEC_MAX_SPLIT_GQA).chunk;
}
// floats of workspace the launch needs (0 with one split)
DDL_API long ddl_attn_decode_gqa_ws(int B, int H, int Hkv, int max_len) {
    const int ns = dec_plan(B, Hkv, std::max(1, max_len), DEC_MAX_SPLIT_GQA).nsplit;
    return ns == 1 ? 0 : (long)B * H * ns * (2 + DEC_D);
}

DDL_API int ddl_attn_decode_gqa(const void* qkv_new, const float* tab, void* kcache, void* vcache, const void* lens,
                                void* out, void* ws, int B, int H, int Hkv, int C, int max_len, long n_pos, float scale,
                                hipStream_t st) {
    if (!gqa_group_ok(H, Hkv)) return (int)hipErrorInvalidValue;
    if (B <= 0) return 0;
    if (max_len < 1 || max_len > C || max_len > n_pos || H > 65535 || B > 65535) return (int)hipErrorInvalidValue;
    const DecPlan pl = dec_plan(B, Hkv, max_len, DEC_MAX_SPLIT_GQA);
    if (pl.nsplit > 1 && !ws) return (int)hipErrorInvalidValue;
#define DEC_LAUNCH(G_, U_) \
    dec_launch<G_, U_, true>(pl, qkv_new, tab, kcache, vcache, lens, out, ws, B, Hkv, C, max_len, scale, st)
    switch (H / Hkv) {
        case 1: DEC_LAUNCH(1, 4); break;
        case 2: DEC_LAUNCH(2, 4); break;
        case 3: DEC_LAUNCH(3, 4); break;
        case 4: DEC_LAUNCH(4, 4); break;
        default: DEC_LAUNCH(8, 2); break;
    }
#undef DEC_LAUNCH
    DDL_RETURN_LAUNCH();
}

DDL_API int ddl_kv_cache_fill_gqa(const void* packed, void* kcache, void* vcache, int B, int S, int H, int Hkv, int C,
                                  hipStream_t st) {
    if (Hkv < 1 || H < Hkv || H % Hkv) return (int)hipErrorInvalidValue;
    if (B <= 0 || S <= 0) return 0;
    if (S > C) return (int)hipErrorInvalidValue;
    return fill_launch(packed, kcache, vcache, B, S, Hkv, H / Hkv, C, st);
}
