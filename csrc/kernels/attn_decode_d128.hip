// Rotary grouped-query single-query (decode) attention over a KV cache at HEAD DIM 128, with the new token's
// rotation and append, and the head-dim-128 cache fill: Llama-2-7B (32 / 32 heads), Llama-3-8B and Mistral-7B
// (32 / 8).  bf16.  The contract is attn_decode.hip's rotary one with D = 128:
//
// Cache: per layer kcache / vcache [B, Hkv, C, 128] bf16 of ROTATED keys (a head's keys are contiguous 256-byte
// rows), lens [B] int32 on the device.  qkv_new [B, (H + 2 Hkv) 128] is the new token's fused, UNROTATED
// projection [q heads | k heads | v heads]; G = H / Hkv in {1, 2, 3, 4, 8} query heads share a KV head.  tab
// [n_pos, 128] is the fp32 rotary table (row s = [cos 0..63 | sin 0..63]).  For batch row b with n = lens[b]
// the G queries of a KV head and the new key are rotated by table row n (HF half-split pairs i / i+64, fp32,
// the expression of llama.hip's rope_qkv_fwd_k, rounded ONCE to bf16); the queries attend to cached keys
// 0 .. n-1 and to the new key, which is read from qkv_new, never from the cache; the lanes that own position n
// store the rotated key and the bit-copied value to cache[b, hkv, n].  No workgroup reads a row another one
// writes in the same launch, and lens is not modified.
//
// Layout (not the D = 64 one with a constant doubled):
//   - A key row is 16 x 16 bytes and 16 lanes -- one DPP row -- own a key, each lane the 8 head-dim elements
//     of its piece for both the score and the P V accumulation.  So the per-lane state (q[G][8], acc[G][8],
//     m[G], l[G]) is exactly the D = 64 kernel's and G = 8 still fits in registers; 8 lanes x 16 columns would
//     double q and acc.  The score's 16-lane sum is ddl_common.h's row16_sum: quad_perm xor 1 and xor 2,
//     row_half_mirror, row_mirror -- four DPP adds, no cross-row shuffle, every lane of the row ending with the
//     same bits.
//   - Rotation pairs sit across the two half-rows: lanes 0-7 of a group own columns 8 sub of the low half,
//     lanes 8-15 the high half.  A lane loads both 16-byte pieces of its pair and the matching 8 cos and 8 sin
//     values, forms both halves and keeps its own.
//   - A 256-thread workgroup is 16 key groups (4 per wave); each takes U keys per round, 2 U 16-byte loads in
//     flight per lane as at D = 64 (U = 4; 2 at G = 8), so a round is 64 (32) keys = 32 (16) KB of rows.
//   - The 16 group states of up to 4 query heads merge through LDS at a time, in group order: 16 x 128 fp32 =
//     8 KB per head, 32.5 KB at G >= 4 (what the D = 64 kernel declares); one wave per head, two adjacent
//     columns per thread (8-byte LDS reads, a packed bf16 pair or a float2 out).  G = 8 takes two passes.
//
// Split-KV is attn_decode.hip's: grid (nsplit, Hkv, B) from dec_plan(B, Hkv, max_len) -- host values only; the
// chunk is a multiple of 32, so of the 16 groups -- empty splits write empty partials, partials go to ws
// ([B H nsplit] x (m, l) then x 128 fp32) and a second launch merges them in split order.  No atomics;
// bitwise repeatable.  Positions past n are never loaded and selects, not multiplies, keep them out.
#include "attn_decode.h"

namespace {

constexpr int D128 = 128;
constexpr int D128_GRPS = DEC_NT / 16;      // key groups per workgroup: 16 lanes (a DPP row) per key
static_assert(DEC_PLAN_ALIGN % D128_GRPS == 0, "a split's chunk must be whole rounds of groups");

// This lane's 8 columns (sub * 8 ..) of one head rotated by (c, sn), the table's entries for columns
// 8 (sub & 7) .. of the low half.  Both halves are formed by rope_qkv_fwd_k's expressions, operand order
// included, and the lane keeps its own: lanes 0-7 of a group own the low half, lanes 8-15 the high one.
__device__ __forceinline__ uint4 rotate8_d128(const bf16_t* head, int sub, const float* c, const float* sn) {
    float x1[8], x2[8], o1[8], o2[8];
    unpack8(ld16(head + 8 * (sub & 7)), x1);
    unpack8(ld16(head + D128 / 2 + 8 * (sub & 7)), x2);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o1[e] = x1[e] * c[e] - x2[e] * sn[e];
        o2[e] = x2[e] * c[e] + x1[e] * sn[e];
    }
    const uint4 lo = pack8(o1), hi = pack8(o2);
    return sub < 8 ? lo : hi;
}

template <int G, int U>
__global__ __launch_bounds__(DEC_NT) void attn_decode_d128_k(const bf16_t* __restrict__ qkv_new, const float* __restrict__ tab,
                                                             bf16_t* __restrict__ kcache, bf16_t* __restrict__ vcache,
                                                             const int* __restrict__ lens, bf16_t* __restrict__ out,
                                                             float* __restrict__ ws, int Hkv, int C, int max_len,
                                                             int chunk, float scale) {
    constexpr int NH = G < 4 ? G : 4;       // query heads merged through LDS at a time
    __shared__ float s_ml[NH][D128_GRPS][2];
    __shared__ __attribute__((aligned(16))) float s_acc[NH][D128_GRPS][D128];
    const int split = blockIdx.x, nsplit = gridDim.x, hkv = blockIdx.y, b = blockIdx.z, B = gridDim.z;
    const int tid = threadIdx.x, grp = tid >> 4, sub = tid & 15;
    const int H = Hkv * G;
    // lens beyond the host's bound would index past the cache and the table: clamp (the result is
    // then the caller's problem, the accesses stay inside)
    const int n = std::min(std::max(lens[b], 0), max_len - 1);
    const int start = split * chunk, end = std::min(start + chunk, n + 1);

    const bf16_t* row = qkv_new + (long)b * (H + 2 * Hkv) * D128;
    const bf16_t* knew = row + (long)(H + hkv) * D128;
    const bf16_t* vnew = row + (long)(H + Hkv + hkv) * D128 + sub * 8;
    const long cbase = ((long)b * Hkv + hkv) * C * D128 + sub * 8;
    const bf16_t* kbase = kcache + cbase;
    const bf16_t* vbase = vcache + cbase;

    // table row n: the 8 cos and 8 sin values of this lane's rotation pairs
    float c[8], sn[8];
    load8(tab + (long)n * D128 + 8 * (sub & 7), c);
    load8(tab + (long)n * D128 + D128 / 2 + 8 * (sub & 7), sn);

    float q[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        unpack8(rotate8_d128(row + (long)(hkv * G + g) * D128, sub, c, sn), q[g]);
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
    for (int jb = start; jb < end; jb += D128_GRPS * U) {     // trip count uniform over the workgroup
        const int j0 = jb + grp;
        uint4 ku[U], vu[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * D128_GRPS;
            ku[u] = make_uint4(0, 0, 0, 0);
            vu[u] = make_uint4(0, 0, 0, 0);
            if (j < end) {
                // the new key / value come from the projection, cached rows from the cache; the 16 lanes that
                // own position n append
                if (j == n) {
                    // (table row n again, through a pointer the optimiser cannot match with the one above:
                    // 16 cos / sin values kept live across the loop for this one key cost G = 8 its second wave)
                    const float* trow = tab + (long)n * D128 + 8 * (sub & 7);
                    asm volatile("" : "+v"(trow));
                    float ck[8], sk[8];
                    load8(trow, ck);
                    load8(trow + D128 / 2, sk);
                    ku[u] = rotate8_d128(knew, sub, ck, sk);
                    vu[u] = ld16(vnew);
                    st16(kcache + cbase + (long)n * D128, ku[u]);
                    st16(vcache + cbase + (long)n * D128, vu[u]);
                } else {
                    ku[u] = ld16(kbase + (long)j * D128);
                    vu[u] = ld16(vbase + (long)j * D128);
                }
            }
        }
        // (every lane of the wave is active here: the DPP row sum reads its 15 neighbours)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool live = j0 + u * D128_GRPS < end;
            float kf[8], vf[8];
            unpack8(ku[u], kf);
            unpack8(vu[u], vf);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float d = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) d = __builtin_fmaf(q[g][i], kf[i], d);
                d = row16_sum(d);
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

    // merge the 16 group states in group order, NH query heads at a time: wave hh takes head h0 + hh, its
    // lane the columns c2, c2 + 1
    const int hh = tid >> 6, c2 = (tid & 63) * 2;
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
#pragma unroll
            for (int g = 0; g < D128_GRPS; ++g) mm = fmaxf(mm, s_ml[hh][g][0]);
            float ll = 0.f, o0 = 0.f, o1 = 0.f;
#pragma unroll
            for (int g = 0; g < D128_GRPS; ++g) {
                const float mg = s_ml[hh][g][0];
                const float w = mg == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mg - mm);
                const float2 a = *reinterpret_cast<const float2*>(&s_acc[hh][g][c2]);
                ll = __builtin_fmaf(s_ml[hh][g][1], w, ll);
                o0 = __builtin_fmaf(a.x, w, o0);
                o1 = __builtin_fmaf(a.y, w, o1);
            }
            const int h = hkv * G + h0 + hh;
            if (nsplit == 1) {      // ll >= 1: the new key is live
                *reinterpret_cast<uint32_t*>(out + ((long)b * H + h) * D128 + c2) = pack2bf(o0 / ll, o1 / ll);
            } else {
                const long pi = ((long)b * H + h) * nsplit + split;
                float* ws_ml = ws;
                float* ws_acc = ws + (long)B * H * nsplit * 2;
                if (c2 == 0) {
                    ws_ml[pi * 2] = mm;
                    ws_ml[pi * 2 + 1] = ll;
                }
                *reinterpret_cast<float2*>(ws_acc + pi * D128 + c2) = make_float2(o0, o1);
            }
        }
    }
}

// out[b, h, :] from the nsplit partials, in split order; one 128-thread workgroup per (b, h)
__global__ __launch_bounds__(D128) void attn_decode_d128_merge_k(const float* __restrict__ ws, bf16_t* __restrict__ out,
                                                                 int H, int nsplit) {
    const int h = blockIdx.x, b = blockIdx.y, B = gridDim.y, tid = threadIdx.x;
    const long p0 = ((long)b * H + h) * nsplit;
    const float* ws_ml = ws + p0 * 2;
    const float* ws_acc = ws + (long)B * H * nsplit * 2 + p0 * D128;
    float mm = -INFINITY;
    for (int s = 0; s < nsplit; ++s) mm = fmaxf(mm, ws_ml[2 * s]);
    float ll = 0.f, o = 0.f;
    for (int s = 0; s < nsplit; ++s) {
        const float ms = ws_ml[2 * s];
        const float w = ms == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(ms - mm);
        ll = __builtin_fmaf(ws_ml[2 * s + 1], w, ll);
        o = __builtin_fmaf(ws_acc[(long)s * D128 + tid], w, o);
    }
    out[((long)b * H + h) * D128 + tid] = f2bf(o / ll);
}

// Slot hkv G of the K and V thirds of rope_qkv's packed [B, S, 3, Hkv G, 128] -> cache positions 0 .. S-1 of
// [B, Hkv, C, 128]; one thread per 16 bytes, 16 per row.
__global__ __launch_bounds__(256) void kv_cache_fill_d128_k(const bf16_t* __restrict__ packed, bf16_t* __restrict__ kcache,
                                                            bf16_t* __restrict__ vcache, int S, int Hkv, int G, int C,
                                                            long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int sub = (int)(i & 15);
    long r = i >> 4;
    const int hkv = (int)(r % Hkv);
    r /= Hkv;
    const int kv = (int)(r & 1);
    r >>= 1;
    const int s = (int)(r % S);
    const long b = r / S;
    const long HD = (long)Hkv * G * D128;
    const uint4 u = ld16(packed + (b * S + s) * 3 * HD + (1 + kv) * HD + (long)hkv * G * D128 + sub * 8);
    st16((kv ? vcache : kcache) + ((b * Hkv + hkv) * C + s) * D128 + sub * 8, u);
}

template <int G, int U>
inline void dec_launch_d128(const DecPlan& pl, const void* qkv_new, const float* tab, void* kcache, void* vcache,
                            const void* lens, void* out, void* ws, int B, int Hkv, int C, int max_len, float scale,
                            hipStream_t st) {
    attn_decode_d128_k<G, U><<<dim3(pl.nsplit, Hkv, B), DEC_NT, 0, st>>>(
        (const bf16_t*)qkv_new, tab, (bf16_t*)kcache, (bf16_t*)vcache, (const int*)lens, (bf16_t*)out, (float*)ws, Hkv, C,
        max_len, pl.chunk, scale);
    if (pl.nsplit > 1)
        attn_decode_d128_merge_k<<<dim3(Hkv * G, B), D128, 0, st>>>((const float*)ws, (bf16_t*)out, Hkv * G, pl.nsplit);
}

}  // namespace

DDL_API int ddl_attn_decode_gqa_supported(int H, int Hkv);      // attn_decode.hip
DDL_API long ddl_attn_decode_gqa_ws(int B, int H, int Hkv, int max_len);

// 1 when the rotary decode kernel has an instance for this group size at head dim D (64 or 128)
DDL_API int ddl_attn_decode_gqa_supported_hd(int H, int Hkv, int D) {
    if (D == 64) return ddl_attn_decode_gqa_supported(H, Hkv);
    return D == D128 && gqa_group_ok(H, Hkv) ? 1 : 0;
}

// floats of workspace the launch needs at head dim D (0 with one split); the split plan itself does not depend
// on D: ddl_attn_decode_gqa_nsplit / _chunk answer for both
DDL_API long ddl_attn_decode_gqa_ws_hd(int B, int H, int Hkv, int max_len, int D) {
    if (D == 64) return ddl_attn_decode_gqa_ws(B, H, Hkv, max_len);
    if (D != D128) return -1;
    const int ns = dec_plan(B, Hkv, std::max(1, max_len), DEC_MAX_SPLIT_GQA).nsplit;
    return ns == 1 ? 0 : (long)B * H * ns * (2 + D128);
}

DDL_API int ddl_attn_decode_gqa_d128(const void* qkv_new, const float* tab, void* kcache, void* vcache, const void* lens,
                                     void* out, void* ws, int B, int H, int Hkv, int C, int max_len, long n_pos,
                                     float scale, hipStream_t st) {
    if (!gqa_group_ok(H, Hkv)) return (int)hipErrorInvalidValue;
    if (B <= 0) return 0;
    if (max_len < 1 || max_len > C || max_len > n_pos || H > 65535 || B > 65535) return (int)hipErrorInvalidValue;
    const DecPlan pl = dec_plan(B, Hkv, max_len, DEC_MAX_SPLIT_GQA);
    if (pl.nsplit > 1 && !ws) return (int)hipErrorInvalidValue;
#define DEC_LAUNCH(G_, U_) \
    dec_launch_d128<G_, U_>(pl, qkv_new, tab, kcache, vcache, lens, out, ws, B, Hkv, C, max_len, scale, st)
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

DDL_API int ddl_kv_cache_fill_gqa_d128(const void* packed, void* kcache, void* vcache, int B, int S, int H, int Hkv,
                                       int C, hipStream_t st) {
    if (Hkv < 1 || H < Hkv || H % Hkv) return (int)hipErrorInvalidValue;
    if (B <= 0 || S <= 0) return 0;
    if (S > C) return (int)hipErrorInvalidValue;
    const long total = (long)B * S * 2 * Hkv * 16;
    kv_cache_fill_d128_k<<<(unsigned)((total + 255) / 256), 256, 0, st>>>((const bf16_t*)packed, (bf16_t*)kcache,
                                                                         (bf16_t*)vcache, S, Hkv, H / Hkv, C, total);
    DDL_RETURN_LAUNCH();
}
