// Rotary grouped-query single-query (decode) attention at HEAD DIM 128 over an FP8 KV CACHE, with the new
// token's rotation, quantisation and append, and the cache fill that quantises a prefill.  The contract is
// attn_decode_d128.hip's (qkv_new, the rotary table, lens / max_len, the dead-row rule, the split plan and the
// workspace layout) with this cache format:
//
// Cache: per layer kcache / vcache [B, Hkv, C, 128], one byte per element (OCP e4m3, torch.float8_e4m3fn's
// bits), and kscale / vscale [B, Hkv, C] fp32: element (b, h, j, i) is value(byte) * scale[b, h, j].  A row is
// quantised as ops.quantize_fp8_rows defines it: scale = amax / 448 (1.0 for an all-zero row), byte =
// e4m3_rne(clamp(x / scale, -448, 448)), the division a true fp32 one.  Keys are quantised after the rotation
// and its one rounding to bf16, values from the bf16 projection.  The attention sees the DEQUANTISED row also
// for the token being appended, so every later step sees a key exactly as the step that wrote it did:
//   s_j = (q . kbytes_j) * kscale[j] / sqrt(128),   out = sum_j p_j vscale[j] vbytes_j / sum_j p_j.
//
// Layout.  The per-lane state is the bf16 kernel's: 16 lanes -- one DPP row -- own a key, each lane 8 head-dim
// elements (q[G][8], acc[G][8], m[G], l[G]); the score's 16-lane sum is row16_sum; the 16 group states merge
// through LDS in group order.  What changes is the stream:
//   - a lane's piece of a row is 8 bytes: one 8-byte load.  To keep the bf16 kernel's bytes in flight a group
//     takes U = 8 keys per round (4 at G = 8): ku / vu cost the same 32 (16) VGPRs and a round is 128 (64)
//     keys = 32 (16) KB of rows per workgroup.  A split's chunk is a multiple of 32 keys, not of a round: the
//     last round of a split is cut by the j < end selects.
//   - the two scales of a key are one fp32 each, read by all 16 lanes of the group from the same address (one
//     request per row of lanes); they are 3 % of the row bytes.
//   - e4m3 -> fp32 is v_cvt_pk_f32_fp8, exact, four per 8 bytes (cheaper than the bf16 unpack).  kscale[j]
//     multiplies the finished 16-lane score sum once per (key, head); vscale[j] is folded into p before the
//     accumulation.  No element is ever multiplied by a scale, and the scaled-convert forms are not used.
//   - append: the 16 lanes that own position n rotate the new key as the bf16 kernel does, take the row's amax
//     (8 elements per lane, then row16_max: row16_sum's four DPP steps with max), form scale = amax / 448,
//     divide, clamp and convert with v_cvt_pk_fp8_f32 (round to nearest even, subnormals kept), store 8 bytes
//     each and lane 0 the scale, and go on with those bytes and that scale like any cached row.  The value row
//     likewise.  All 16 lanes of a group take the j == n branch together, so the DPP reads stay inside active
//     lanes.
//
// Split-KV: grid (nsplit, Hkv, B) from dec_plan(B, Hkv, max_len) -- host values only -- partials to ws
// ([B H nsplit] x (m, l) then x 128 fp32), merged in split order by a second launch.  No atomics, no scratch;
// bitwise repeatable.  Positions past n are never loaded, bytes or scales, and selects, not multiplies, keep
// them out.
#include "attn_decode.h"

namespace {

constexpr int D128 = 128;
constexpr int F8_GRPS = DEC_NT / 16;        // key groups per workgroup: 16 lanes (a DPP row) per key
constexpr float E4M3_MAX = 448.f;
static_assert(DEC_PLAN_ALIGN % F8_GRPS == 0, "a split's chunk must be whole rows of groups");

typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint2 ld8(const uint8_t* p) { return *reinterpret_cast<const uint2*>(p); }
__device__ __forceinline__ void st8(uint8_t* p, const uint2& u) { *reinterpret_cast<uint2*>(p) = u; }

// 8 e4m3 bytes -> 8 floats, exactly
__device__ __forceinline__ void dec8(const uint2& u, float* v) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(u.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(u.x, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8(u.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8(u.y, true);
    v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
    v[4] = c[0]; v[5] = c[1]; v[6] = d[0]; v[7] = d[1];
}

// Max over the 16 lanes of a DPP row (every lane of the row gets it): row16_sum's four steps.
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

// This lane's 8 elements x of a 128-wide row held by the 16 lanes of a DPP row -> its 8 bytes and the row's
// scale (the same bits in every lane): ops.quantize_fp8_rows on that row.
__device__ __forceinline__ uint2 quant_row8(const float* x, float& sc) {
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

// attn_decode_d128.hip's rotation: this lane's 8 columns (sub * 8 ..) of one head rotated by (c, sn), the
// table's entries for columns 8 (sub & 7) .. of the low half; rope_qkv_fwd_k's expressions, operand order
// included.  Lanes 0-7 of a group own the low half, lanes 8-15 the high one.
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

// (two waves per SIMD asked for: G = 8 allocates 257 VGPRs without the bound and 255, still with no scratch,
// with it; the other instances sit under 256 either way, at 141 (G = 1) to 187 (G = 4): fewer waves per SIMD than
// the bf16 kernel's 115 to 163 allow, at a cost nobody has measured)
template <int G, int U>
__global__ __launch_bounds__(DEC_NT, 2) void attn_decode_d128_fp8_k(
    const bf16_t* __restrict__ qkv_new, const float* __restrict__ tab, uint8_t* __restrict__ kcache,
    uint8_t* __restrict__ vcache, float* __restrict__ kscale, float* __restrict__ vscale, const int* __restrict__ lens,
    bf16_t* __restrict__ out, float* __restrict__ ws, int Hkv, int C, int max_len, int chunk, float scale) {
    constexpr int NH = G < 4 ? G : 4;       // query heads merged through LDS at a time
    __shared__ float s_ml[NH][F8_GRPS][2];
    __shared__ __attribute__((aligned(16))) float s_acc[NH][F8_GRPS][D128];
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
    const long sbase = ((long)b * Hkv + hkv) * C;       // of this head's scales; x 128 + this lane's bytes:
    const long cbase = sbase * D128 + sub * 8;

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
    for (int jb = start; jb < end; jb += F8_GRPS * U) {       // trip count uniform over the workgroup
        const int j0 = jb + grp;
        uint2 ku[U], vu[U];
        float ks[U], vs[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * F8_GRPS;
            ku[u] = make_uint2(0, 0);
            vu[u] = make_uint2(0, 0);
            ks[u] = 0.f;
            vs[u] = 0.f;
            if (j < end) {
                // the new key / value come from the projection, cached rows from the cache; the 16 lanes that
                // own position n quantise and append, and go on with what they stored
                if (j == n) {
                    // (table row n again, through a pointer the optimiser cannot match with the one above: 16
                    // cos / sin values kept live across the loop for this one key cost registers in every round)
                    const float* trow = tab + (long)n * D128 + 8 * (sub & 7);
                    asm volatile("" : "+v"(trow));
                    float ck[8], sk[8], kf[8], vf[8];
                    load8(trow, ck);
                    load8(trow + D128 / 2, sk);
                    unpack8(rotate8_d128(knew, sub, ck, sk), kf);
                    unpack8(ld16(vnew), vf);
                    ku[u] = quant_row8(kf, ks[u]);
                    vu[u] = quant_row8(vf, vs[u]);
                    st8(kcache + cbase + (long)n * D128, ku[u]);
                    st8(vcache + cbase + (long)n * D128, vu[u]);
                    if (sub == 0) {
                        kscale[sbase + n] = ks[u];
                        vscale[sbase + n] = vs[u];
                    }
                } else {
                    ku[u] = ld8(kcache + cbase + (long)j * D128);
                    vu[u] = ld8(vcache + cbase + (long)j * D128);
                    ks[u] = kscale[sbase + j];
                    vs[u] = vscale[sbase + j];
                }
            }
        }
        // (every lane of the wave is active here: the DPP row sum reads its 15 neighbours)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool live = j0 + u * F8_GRPS < end;
            float kf[8], vf[8];
            dec8(ku[u], kf);
            dec8(vu[u], vf);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float d = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) d = __builtin_fmaf(q[g][i], kf[i], d);
                d = row16_sum(d) * ks[u];
                const float s = live ? d : -INFINITY;
                const float mn = fmaxf(m[g], s);
                const float corr = m[g] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m[g] - mn);
                const float p = live ? __builtin_amdgcn_exp2f(s - mn) : 0.f;
                const float pv = p * vs[u];
                l[g] = __builtin_fmaf(l[g], corr, p);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[g][i] = __builtin_fmaf(acc[g][i], corr, pv * vf[i]);
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
            for (int g = 0; g < F8_GRPS; ++g) mm = fmaxf(mm, s_ml[hh][g][0]);
            float ll = 0.f, o0 = 0.f, o1 = 0.f;
#pragma unroll
            for (int g = 0; g < F8_GRPS; ++g) {
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

// out[b, h, :] from the nsplit partials, in split order; one 128-thread workgroup per (b, h).  (The bf16
// kernel's merge, kept as a copy: sharing it through the header would change how that file is compiled.)
__global__ __launch_bounds__(D128) void attn_decode_d128_fp8_merge_k(const float* __restrict__ ws, bf16_t* __restrict__ out,
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

// Slot hkv G of the K and V thirds of rope_qkv's packed [B, S, 3, Hkv G, 128] -> positions 0 .. S-1 of the two
// byte caches and the two scale tensors.  One DPP row per (token, K | V, KV head) row: a 16-byte bf16 load per
// lane, the row's amax and scale, 8 bytes out; lane 0 of the row stores the scale.  (total is a multiple of
// 16: a row of lanes is inside or outside as a whole.)
__global__ __launch_bounds__(256) void kv_cache_fill_d128_fp8_k(const bf16_t* __restrict__ packed, uint8_t* __restrict__ kcache,
                                                                uint8_t* __restrict__ vcache, float* __restrict__ kscale,
                                                                float* __restrict__ vscale, int S, int Hkv, int G, int C,
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
    float x[8], sc;
    unpack8(ld16(packed + (b * S + s) * 3 * HD + (1 + kv) * HD + (long)hkv * G * D128 + sub * 8), x);
    const uint2 u = quant_row8(x, sc);
    const long pos = (b * Hkv + hkv) * C + s;
    st8((kv ? vcache : kcache) + pos * D128 + sub * 8, u);
    if (sub == 0) (kv ? vscale : kscale)[pos] = sc;
}

template <int G, int U>
inline void dec_launch_d128_fp8(const DecPlan& pl, const void* qkv_new, const float* tab, void* kcache, void* vcache,
                                void* kscale, void* vscale, const void* lens, void* out, void* ws, int B, int Hkv, int C,
                                int max_len, float scale, hipStream_t st) {
    attn_decode_d128_fp8_k<G, U><<<dim3(pl.nsplit, Hkv, B), DEC_NT, 0, st>>>(
        (const bf16_t*)qkv_new, tab, (uint8_t*)kcache, (uint8_t*)vcache, (float*)kscale, (float*)vscale, (const int*)lens,
        (bf16_t*)out, (float*)ws, Hkv, C, max_len, pl.chunk, scale);
    if (pl.nsplit > 1)
        attn_decode_d128_fp8_merge_k<<<dim3(Hkv * G, B), D128, 0, st>>>((const float*)ws, (bf16_t*)out, Hkv * G,
                                                                       pl.nsplit);
}

}  // namespace

// 1 when the FP8-cache decode kernel and fill have an instance for this group size at head dim D (128 only)
DDL_API int ddl_attn_decode_gqa_d128_fp8_supported(int H, int Hkv, int D) {
    return D == D128 && gqa_group_ok(H, Hkv) ? 1 : 0;
}

// kcache / vcache: e4m3 bytes [B, Hkv, C, 128]; kscale / vscale: fp32 [B, Hkv, C]; ws: the floats
// ddl_attn_decode_gqa_ws_hd(B, H, Hkv, max_len, 128) asks for (the plan and the partials are the bf16 kernel's)
DDL_API int ddl_attn_decode_gqa_d128_fp8(const void* qkv_new, const float* tab, void* kcache, void* vcache, void* kscale,
                                         void* vscale, const void* lens, void* out, void* ws, int B, int H, int Hkv,
                                         int C, int max_len, long n_pos, float scale, hipStream_t st) {
    if (!gqa_group_ok(H, Hkv)) return (int)hipErrorInvalidValue;
    if (B <= 0) return 0;
    if (max_len < 1 || max_len > C || max_len > n_pos || H > 65535 || B > 65535) return (int)hipErrorInvalidValue;
    const DecPlan pl = dec_plan(B, Hkv, max_len, DEC_MAX_SPLIT_GQA);
    if (pl.nsplit > 1 && !ws) return (int)hipErrorInvalidValue;
#define DEC_LAUNCH(G_, U_)                                                                                          \
    dec_launch_d128_fp8<G_, U_>(pl, qkv_new, tab, kcache, vcache, kscale, vscale, lens, out, ws, B, Hkv, C, max_len, \
                                scale, st)
    switch (H / Hkv) {
        case 1: DEC_LAUNCH(1, 8); break;
        case 2: DEC_LAUNCH(2, 8); break;
        case 3: DEC_LAUNCH(3, 8); break;
        case 4: DEC_LAUNCH(4, 8); break;
        default: DEC_LAUNCH(8, 4); break;
    }
#undef DEC_LAUNCH
    DDL_RETURN_LAUNCH();
}

DDL_API int ddl_kv_cache_fill_gqa_d128_fp8(const void* packed, void* kcache, void* vcache, void* kscale, void* vscale,
                                           int B, int S, int H, int Hkv, int C, hipStream_t st) {
    if (Hkv < 1 || H < Hkv || H % Hkv) return (int)hipErrorInvalidValue;
    if (B <= 0 || S <= 0) return 0;
    if (S > C) return (int)hipErrorInvalidValue;
    const long total = (long)B * S * 2 * Hkv * 16;
    kv_cache_fill_d128_fp8_k<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(
        (const bf16_t*)packed, (uint8_t*)kcache, (uint8_t*)vcache, (float*)kscale, (float*)vscale, S, Hkv, H / Hkv, C,
        total);
    DDL_RETURN_LAUNCH();
}
