// Single-query (decode) attention over a key/value cache, and the cache fill after a prefill.
// Head dim 64, bf16, one query row per KV head (MHA).
//
// Cache: per layer kcache / vcache [B, H, C, 64] bf16 (a head's keys are contiguous 128-byte rows),
// lens [B] int32 on the device.  For batch row b with n = lens[b] the query (the q third of the new
// token's packed [B, 3 H 64] projection) attends to cached keys 0 .. n-1 and to the new key, which is
// read from qkv_new, never from the cache; the lane group that owns position n also stores the new
// K / V rows to cache[b, h, n] (plain 16-byte vector stores).  No workgroup reads a row another one
// writes in the same launch, and lens is not modified (all layers of a step share it).
//
// Memory / latency bound, so VALU, no MFMA, no LDS staging of K / V: a key row is 8 x 16 bytes, 8
// lanes (one "group") own a key, each lane the 8 head-dim elements of its 16-byte piece for both the
// score (8 FMAs + a 3-step reduce over the group) and the P V accumulation.  A 256-thread workgroup
// is 32 groups; each takes DEC_U keys per round (2 DEC_U 16-byte loads in flight per lane) and keeps
// its own online softmax (m, l, acc[8]); the 32 group states merge through LDS in group order.
//
// Split-KV: grid (nsplit, H, B); split s covers positions [s chunk, (s+1) chunk), clipped to n+1.
// nsplit and chunk come from max_len (the host's upper bound on n+1) alone, so the grid never
// depends on device data.  A split whose range is empty writes an empty partial (m = -inf, l = 0)
// and touches no cache row.  Partials go to ws ([B H nsplit] x (m, l) then x 64 fp32) and a second
// launch merges them in split order: no float atomics, no in-launch hand-off; nsplit = 1 writes out
// directly.  Positions past n are never loaded (selects, not multiplies, keep them out), so
// whatever bit patterns the unwritten part of the cache holds cannot reach the output.
#include "ddl_common.h"

namespace {

constexpr int DEC_D = 64;
constexpr int DEC_NT = 256;                 // threads per workgroup
constexpr int DEC_G = DEC_NT / 8;           // key groups per workgroup
constexpr int DEC_U = 4;                    // keys per group per round
constexpr int DEC_MAX_SPLIT = 16;
constexpr int DEC_MIN_CHUNK = 64;           // positions per split, at least (and a multiple of DEC_G)
constexpr float LOG2E = 1.4426950408889634f;

struct DecPlan {
    int nsplit, chunk;
};

// From max_len alone: enough splits that B H nsplit covers the chip, each at least DEC_MIN_CHUNK
// positions, chunk a multiple of DEC_G.
inline DecPlan dec_plan(int B, int H, int max_len) {
    const int bh = std::max(1, B * H);
    int want = std::min(DEC_MAX_SPLIT, (num_cus() + bh - 1) / bh);
    want = std::max(1, std::min(want, (max_len + DEC_MIN_CHUNK - 1) / DEC_MIN_CHUNK));
    int chunk = (max_len + want - 1) / want;
    chunk = (chunk + DEC_G - 1) / DEC_G * DEC_G;
    return {(max_len + chunk - 1) / chunk, chunk};
}

__device__ __forceinline__ void unpack8(const uint4& u, float* v) {
    v[0] = lo_f(u.x); v[1] = hi_f(u.x); v[2] = lo_f(u.y); v[3] = hi_f(u.y);
    v[4] = lo_f(u.z); v[5] = hi_f(u.z); v[6] = lo_f(u.w); v[7] = hi_f(u.w);
}

// sum over the 8 lanes of a group (lanes 8 g .. 8 g + 7): xor 1, 2 inside the quad, then xor 4
__device__ __forceinline__ float group8_sum(float v) {
    v = dpp_add<0xB1>(v);
    v = dpp_add<0x4E>(v);
    return v + __shfl_xor(v, 4, 64);
}

__global__ __launch_bounds__(DEC_NT) void attn_decode_k(const bf16_t* __restrict__ qkv_new, bf16_t* __restrict__ kcache,
                                                        bf16_t* __restrict__ vcache, const int* __restrict__ lens,
                                                        bf16_t* __restrict__ out, float* __restrict__ ws, int H, int C,
                                                        int max_len, int chunk, float scale) {
    __shared__ float s_ml[DEC_G][2];
    __shared__ float s_acc[DEC_G][DEC_D];
    const int split = blockIdx.x, nsplit = gridDim.x, h = blockIdx.y, b = blockIdx.z, B = gridDim.z;
    const int tid = threadIdx.x, grp = tid >> 3, sub = tid & 7;
    // lens beyond the host's bound would index past the cache: clamp (the result is then the
    // caller's problem, the stores stay inside the cache)
    const int n = std::min(std::max(lens[b], 0), max_len - 1);
    const int start = split * chunk, end = std::min(start + chunk, n + 1);

    const long HD = (long)H * DEC_D;
    const bf16_t* qrow = qkv_new + (long)b * 3 * HD + (long)h * DEC_D + sub * 8;
    const bf16_t* kbase = kcache + ((long)b * H + h) * C * DEC_D + sub * 8;
    const bf16_t* vbase = vcache + ((long)b * H + h) * C * DEC_D + sub * 8;

    float q[8];
    load8(qrow, q);
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] *= scale * LOG2E;      // scores in the exp2 domain

    float m = -INFINITY, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int jb = start; jb < end; jb += DEC_G * DEC_U) {     // trip count uniform over the workgroup
        const int j0 = jb + grp;
        uint4 ku[DEC_U], vu[DEC_U];
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const int j = j0 + u * DEC_G;
            ku[u] = make_uint4(0, 0, 0, 0);
            vu[u] = make_uint4(0, 0, 0, 0);
            if (j < end) {
                // the new key / value come from the projection; cached rows from the cache
                const bf16_t* kp = j == n ? qrow + HD : kbase + (long)j * DEC_D;
                const bf16_t* vp = j == n ? qrow + 2 * HD : vbase + (long)j * DEC_D;
                ku[u] = *reinterpret_cast<const uint4*>(kp);
                vu[u] = *reinterpret_cast<const uint4*>(vp);
                if (j == n) {       // append: this group owns position n
                    *reinterpret_cast<uint4*>(kcache + ((long)b * H + h) * C * DEC_D + (long)n * DEC_D + sub * 8) = ku[u];
                    *reinterpret_cast<uint4*>(vcache + ((long)b * H + h) * C * DEC_D + (long)n * DEC_D + sub * 8) = vu[u];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const bool live = j0 + u * DEC_G < end;
            float kf[8], vf[8];
            unpack8(ku[u], kf);
            unpack8(vu[u], vf);
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) d = __builtin_fmaf(q[i], kf[i], d);
            d = group8_sum(d);
            const float s = live ? d : -INFINITY;
            const float mn = fmaxf(m, s);
            const float corr = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - mn);
            const float p = live ? __builtin_amdgcn_exp2f(s - mn) : 0.f;
            l = __builtin_fmaf(l, corr, p);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(acc[i], corr, p * vf[i]);
            m = mn;
        }
    }

    // merge the 32 group states in group order
    if (sub == 0) {
        s_ml[grp][0] = m;
        s_ml[grp][1] = l;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) s_acc[grp][sub * 8 + i] = acc[i];
    __syncthreads();
    if (tid < DEC_D) {
        float mm = -INFINITY;
#pragma unroll 8
        for (int g = 0; g < DEC_G; ++g) mm = fmaxf(mm, s_ml[g][0]);
        float ll = 0.f, o = 0.f;
#pragma unroll 8
        for (int g = 0; g < DEC_G; ++g) {
            const float mg = s_ml[g][0];
            const float w = mg == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mg - mm);
            ll = __builtin_fmaf(s_ml[g][1], w, ll);
            o = __builtin_fmaf(s_acc[g][tid], w, o);
        }
        if (nsplit == 1) {
            out[(long)b * HD + (long)h * DEC_D + tid] = f2bf(o / ll);     // ll >= 1: the new key is live
        } else {
            const long pi = ((long)b * H + h) * nsplit + split;
            float* ws_ml = ws;
            float* ws_acc = ws + (long)B * H * nsplit * 2;
            if (tid == 0) {
                ws_ml[pi * 2] = mm;
                ws_ml[pi * 2 + 1] = ll;
            }
            ws_acc[pi * DEC_D + tid] = o;
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

// K and V thirds of the packed [B, S, 3 H 64] projection -> cache positions 0 .. S-1; one thread per
// 16 bytes
__global__ __launch_bounds__(256) void kv_cache_fill_k(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kcache,
                                                       bf16_t* __restrict__ vcache, int S, int H, int C, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int sub = (int)(i & 7);
    long r = i >> 3;
    const int h = (int)(r % H);
    r /= H;
    const int kv = (int)(r & 1);
    r >>= 1;
    const int s = (int)(r % S);
    const long b = r / S;
    const long HD = (long)H * DEC_D;
    const uint4 u = *reinterpret_cast<const uint4*>(qkv + (b * S + s) * 3 * HD + (1 + kv) * HD + (long)h * DEC_D + sub * 8);
    bf16_t* dst = (kv ? vcache : kcache) + ((b * H + h) * C + s) * DEC_D + sub * 8;
    *reinterpret_cast<uint4*>(dst) = u;
}

}  // namespace

// number of key splits for this (B, H, max_len): what the launch will use
DDL_API int ddl_attn_decode_nsplit(int B, int H, int max_len) { return dec_plan(B, H, std::max(1, max_len)).nsplit; }
// positions per split
DDL_API int ddl_attn_decode_chunk(int B, int H, int max_len) { return dec_plan(B, H, std::max(1, max_len)).chunk; }
// floats of workspace the launch needs (0 with one split)
DDL_API long ddl_attn_decode_ws(int B, int H, int max_len) {
    const int ns = dec_plan(B, H, std::max(1, max_len)).nsplit;
    return ns == 1 ? 0 : (long)B * H * ns * (2 + DEC_D);
}

DDL_API int ddl_attn_decode(const void* qkv_new, void* kcache, void* vcache, const void* lens, void* out, void* ws, int B,
                            int H, int C, int max_len, float scale, hipStream_t st) {
    if (B <= 0 || H <= 0) return 0;
    if (max_len < 1 || max_len > C || H > 65535 || B > 65535) return (int)hipErrorInvalidValue;
    const DecPlan pl = dec_plan(B, H, max_len);
    if (pl.nsplit > 1 && !ws) return (int)hipErrorInvalidValue;
    attn_decode_k<<<dim3(pl.nsplit, H, B), DEC_NT, 0, st>>>((const bf16_t*)qkv_new, (bf16_t*)kcache, (bf16_t*)vcache,
                                                           (const int*)lens, (bf16_t*)out, (float*)ws, H, C, max_len,
                                                           pl.chunk, scale);
    if (pl.nsplit > 1)
        attn_decode_merge_k<<<dim3(H, B), DEC_D, 0, st>>>((const float*)ws, (bf16_t*)out, H, pl.nsplit);
    DDL_RETURN_LAUNCH();
}

DDL_API int ddl_kv_cache_fill(const void* qkv, void* kcache, void* vcache, int B, int S, int H, int C, hipStream_t st) {
    if (B <= 0 || S <= 0 || H <= 0) return 0;
    if (S > C) return (int)hipErrorInvalidValue;
    const long total = (long)B * S * 2 * H * 8;
    kv_cache_fill_k<<<(unsigned)((total + 255) / 256), 256, 0, st>>>((const bf16_t*)qkv, (bf16_t*)kcache, (bf16_t*)vcache, S,
                                                                    H, C, total);
    DDL_RETURN_LAUNCH();
}
