// What the decode-attention kernels of every head dimension share (attn_decode.hip: head dim 64;
// attn_decode_d128.hip: head dim 128): the host-only split plan, the 16-byte bf16 piece helpers and the
// group sizes the rotary kernels are built for.
#pragma once
#include "ddl_common.h"

namespace {

constexpr int DEC_NT = 256;                 // threads per workgroup
constexpr int DEC_PLAN_ALIGN = 32;          // a split's chunk is a multiple of this (and so of every kernel's group count)
constexpr int DEC_MAX_SPLIT = 16;           // ddl_attn_decode
constexpr int DEC_MAX_SPLIT_GQA = 32;       // ddl_attn_decode_gqa, ddl_attn_decode_gqa_d128
constexpr int DEC_MIN_CHUNK = 64;           // positions per split, at least (and a multiple of DEC_PLAN_ALIGN)
constexpr float LOG2E = 1.4426950408889634f;

struct DecPlan {
    int nsplit, chunk;
};

// From max_len alone: enough splits (max_split at most) that B Hkv nsplit covers the chip, each at least
// DEC_MIN_CHUNK positions, chunk a multiple of DEC_PLAN_ALIGN.
inline DecPlan dec_plan(int B, int Hkv, int max_len, int max_split) {
    const int bh = std::max(1, B * Hkv);
    int want = std::min(max_split, (num_cus() + bh - 1) / bh);
    want = std::max(1, std::min(want, (max_len + DEC_MIN_CHUNK - 1) / DEC_MIN_CHUNK));
    int chunk = (max_len + want - 1) / want;
    chunk = (chunk + DEC_PLAN_ALIGN - 1) / DEC_PLAN_ALIGN * DEC_PLAN_ALIGN;
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

// the group sizes G = H / Hkv the rotary kernels have instances for
inline bool gqa_group_ok(int H, int Hkv) {
    if (Hkv < 1 || H < Hkv || H % Hkv) return false;
    const int G = H / Hkv;
    return G == 1 || G == 2 || G == 3 || G == 4 || G == 8;
}

}  // namespace
