// The glue of a GPT-2 decode step, so that a step launches nothing but the project's own kernels and has
// no host-side state (what lets the step be captured once into a hipGraph and replayed):
//
//   ddl_decode_embed   h[b, :] = wte[tok[b], :] + wpe[lens[b], :]          (bf16 rows, fp32 add, one rounding)
//   ddl_next_token     logits [B, V] bf16 -> one token per row (argmax, or temperature / top-k sampling from
//                      a given uniform number), the eos / pad rule, and the advance of the step's device
//                      state (token fed to the next step, output column, step counter, cache lengths).
//   ddl_next_token_ex  the same with a repetition penalty, top-p and min-p: next_token_ex_k, further down.
//
// ddl_next_token: one 1024-thread workgroup per row.  The row is read from memory once, as 16-byte pieces,
// into LDS as ordered 16-bit keys (key order == value order, so the k-th largest VALUE is the k-th largest
// KEY and a 16-step bisection on the key with a block-wide count finds it exactly, without a sort); a row
// too long for the CU's LDS is re-read from memory (L2) by every pass instead -- same code, other loader.
// Rows of an odd V are only 2-byte aligned: the row is laid out in "slots" p = off + i (off = the row's
// element offset within its 16-byte line), so that 16-byte pieces of memory are 16-byte pieces of slots;
// thread t owns the R consecutive slots [t R, (t + 1) R) (R % 8 == 0), i.e. a run of consecutive columns.
//
// Sampling, for u in [0, 1): kept = every column whose logit >= the k-th largest value (ties at the k-th
// value all kept); w_j = exp((x_j - max) * inv_temperature) in fp32; the token is the lowest kept j whose
// inclusive prefix sum of w in index order exceeds u * W (W: the total), or the last kept j if rounding
// leaves none.  The prefix sums are a serial sum over the thread's run (<= R terms) on top of a tree over
// the threads (6 shuffle levels in the wave, <= 15 wave totals): about R + 21 roundings, not V.
// No atomics: every word written is owned by one workgroup (row b: tok_out[b], tokens_out[b, :], done[b],
// step[b], lens[b]) and written by its thread 0 with plain stores.  The step counter is per row for that
// reason: a single counter incremented by workgroup 0 could be read by a workgroup that starts later.
#include "ddl_common.h"

namespace {

constexpr int NT_THREADS = 1024;
constexpr int NT_WAVES = NT_THREADS / 64;
constexpr int NT_MAX_LDS = 160 * 1024 - 2048;       // dynamic LDS for the row; the rest: the reduction arrays

// params (int32 [5], on the device so that one captured launch serves any setting):
//   [0] inv_temperature (fp32 bits)  [1] top_k (<= 0 or >= V: keep all)  [2] eos (< 0: none)  [3] pad
//   [4] 0: greedy even when u is given
constexpr int PRM_INVT = 0, PRM_TOPK = 1, PRM_EOS = 2, PRM_PAD = 3, PRM_SAMPLE = 4;

// bf16 bits -> 16-bit key with the values' order (-0 counts as +0, as in a float compare)
__device__ __forceinline__ uint32_t bf_key(uint32_t h) {
    if (h == 0x8000u) h = 0;
    return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}
__device__ __forceinline__ float key_val(uint32_t k) {
    const uint32_t h = (k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xffffu);
    return __uint_as_float(h << 16);
}

// The row as slots: lo <= p < hi are columns p - lo; `base` is the 16-byte aligned address of slot 0.
template <bool LDS_ROW>
struct Row {
    const bf16_t* base;
    const uint16_t* lds;
    int lo, hi;
    // the raw bf16 of slots p0 .. p0 + 7 (p0 % 8 == 0) from memory; slots outside the row read as 0
    __device__ __forceinline__ uint4 raw(int p0) const {
        if (p0 >= lo && p0 + 8 <= hi) return *reinterpret_cast<const uint4*>(base + p0);
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int p = p0 + e;
            if (p >= lo && p < hi) w[e >> 1] |= (uint32_t)base[p] << (16 * (e & 1));
        }
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
    __device__ __forceinline__ static uint4 to_keys(uint4 r) {
        uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = bf_key(w[i] & 0xffffu) | (bf_key(w[i] >> 16) << 16);
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
    // the keys of slots p0 .. p0 + 7
    __device__ __forceinline__ uint4 keys(int p0) const {
        if (LDS_ROW) return *reinterpret_cast<const uint4*>(lds + p0);
        return to_keys(raw(p0));
    }
};

__device__ __forceinline__ uint32_t key_of(const uint4& k, int e) {
    const uint32_t w = e < 2 ? k.x : e < 4 ? k.y : e < 6 ? k.z : k.w;
    return (w >> (16 * (e & 1))) & 0xffffu;
}

// FOR_RUN(body): every slot p of this thread's run that is a column of the row, in index order, with `key`
#define FOR_RUN(BODY)                                                       \
    for (int p0_ = p_first; p0_ < p_last; p0_ += 8) {                       \
        if (p0_ + 8 <= row.lo) continue;                                    \
        const uint4 k8_ = row.keys(p0_);                                    \
        _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) {                  \
            const int p = p0_ + e_;                                         \
            const uint32_t key = key_of(k8_, e_);                           \
            if (p >= row.lo && p < row.hi) { BODY }                         \
        }                                                                   \
    }

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool LDS_ROW>
__global__ __launch_bounds__(NT_THREADS) void next_token_k(const bf16_t* __restrict__ logits, int V, int R,
                                                           const float* __restrict__ u, int Tu,
                                                           const int* __restrict__ params, int* step, uint8_t* done,
                                                           int64_t* tok_out, int64_t* tokens_out, int To, int* lens) {
    extern __shared__ uint4 row_lds[];
    __shared__ uint32_t red_hi[NT_WAVES], red_lo[NT_WAVES];
    __shared__ int red_cnt[2][NT_WAVES], red_min[NT_WAVES], red_max[NT_WAVES];
    __shared__ float red_w[NT_WAVES];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int step0 = step ? step[b] : 0;       // read once, before anything of this row is written
    const bf16_t* rowp = logits + (long)b * V;
    Row<LDS_ROW> row;
    row.lo = (int)((reinterpret_cast<uintptr_t>(rowp) >> 1) & 7);
    row.hi = row.lo + V;
    row.base = rowp - row.lo;
    row.lds = reinterpret_cast<const uint16_t*>(row_lds);
    const int p_first = tid * R, p_last = std::min(p_first + R, row.hi);

    // ---- pass 1: the row into LDS as keys; the maximum, ties to the lowest slot.
    // (key + 1, 0x7fffffff - p) ordered lexicographically; (0, 0) = nothing seen
    uint32_t bk = 0, bp = 0;
    for (int p0 = p_first; p0 < p_last; p0 += 8) {
        if (p0 + 8 <= row.lo) continue;
        const uint4 k8 = Row<LDS_ROW>::to_keys(row.raw(p0));
        if (LDS_ROW) row_lds[p0 >> 3] = k8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int p = p0 + e;
            const uint32_t key = key_of(k8, e) + 1;
            if (p >= row.lo && p < row.hi && key > bk) { bk = key; bp = 0x7fffffffu - (uint32_t)p; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t ok = __shfl_xor(bk, o, 64), op = __shfl_xor(bp, o, 64);
        if (ok > bk || (ok == bk && op > bp)) { bk = ok; bp = op; }
    }
    if (lane == 0) { red_hi[wave] = bk; red_lo[wave] = bp; }
    __syncthreads();        // also: the row's keys are in LDS
#pragma unroll
    for (int w = 0; w < NT_WAVES; ++w) {
        const uint32_t ok = red_hi[w], op = red_lo[w];
        if (ok > bk || (ok == bk && op > bp)) { bk = ok; bp = op; }
    }
    int pick = (int)(0x7fffffffu - bp);         // the argmax slot

    const bool sample = u != nullptr && (params == nullptr || params[PRM_SAMPLE] != 0);
    if (sample) {
        const float inv_t = params ? __int_as_float(params[PRM_INVT]) : 1.f;
        const int top_k = params ? params[PRM_TOPK] : 0;
        const float xmax = key_val(bk - 1);

        // ---- the k-th largest key: the largest T with count(key >= T) >= k
        uint32_t thr = 0;
        if (top_k > 0 && top_k < V) {
            for (int bit = 15; bit >= 0; --bit) {
                const uint32_t cand = thr | (1u << bit);
                int c = 0;
                FOR_RUN(c += key >= cand ? 1 : 0;)
                c = wave_sum_i(c);
                int* rc = red_cnt[bit & 1];     // two buffers: one barrier per step
                if (lane == 0) rc[wave] = c;
                __syncthreads();
                int tot = 0;
#pragma unroll
                for (int w = 0; w < NT_WAVES; ++w) tot += rc[w];
                if (tot >= top_k) thr = cand;
            }
        }

        // ---- weights: this thread's run, then an exclusive scan over the threads
        float mine = 0.f;
        FOR_RUN(if (key >= thr) mine += __expf((key_val(key) - xmax) * inv_t);)
        float incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0.f;
        if (lane == 63) red_w[wave] = incl;
        __syncthreads();
        float before = 0.f, total = 0.f;
#pragma unroll
        for (int w = 0; w < NT_WAVES; ++w) {
            if (w == wave) before = total;
            total += red_w[w];
        }
        const int ui = std::min(std::max(step0, 0), Tu - 1);
        const float target = u[(long)ui * gridDim.x + b] * total;

        // ---- the first kept slot whose inclusive prefix exceeds the target; the last kept slot
        float c = before + excl;
        int first = 0x7fffffff, last = -1;
        FOR_RUN(if (key >= thr) {
            c += __expf((key_val(key) - xmax) * inv_t);
            last = p;
            if (c > target && first == 0x7fffffff) first = p;
        })
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            first = std::min(first, __shfl_xor(first, o, 64));
            last = std::max(last, __shfl_xor(last, o, 64));
        }
        if (lane == 0) { red_min[wave] = first; red_max[wave] = last; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NT_WAVES; ++w) {
            first = std::min(first, red_min[w]);
            last = std::max(last, red_max[w]);
        }
        pick = first != 0x7fffffff ? first : last;
    }

    // ---- the step's bookkeeping: row b's words, plain stores by one thread
    if (tid == 0) {
        int64_t tok = pick - row.lo;
        const int eos = params ? params[PRM_EOS] : -1;
        if (done) {
            uint8_t d = done[b];
            if (d) tok = params ? params[PRM_PAD] : 0;
            if (eos >= 0 && tok == eos) d = 1;
            done[b] = d;
        }
        tok_out[b] = tok;
        if (tokens_out && step0 >= 0 && step0 < To) tokens_out[(long)b * To + step0] = tok;
        if (step) step[b] = step0 + 1;
        if (lens) lens[b] += 1;
    }
}

// ---- next_token_ex_k: next_token_k with a repetition penalty, top-p and min-p.  Its own kernel, so that
// next_token_k's instances compile as they always did; with the three settings off it does what that one does.
// params int32 [8]: the five slots above, then the fp32 bits of
//   [5] top_p (1: off)  [6] min_p (0: off)  [7] repetition_penalty (1: off)
// Order: penalty, (temperature,) top-k, top-p, min-p.  Each of the three filters is "key >= a threshold", so the
// kept set is still one key threshold: the largest of the three.
//   penalty  x_j <- x_j / r (x_j > 0) or x_j * r, in fp32 from the logit in memory, rounded once to bf16, for every
//            column id in history[b, :history_lens[b]] and tokens_out[b, :step[b]]; ids outside [0, V) are
//            skipped.  The new key is stored over the column's key in LDS: a column listed twice gets the same
//            value twice, so the stores need no order.  LDS-resident rows only (the other loader re-reads
//            memory; its caller penalises the logits itself and passes r = 1).
//   top-p    the largest key T with mass(key >= T) >= p W, W and the masses over the top-k set: the 16-step
//            bisection of top-k with a block-wide fp32 sum in place of the count, every sum in one fixed order
//            (the thread's run, a butterfly over the wave, the waves in index order), hence repeatable, and
//            monotone in T because fp32 addition of non-negative terms is.
//   min-p    the smallest key whose value x has (x - max) * inv_t >= log(min_p) in fp32: the predicate is
//            monotone in the key, so every thread bisects it in registers, with no pass over the row.
constexpr int PRM_TOPP = 5, PRM_MINP = 6, PRM_PEN = 7, PRM_EX = 8;

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);     // a + b == b + a: every lane gets the same bits
    return v;
}

template <bool LDS_ROW>
__global__ __launch_bounds__(NT_THREADS) void next_token_ex_k(const bf16_t* __restrict__ logits, int V, int R,
                                                              const float* __restrict__ u, int Tu,
                                                              const int* __restrict__ params, int n_params,
                                                              const int64_t* __restrict__ history, int Lh,
                                                              const int* __restrict__ history_lens, int* step,
                                                              uint8_t* done, int64_t* tok_out, int64_t* tokens_out,
                                                              int To, int* lens) {
    extern __shared__ uint4 row_lds[];
    __shared__ uint32_t red_hi[NT_WAVES], red_lo[NT_WAVES];
    __shared__ int red_cnt[2][NT_WAVES], red_min[NT_WAVES], red_max[NT_WAVES];
    __shared__ float red_w[NT_WAVES], red_m[2][NT_WAVES];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int step0 = step ? step[b] : 0;       // read once, before anything of this row is written
    const bf16_t* rowp = logits + (long)b * V;
    Row<LDS_ROW> row;
    row.lo = (int)((reinterpret_cast<uintptr_t>(rowp) >> 1) & 7);
    row.hi = row.lo + V;
    row.base = rowp - row.lo;
    row.lds = reinterpret_cast<const uint16_t*>(row_lds);
    const int p_first = tid * R, p_last = std::min(p_first + R, row.hi);

    const bool ex = params != nullptr && n_params >= PRM_EX;
    const float top_p = ex ? __int_as_float(params[PRM_TOPP]) : 1.f;
    const float min_p = ex ? __int_as_float(params[PRM_MINP]) : 0.f;
    const float pen = ex ? __int_as_float(params[PRM_PEN]) : 1.f;
    const bool penalise = LDS_ROW && pen != 1.f && pen > 0.f;      // (uniform over the workgroup)

    // ---- pass 1: the row into LDS as keys; the maximum, ties to the lowest slot.
    // (key + 1, 0x7fffffff - p) ordered lexicographically; (0, 0) = nothing seen
    uint32_t bk = 0, bp = 0;
    if (!penalise) {
        for (int p0 = p_first; p0 < p_last; p0 += 8) {
            if (p0 + 8 <= row.lo) continue;
            const uint4 k8 = Row<LDS_ROW>::to_keys(row.raw(p0));
            if (LDS_ROW) row_lds[p0 >> 3] = k8;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int p = p0 + e;
                const uint32_t key = key_of(k8, e) + 1;
                if (p >= row.lo && p < row.hi && key > bk) { bk = key; bp = 0x7fffffffu - (uint32_t)p; }
            }
        }
    } else {
        for (int p0 = p_first; p0 < p_last; p0 += 8) {
            if (p0 + 8 <= row.lo) continue;
            row_lds[p0 >> 3] = Row<LDS_ROW>::to_keys(row.raw(p0));
        }
        __syncthreads();
        // the penalised columns' keys over the row's; then the maximum, from LDS
        uint16_t* keys16 = reinterpret_cast<uint16_t*>(row_lds);
        const int n_h = history ? std::min(std::max(history_lens ? history_lens[b] : Lh, 0), Lh) : 0;
        const int n_g = tokens_out && step ? std::min(std::max(step0, 0), To) : 0;
        for (int i = tid; i < n_h + n_g; i += NT_THREADS) {
            const int64_t id = i < n_h ? history[(long)b * Lh + i] : tokens_out[(long)b * To + (i - n_h)];
            if (id < 0 || id >= V) continue;
            const float x = bf2f(rowp[id]);
            keys16[row.lo + (int)id] = (uint16_t)bf_key(f2bf(x > 0.f ? __fdiv_rn(x, pen) : x * pen));
        }
        __syncthreads();
        FOR_RUN(if (key + 1 > bk) { bk = key + 1; bp = 0x7fffffffu - (uint32_t)p; })
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t ok = __shfl_xor(bk, o, 64), op = __shfl_xor(bp, o, 64);
        if (ok > bk || (ok == bk && op > bp)) { bk = ok; bp = op; }
    }
    if (lane == 0) { red_hi[wave] = bk; red_lo[wave] = bp; }
    __syncthreads();        // also: the row's keys are in LDS
#pragma unroll
    for (int w = 0; w < NT_WAVES; ++w) {
        const uint32_t ok = red_hi[w], op = red_lo[w];
        if (ok > bk || (ok == bk && op > bp)) { bk = ok; bp = op; }
    }
    int pick = (int)(0x7fffffffu - bp);         // the argmax slot

    const bool sample = u != nullptr && (params == nullptr || params[PRM_SAMPLE] != 0);
    if (sample) {
        const float inv_t = params ? __int_as_float(params[PRM_INVT]) : 1.f;
        const int top_k = params ? params[PRM_TOPK] : 0;
        const float xmax = key_val(bk - 1);

        // ---- the k-th largest key: the largest T with count(key >= T) >= k
        uint32_t thr = 0;
        if (top_k > 0 && top_k < V) {
            for (int bit = 15; bit >= 0; --bit) {
                const uint32_t cand = thr | (1u << bit);
                int c = 0;
                FOR_RUN(c += key >= cand ? 1 : 0;)
                c = wave_sum_i(c);
                int* rc = red_cnt[bit & 1];     // two buffers: one barrier per step
                if (lane == 0) rc[wave] = c;
                __syncthreads();
                int tot = 0;
#pragma unroll
                for (int w = 0; w < NT_WAVES; ++w) tot += rc[w];
                if (tot >= top_k) thr = cand;
            }
        }

        // ---- top-p: the largest T with mass(key >= max(T, thr)) >= p W.  Up to T = thr that mass is W itself
        // (the same terms in the same order) and p <= 1, so the search never ends below thr.
        if (top_p < 1.f) {
            float m = 0.f;
            FOR_RUN(if (key >= thr) m += __expf((key_val(key) - xmax) * inv_t);)
            m = wave_sum_f(m);
            if (lane == 0) red_w[wave] = m;
            __syncthreads();
            float need = 0.f;
#pragma unroll
            for (int w = 0; w < NT_WAVES; ++w) need += red_w[w];
            need *= top_p;
            const uint32_t thr_k = thr;
            thr = 0;
            for (int bit = 15; bit >= 0; --bit) {
                const uint32_t cand = thr | (1u << bit);
                const uint32_t lim = std::max(cand, thr_k);
                m = 0.f;
                FOR_RUN(if (key >= lim) m += __expf((key_val(key) - xmax) * inv_t);)
                m = wave_sum_f(m);
                float* rm = red_m[bit & 1];     // two buffers: one barrier per step
                if (lane == 0) rm[wave] = m;
                __syncthreads();
                float tot = 0.f;
#pragma unroll
                for (int w = 0; w < NT_WAVES; ++w) tot += rm[w];
                if (tot >= need) thr = cand;
            }
            thr = std::min(std::max(thr, thr_k), bk - 1);      // (the maximum is kept whatever the sums gave)
        }

        // ---- min-p: the lowest key that passes, found among the keys up to the maximum's (which passes)
        if (min_p > 0.f) {
            const float bound = logf(min_p);
            uint32_t lo = 0, hi = bk - 1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if ((key_val(mid) - xmax) * inv_t >= bound) hi = mid; else lo = mid + 1;
            }
            thr = std::max(thr, lo);
        }

        // ---- weights: this thread's run, then an exclusive scan over the threads
        float mine = 0.f;
        FOR_RUN(if (key >= thr) mine += __expf((key_val(key) - xmax) * inv_t);)
        float incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0.f;
        if (lane == 63) red_w[wave] = incl;
        __syncthreads();
        float before = 0.f, total = 0.f;
#pragma unroll
        for (int w = 0; w < NT_WAVES; ++w) {
            if (w == wave) before = total;
            total += red_w[w];
        }
        const int ui = std::min(std::max(step0, 0), Tu - 1);
        const float target = u[(long)ui * gridDim.x + b] * total;

        // ---- the first kept slot whose inclusive prefix exceeds the target; the last kept slot
        float c = before + excl;
        int first = 0x7fffffff, last = -1;
        FOR_RUN(if (key >= thr) {
            c += __expf((key_val(key) - xmax) * inv_t);
            last = p;
            if (c > target && first == 0x7fffffff) first = p;
        })
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            first = std::min(first, __shfl_xor(first, o, 64));
            last = std::max(last, __shfl_xor(last, o, 64));
        }
        if (lane == 0) { red_min[wave] = first; red_max[wave] = last; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NT_WAVES; ++w) {
            first = std::min(first, red_min[w]);
            last = std::max(last, red_max[w]);
        }
        pick = first != 0x7fffffff ? first : last;
    }

    // ---- the step's bookkeeping: row b's words, plain stores by one thread
    if (tid == 0) {
        int64_t tok = pick - row.lo;
        const int eos = params ? params[PRM_EOS] : -1;
        if (done) {
            uint8_t d = done[b];
            if (d) tok = params ? params[PRM_PAD] : 0;
            if (eos >= 0 && tok == eos) d = 1;
            done[b] = d;
        }
        tok_out[b] = tok;
        if (tokens_out && step0 >= 0 && step0 < To) tokens_out[(long)b * To + step0] = tok;
        if (step) step[b] = step0 + 1;
        if (lens) lens[b] += 1;
    }
}

// slots per thread: the row's V columns and up to 7 slots of alignment over 1024 threads, in 8s
inline int nt_run(int V) { return (((V + 7 + NT_THREADS - 1) / NT_THREADS) + 7) / 8 * 8; }

constexpr int DE_THREADS = 128;

__global__ __launch_bounds__(DE_THREADS) void decode_embed_k(const int64_t* __restrict__ tok, const int* __restrict__ lens,
                                                             const bf16_t* __restrict__ wte, const bf16_t* __restrict__ wpe,
                                                             bf16_t* __restrict__ h, int E, int V, int P) {
    const int b = blockIdx.x;
    // an id outside its table is the caller's bug; it must not become a read outside the table
    const long t = std::min<long>(std::max<long>(tok[b], 0), V - 1);
    const long n = std::min(std::max(lens[b], 0), P - 1);
    for (int c = threadIdx.x * 8; c < E; c += DE_THREADS * 8) {
        float a[8], p[8];
        load8(wte + t * E + c, a);
        load8(wpe + n * E + c, p);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += p[j];
        store8(h + (long)b * E + c, a);
    }
}

}  // namespace

// bytes of LDS the launch keeps the row in; 0: the row is too long and is re-read from memory by every pass
DDL_API long ddl_next_token_lds(int V) {
    const long bytes = (long)NT_THREADS * nt_run(std::max(1, V)) * 2;
    return bytes <= NT_MAX_LDS ? bytes : 0;
}

// logits [B, V] bf16 (contiguous) -> tok_out [B] int64.  u [Tu, B] fp32 (nullable: greedy), read at row
// step[b] (0 without step); params int32 [5] (nullable: greedy / temperature 1 / no top-k / no eos);
// step int32 [B], done uint8 [B], tokens_out int64 [B, To], lens int32 [B]: all nullable.
DDL_API int ddl_next_token(const void* logits, int B, int V, const void* u, int Tu, const void* params, void* step,
                           void* done, void* tok_out, void* tokens_out, int To, void* lens, hipStream_t st) {
    if (B < 1 || V < 1 || V > (1 << 30) || !logits || !tok_out || (u && Tu < 1) || (tokens_out && To < 1))
        return (int)hipErrorInvalidValue;
    const int R = nt_run(V);
    const long bytes = ddl_next_token_lds(V);
    if (bytes) {
        static const bool ok = hipFuncSetAttribute((const void*)next_token_k<true>,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, NT_MAX_LDS) == hipSuccess;
        if (!ok) return (int)hipErrorInvalidValue;
        next_token_k<true><<<B, NT_THREADS, (size_t)bytes, st>>>((const bf16_t*)logits, V, R, (const float*)u, Tu,
                                                                 (const int*)params, (int*)step, (uint8_t*)done,
                                                                 (int64_t*)tok_out, (int64_t*)tokens_out, To, (int*)lens);
    } else {
        next_token_k<false><<<B, NT_THREADS, 0, st>>>((const bf16_t*)logits, V, R, (const float*)u, Tu, (const int*)params,
                                                      (int*)step, (uint8_t*)done, (int64_t*)tok_out,
                                                      (int64_t*)tokens_out, To, (int*)lens);
    }
    DDL_RETURN_LAUNCH();
}

// ddl_next_token with params int32 [n_params] (5, or 8: top_p, min_p, repetition_penalty as fp32 bits) and the
// penalty's history: history int64 [B, Lh] (nullable), of which row b counts its first history_lens[b] (int32 [B],
// clamped to 0 .. Lh; nullable: all Lh) entries, plus tokens_out[b, :step[b]] when both are given.  The penalty is
// applied to rows that fit LDS (ddl_next_token_lds(V) != 0); for longer rows the caller penalises the logits.
DDL_API int ddl_next_token_ex(const void* logits, int B, int V, const void* u, int Tu, const void* params, int n_params,
                              const void* history, int Lh, const void* history_lens, void* step, void* done,
                              void* tok_out, void* tokens_out, int To, void* lens, hipStream_t st) {
    if (B < 1 || V < 1 || V > (1 << 30) || !logits || !tok_out || (u && Tu < 1) || (tokens_out && To < 1) ||
        (params && n_params != PRM_SAMPLE + 1 && n_params != PRM_EX) || (history && Lh < 1))
        return (int)hipErrorInvalidValue;
    const int R = nt_run(V);
    const long bytes = ddl_next_token_lds(V);
    if (bytes) {
        static const bool ok = hipFuncSetAttribute((const void*)next_token_ex_k<true>,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, NT_MAX_LDS) == hipSuccess;
        if (!ok) return (int)hipErrorInvalidValue;
        next_token_ex_k<true><<<B, NT_THREADS, (size_t)bytes, st>>>(
            (const bf16_t*)logits, V, R, (const float*)u, Tu, (const int*)params, n_params, (const int64_t*)history, Lh,
            (const int*)history_lens, (int*)step, (uint8_t*)done, (int64_t*)tok_out, (int64_t*)tokens_out, To, (int*)lens);
    } else {
        next_token_ex_k<false><<<B, NT_THREADS, 0, st>>>(
            (const bf16_t*)logits, V, R, (const float*)u, Tu, (const int*)params, n_params, (const int64_t*)history, Lh,
            (const int*)history_lens, (int*)step, (uint8_t*)done, (int64_t*)tok_out, (int64_t*)tokens_out, To, (int*)lens);
    }
    DDL_RETURN_LAUNCH();
}

// h [B, E] = wte[tok] + wpe[lens]: bf16, E % 8 == 0, 16-byte aligned rows; tok int64 [B], lens int32 [B]
DDL_API int ddl_decode_embed(const void* tok, const void* lens, const void* wte, const void* wpe, void* h, int B, int E,
                             int V, int P, hipStream_t st) {
    if (B < 1 || E < 8 || E % 8 || V < 1 || P < 1) return (int)hipErrorInvalidValue;
    decode_embed_k<<<B, DE_THREADS, 0, st>>>((const int64_t*)tok, (const int*)lens, (const bf16_t*)wte, (const bf16_t*)wpe,
                                            (bf16_t*)h, E, V, P);
    DDL_RETURN_LAUNCH();
}
