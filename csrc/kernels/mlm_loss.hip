// Masked-LM loss kernels: row cross-entropy over strided rows with ignored targets, split into a
// forward (log-sum-exp + row loss) and a backward (softmax - onehot, scaled), and the row scatter of
// the masked-position gather's backward.  HBM-bound row kernels: one 256-thread block per row,
// 16-byte accesses, fixed-order reductions (bitwise repeatable, no float atomics, no host sync).
//
// Row layout: logits [M, ld], columns [0, C) valid, columns [C, ld) padding (ld % 8 == 0, so the
// vocabulary GEMM's 8-padded output feeds these kernels and the backward's output feeds the dgrad /
// wgrad GEMMs with no slicing copy).  Padding is loaded with its vector but masked before any math.
//
// A row is skipped when its label equals ignore_index -- or lies outside [0, C), which F.cross_entropy
// rejects on the host; a device-side check cannot raise, so such a row counts as ignored rather than
// indexing outside its row.
#include "ddl_common.h"

namespace {

__device__ __forceinline__ bool row_valid(long lab, long ignore_index, int C) {
    return lab != ignore_index && lab >= 0 && lab < (long)C;
}

__device__ __forceinline__ float block_max256(float m, float* red) {
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return m;
}

// Forward, register-resident: thread t holds vectors t, t + 256, ... (NV of them, 8 columns each), so
// the row is read from memory once: max, then sum of exponentials, from registers.
template <typename T, int NV>
__global__ __launch_bounds__(256) void ce_lse_reg_k(const T* __restrict__ logits, long ld, int C,
                                                    const int64_t* __restrict__ labels, long ignore_index,
                                                    float* __restrict__ lse, float* __restrict__ row_loss) {
    __shared__ float red[4];
    const long row = blockIdx.x;
    const long lab = labels[row];
    if (!row_valid(lab, ignore_index, C)) return;     // the row is not read at all
    const T* x = logits + row * ld;
    float v[NV][8];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c0 = ((int)threadIdx.x + i * 256) * 8;
        if (c0 < C) {
            load8(x + c0, v[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (c0 + j >= C) v[i][j] = -INFINITY;
                m = fmaxf(m, v[i][j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[i][j] = -INFINITY;
        }
    }
    m = block_max256(m, red);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j) s += __expf(v[i][j] - m);    // exp(-inf) = 0 for masked columns
    }
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) {
        const float l = m + logf(s);
        lse[row] = l;
        row_loss[row] = l - to_f(x[lab]);
    }
}

// Forward, streaming (rows wider than the register form holds): a max pass, then a sum pass that
// re-reads the row (from L2 for any realistic width).
template <typename T>
__global__ __launch_bounds__(256) void ce_lse_stream_k(const T* __restrict__ logits, long ld, int C,
                                                       const int64_t* __restrict__ labels, long ignore_index,
                                                       float* __restrict__ lse, float* __restrict__ row_loss) {
    __shared__ float red[4];
    const long row = blockIdx.x;
    const long lab = labels[row];
    if (!row_valid(lab, ignore_index, C)) return;
    const T* x = logits + row * ld;
    const int nvec = (C + 7) / 8;
    float m = -INFINITY;
    for (int vi = threadIdx.x; vi < nvec; vi += 256) {
        float v[8];
        load8(x + vi * 8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (vi * 8 + j < C) m = fmaxf(m, v[j]);
    }
    m = block_max256(m, red);
    float s = 0.f;
    for (int vi = threadIdx.x; vi < nvec; vi += 256) {
        float v[8];
        load8(x + vi * 8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (vi * 8 + j < C) s += __expf(v[j] - m);
    }
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) {
        const float l = m + logf(s);
        lse[row] = l;
        row_loss[row] = l - to_f(x[lab]);
    }
}

// Mean over the valid rows in a fixed order (thread t sums rows t, t + 256, ...; then the block tree):
// the same bits on every run.  No valid row: loss 0 and 1 / n_valid = 0, so the backward writes zeros.
__global__ __launch_bounds__(256) void ce_finish_k(const float* __restrict__ row_loss,
                                                   const int64_t* __restrict__ labels, long M, int C,
                                                   long ignore_index, float* __restrict__ loss,
                                                   float* __restrict__ inv_n) {
    __shared__ float red[4];
    __shared__ int cnt[4];
    float s = 0.f;
    int n = 0;
    for (long r = threadIdx.x; r < M; r += 256) {
        if (row_valid(labels[r], ignore_index, C)) {
            s += row_loss[r];
            ++n;
        }
    }
    s = block_sum<256>(s, red);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int tot = cnt[0] + cnt[1] + cnt[2] + cnt[3];
        loss[0] = tot > 0 ? s / (float)tot : 0.f;
        inv_n[0] = tot > 0 ? 1.f / (float)tot : 0.f;
    }
}

// Backward: dst[r, c] = (exp(x[r, c] - lse[r]) - [c == label]) * g / n_valid for c < C, exact zeros
// for c in [C, ld) and for ignored rows.  dst may be the logits buffer itself (every thread reads a
// vector before it writes the same one; x / dst are therefore not __restrict__).
template <typename T>
__global__ __launch_bounds__(256) void ce_bwd_k(const T* x, long ld, int C, const int64_t* __restrict__ labels,
                                                long ignore_index, const float* __restrict__ lse,
                                                const float* __restrict__ g, const float* __restrict__ inv_n,
                                                T* dst) {
    const long row = blockIdx.x;
    const long lab = labels[row];
    const int nvec = (int)(ld / 8);
    T* d = dst + row * ld;
    if (!row_valid(lab, ignore_index, C)) {
        const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int vi = threadIdx.x; vi < nvec; vi += 256) store8(d + vi * 8, z);
        return;
    }
    const T* xr = x + row * ld;
    const float l = lse[row];
    const float scale = g[0] * inv_n[0];
    for (int vi = threadIdx.x; vi < nvec; vi += 256) {
        const int c0 = vi * 8;
        float v[8];
        if (c0 < C) {
            load8_nt(xr + c0, v);       // the last read of these logits
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = c0 + j;
                const float p = __expf(v[j] - l) - (c == (int)lab ? 1.f : 0.f);
                v[j] = c < C ? p * scale : 0.f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.f;
        }
        store8(d + c0, v);
    }
}

// Row of slot t: pos[t] itself, or, for positions given per sequence ([B, P] slots into [B, S] rows),
// (t / P) * S + pos[t] -- the flat index is formed here, not by index arithmetic kernels before.
__device__ __forceinline__ long slot_row(const int64_t* __restrict__ pos, long t, long P, long S) {
    return pos[t] + (P > 0 ? (t / P) * S : 0);
}

// out[i, :] = h[row(i), :], 16 bytes per lane (the embedding gather with the per-sequence offset and a
// range check: a position outside [0, R) reads nothing and yields zeros).
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_k(const T* __restrict__ h, const int64_t* __restrict__ pos,
                                                     T* __restrict__ out, long n, long R, int D, long P, long S) {
    const int d8 = D / 8;
    const long total = n * d8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long t = i / d8;
        const int dg = (int)(i % d8);
        const long r = slot_row(pos, t, P, S);
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (r >= 0 && r < R) load8(h + r * D + dg * 8, v);
        store8(out + t * D + dg * 8, v);
    }
}

// dh[row(i), :] = dy[i, :] for every slot i whose label is not ignore_index (labels == nullptr: every
// slot), 16 bytes per lane.  dh was zero-filled before; valid positions are unique, so no two slots
// write the same row.
template <typename T>
__global__ __launch_bounds__(256) void scatter_rows_k(const T* __restrict__ dy, const int64_t* __restrict__ pos,
                                                      const int64_t* __restrict__ labels, long ignore_index,
                                                      T* __restrict__ dh, long n, long R, int D, long P, long S) {
    const int d8 = D / 8;
    const long total = n * d8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long t = i / d8;
        const int dg = (int)(i % d8);
        if (labels && labels[t] == ignore_index) continue;
        const long r = slot_row(pos, t, P, S);
        if (r < 0 || r >= R) continue;
        float v[8];
        load8(dy + t * D + dg * 8, v);
        store8(dh + r * D + dg * 8, v);
    }
}

inline int grid_for(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 8192)); }

template <typename T>
void launch_lse(const T* x, long M, long ld, int C, const int64_t* labels, long ignore_index, float* lse,
                float* row_loss, hipStream_t st) {
    if (C <= 256 * 4 * 8)
        ce_lse_reg_k<T, 4><<<M, 256, 0, st>>>(x, ld, C, labels, ignore_index, lse, row_loss);
    else if (C <= 256 * 16 * 8)
        ce_lse_reg_k<T, 16><<<M, 256, 0, st>>>(x, ld, C, labels, ignore_index, lse, row_loss);
    else
        ce_lse_stream_k<T><<<M, 256, 0, st>>>(x, ld, C, labels, ignore_index, lse, row_loss);
}

}  // namespace

DDL_API int ddl_zero(void* p, long nbytes, hipStream_t st);   // elementwise.hip

// lse / row_loss: fp32 [M] workspaces (entries of ignored rows are left unwritten and never read);
// loss / inv_n: fp32 scalars on the device.
DDL_API int ddl_ce_lse(int dtype, const void* logits, long M, long ld, int C, const int64_t* labels, long ignore_index,
                       float* lse, float* row_loss, float* loss, float* inv_n, hipStream_t st) {
    if (M <= 0 || C <= 0 || ld < C || ld % 8 || ((uintptr_t)logits & 15)) return -1;
    if (dtype == 1) launch_lse<bf16_t>((const bf16_t*)logits, M, ld, C, labels, ignore_index, lse, row_loss, st);
    else launch_lse<float>((const float*)logits, M, ld, C, labels, ignore_index, lse, row_loss, st);
    ce_finish_k<<<1, 256, 0, st>>>(row_loss, labels, M, C, ignore_index, loss, inv_n);
    DDL_RETURN_LAUNCH();
}

DDL_API int ddl_ce_bwd(int dtype, const void* logits, long M, long ld, int C, const int64_t* labels, long ignore_index,
                       const float* lse, const float* g, const float* inv_n, void* dlogits, hipStream_t st) {
    if (M <= 0 || C <= 0 || ld < C || ld % 8 || ((uintptr_t)logits & 15) || ((uintptr_t)dlogits & 15)) return -1;
    if (dtype == 1)
        ce_bwd_k<bf16_t><<<M, 256, 0, st>>>((const bf16_t*)logits, ld, C, labels, ignore_index, lse, g, inv_n,
                                            (bf16_t*)dlogits);
    else
        ce_bwd_k<float><<<M, 256, 0, st>>>((const float*)logits, ld, C, labels, ignore_index, lse, g, inv_n,
                                           (float*)dlogits);
    DDL_RETURN_LAUNCH();
}

// out [n, D]: out[i] = h[row(i)] of h [R, D]; row(i) = pos[i] (P = 0) or (i / P) * S + pos[i].
DDL_API int ddl_gather_rows(int dtype, const void* h, const int64_t* pos, void* out, long n, long R, int D, long P,
                            long S, hipStream_t st) {
    if (D <= 0 || D % 8 || R <= 0 || P < 0 || ((uintptr_t)h & 15) || ((uintptr_t)out & 15)) return -1;
    if (n <= 0) return 0;
    const long tot = n * (D / 8);
    if (dtype == 1)
        gather_rows_k<bf16_t><<<grid_for(tot), 256, 0, st>>>((const bf16_t*)h, pos, (bf16_t*)out, n, R, D, P, S);
    else
        gather_rows_k<float><<<grid_for(tot), 256, 0, st>>>((const float*)h, pos, (float*)out, n, R, D, P, S);
    DDL_RETURN_LAUNCH();
}

// dh [R, D] = 0, then dh[row(i)] = dy[i] for the slots whose label is not ignore_index.
DDL_API int ddl_scatter_rows(int dtype, const void* dy, const int64_t* pos, const int64_t* labels, long ignore_index,
                             void* dh, long n, long R, int D, long P, long S, hipStream_t st) {
    if (D <= 0 || D % 8 || R <= 0 || P < 0 || ((uintptr_t)dy & 15) || ((uintptr_t)dh & 15)) return -1;
    const int rc = ddl_zero(dh, R * (long)D * (dtype == 1 ? 2 : 4), st);
    if (rc != 0 || n <= 0) return rc;
    const long tot = n * (D / 8);
    if (dtype == 1)
        scatter_rows_k<bf16_t><<<grid_for(tot), 256, 0, st>>>((const bf16_t*)dy, pos, labels, ignore_index,
                                                              (bf16_t*)dh, n, R, D, P, S);
    else
        scatter_rows_k<float><<<grid_for(tot), 256, 0, st>>>((const float*)dy, pos, labels, ignore_index, (float*)dh,
                                                             n, R, D, P, S);
    DDL_RETURN_LAUNCH();
}
