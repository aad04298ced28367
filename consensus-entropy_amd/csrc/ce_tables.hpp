// ce_tables.hpp -- kernels that write per-item tables to HBM:
//   k_entropy        per-item entropy (and mean) of a committee (ce_committee_entropy).
//   k_vote           hc frequency table + entropy from votes (amg_test.py:88-117);
//                    finish_counts also closes k_va (ce_abi_core.hip).
//   k_segment_mean   frame -> song mean of one member (groupby mean, amg_test.py:437).
// ce_abi_core.o is the only object that instantiates them.
#pragma once
#include "ce_device.hpp"
#include "ce_topq.hpp"  // kBS, lane_id

namespace ce {

// ---------------------------------------------------------------------------
// Per-item entropy to HBM.
// ---------------------------------------------------------------------------
template <class Src>
__global__ __launch_bounds__(kBS) void k_entropy(Src src, int64_t N, double* __restrict__ mean_out,
                                                 double* __restrict__ ent) {
    stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
    constexpr int C = Src::kC;
    for (int64_t i = (int64_t)blockIdx.x * kBS + threadIdx.x; i < N; i += (int64_t)gridDim.x * kBS) {
        double mean[C];
        src.mean(i, mean);
        if (mean_out)
#pragma unroll
            for (int c = 0; c < C; ++c) mean_out[i * C + c] = mean[c];
        ent[i] = entropy_row<C>(mean);
    }
}

// ---------------------------------------------------------------------------
// hc tables: one wave per row (amg_test.py:109-117).
// ---------------------------------------------------------------------------
template <int C>
__device__ __forceinline__ void finish_counts(int (&cnt)[C], int64_t n_row, double* freq_out,
                                              double* ent) {
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt[c] += __shfl_xor(cnt[c], off);
    if (lane_id() == 0) {
        int n = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) n += cnt[c];
        double f[C];
#pragma unroll
        for (int c = 0; c < C; ++c) f[c] = round3((double)cnt[c] / (double)n);
        if (freq_out)
#pragma unroll
            for (int c = 0; c < C; ++c) freq_out[n_row * C + c] = f[c];
        ent[n_row] = entropy_row<C>(f);
    }
}

template <int C>
__global__ __launch_bounds__(kBS) void k_vote(const int8_t* __restrict__ votes, int64_t N, int A, int64_t ld,
                                              double* __restrict__ freq, double* __restrict__ ent) {
    stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
    const int lane = lane_id();
    for (int64_t n = (int64_t)blockIdx.x * (kBS / 64) + (threadIdx.x >> 6); n < N;
         n += (int64_t)gridDim.x * (kBS / 64)) {
        int cnt[C];
#pragma unroll
        for (int c = 0; c < C; ++c) cnt[c] = 0;
        const int8_t* row = votes + n * ld;
        for (int a = lane; a < A; a += 64) {
            const int v = row[a];
#pragma unroll
            for (int c = 0; c < C; ++c) cnt[c] += (v == c);
        }
        finish_counts<C>(cnt, n, freq, ent);
    }
}

// ---------------------------------------------------------------------------
// Frame -> song segment mean: pd.DataFrame(y_probs, index=X_train.index)
// .groupby(['s_id']).mean() (amg_test.py:437, :469) as pandas 1.1.5's
// group_mean computes it (the reference pins pandas==1.1.5): values upcast to
// f64, per (song, class) a sequential sum over the song's frames in row order
// skipping NaN, divided by the non-NaN count (0 -> NaN); a float32 column is
// cast back to float32 at the end (the result dtype follows the input).
// One thread per (song, class); frames of song n are rows perm[off[n]..off[n+1])
// (perm == nullptr: rows off[n]..off[n+1] themselves, already grouped).
// ---------------------------------------------------------------------------
template <int DT, int ODT>
__global__ __launch_bounds__(kBS) void k_segment_mean(const void* __restrict__ frames, int64_t ld, int C,
                                                      const int64_t* __restrict__ perm,
                                                      const int64_t* __restrict__ offsets, int64_t N,
                                                      void* __restrict__ out, int64_t ldo) {
    const int64_t total = N * C;
    for (int64_t t = (int64_t)blockIdx.x * kBS + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBS) {
        const int64_t n = t / C;
        const int c = (int)(t - n * C);
        const int64_t f0 = offsets[n], f1 = offsets[n + 1];
        CE_DASSERT(f0 >= 0 && f0 <= f1);
        double sum = 0.0;
        int64_t cnt = 0;
        // batches of 8 frames: the 8 loads are issued together (clamped rows,
        // no branch around a load), then added in row order
        constexpr int B = 8;
        for (int64_t fb = f0; fb < f1; fb += B) {
            double v[B];
#pragma unroll
            for (int u = 0; u < B; ++u) {
                const int64_t f = fb + u < f1 ? fb + u : f1 - 1;
                const int64_t r = perm ? perm[f] : f;
                if constexpr (DT == kF32)
                    v[u] = (double)static_cast<const float*>(frames)[r * ld + c];
                else
                    v[u] = static_cast<const double*>(frames)[r * ld + c];
            }
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (fb + u < f1 && v[u] == v[u]) {  // not NaN
                    sum += v[u];
                    ++cnt;
                }
        }
        double m = cnt ? sum / (double)cnt : __longlong_as_double(0x7ff8000000000000ll);
        if constexpr (DT == kF32) m = (double)(float)m;  // the float32 result column
        if constexpr (ODT == kF32)
            static_cast<float*>(out)[n * ldo + c] = (float)m;
        else
            static_cast<double*>(out)[n * ldo + c] = m;
    }
}

}  // namespace ce
