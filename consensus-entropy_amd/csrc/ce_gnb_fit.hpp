// ce_gnb_fit.hpp -- GaussianNB.partial_fit on the device: the
// retrain step of the reference's epoch, mod.partial_fit(X_batch, y_batch) at
// amg_test.py:509, for U independent models in one launch.
//
// The arithmetic is sklearn's _partial_fit + _update_mean_variance, operation
// for operation (restated with row loops in tests/gnb_fit_ref.py):
//   epsilon = var_smoothing * max_d np.var(X_batch, 0)       the whole batch
//   var -= epsilon                                             every class
//   per class c in the batch: new_mu = np.mean(X_c, 0), new_var = np.var(X_c, 0),
//     taken as they are when class_count[c] == 0, else the Chan merge
//       total_mu  = (n_new * new_mu + n_past * mu) / n_total
//       total_var = ((n_past * var + n_new * new_var)
//                    + (n_new * n_past / n_total) * (mu - new_mu)^2) / n_total
//     class_count[c] += n_new
//   var += epsilon;  class_prior = class_count / class_count.sum()
// np.mean / np.var over axis 0 of a [n, D >= 2] block add the rows one after
// the other in row order onto +0.0, so a feature's sums are sequential over the
// rows: the parallelism is over features (lanes) and models (blocks).  One
// block owns one model and updates it in place.  Every operation is a plain
// IEEE f64 add / subtract / multiply / divide (the build has -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_debug.hpp"

namespace ce {

constexpr int kFitBS = 256;     // threads per model: two features each (D <= 512)
constexpr int kFitMaxC = 8;     // classes
constexpr int kFitAhead = 16;   // rows per chunk; two chunks of loads are in flight
constexpr int kFitTile = 1024;  // rows whose offsets and classes are staged in LDS at a time

struct GnbFitArgs {
    const double* X;
    int64_t F;
    int D;
    int64_t ld;
    const int64_t* rows;
    const int32_t* labels;
    const int64_t* row_offsets;
    int C;
    double var_smoothing;
    double* theta;
    double* var;
    double* class_count;
    double* class_prior;
    double* epsilon;
};

// kFitAhead rows of a model's batch: this thread's two features of each, and the rows' classes
struct FitChunk {
    double2 x[kFitAhead];
    int lab[kFitAhead];
};

// Rows base .. base + kFitAhead - 1 of the staged tile (tn rows: element offsets
// s_off, classes s_lab).  Every load is issued unconditionally (a chunk past
// the end re-reads the tile's last row, which nothing accumulates): loads
// under a branch would each wait for their own.
template <bool VEC2>
__device__ __forceinline__ void fit_load(const double* X, const int64_t* s_off, const int* s_lab, int tn, int base,
                                         int f0, int f1, FitChunk& ch) {
#pragma unroll
    for (int j = 0; j < kFitAhead; ++j) {
        const int i = base + j < tn ? base + j : tn - 1;
        CE_DASSERT(i >= 0 && i < kFitTile);
        const double* xr = X + s_off[i];
        if constexpr (VEC2) ch.x[j] = *reinterpret_cast<const double2*>(xr + f0);  // f1 = f0 + 1, 16-byte aligned
        else ch.x[j] = double2{xr[f0], xr[f1]};
        ch.lab[j] = __builtin_amdgcn_readfirstlane(s_lab[i]);  // one class per row: a wave-uniform branch below
    }
}

// One pass over the batch rows[lo .. lo + n) in row order: f(x, class) per row
// (class -1: a slot past the end of the tile, which f must leave out).
// The block stages a tile's row offsets and classes in LDS (one coalesced read,
// so no frame load waits for an index load), then every wave that owns a
// feature walks the tile, two chunks of row loads in flight.  Block-uniform
// control flow around the barriers: every thread of the block calls this.
template <bool VEC2, class Fn>
__device__ __forceinline__ void fit_pass(const GnbFitArgs& a, int64_t lo, int64_t n, int f0, int f1, bool live,
                                         int64_t* s_off, int* s_lab, Fn&& f) {
    for (int64_t t0 = 0; t0 < n; t0 += kFitTile) {
        const int tn = (int)(n - t0 < kFitTile ? n - t0 : kFitTile);
        __syncthreads();  // the tile before is consumed
        for (int i = threadIdx.x; i < tn; i += kFitBS) {
            int64_t row = a.rows[lo + t0 + i];
            const int lab = a.labels[lo + t0 + i];
            CE_DASSERT(row >= 0 && row < a.F);
            CE_DASSERT(lab >= 0 && lab < a.C);
            row = row < 0 ? 0 : (row < a.F ? row : a.F - 1);  // a bad row reads a wrong frame, never outside X
            s_off[i] = row * a.ld;
            s_lab[i] = lab;
        }
        __syncthreads();
        if (!live) continue;  // wave-uniform
        FitChunk c0, c1;
        fit_load<VEC2>(a.X, s_off, s_lab, tn, 0, f0, f1, c0);
        for (int base = 0; base < tn; base += 2 * kFitAhead) {
            fit_load<VEC2>(a.X, s_off, s_lab, tn, base + kFitAhead, f0, f1, c1);
#pragma unroll
            for (int j = 0; j < kFitAhead; ++j) f(c0.x[j], base + j < tn ? c0.lab[j] : -1);
            fit_load<VEC2>(a.X, s_off, s_lab, tn, base + 2 * kFitAhead, f0, f1, c0);
#pragma unroll
            for (int j = 0; j < kFitAhead; ++j) f(c1.x[j], base + kFitAhead + j < tn ? c1.lab[j] : -1);
        }
    }
}

// An empty statement the compiler cannot move or merge, holding v in registers.
__device__ __forceinline__ void fit_pin(double2& v) { asm volatile("" : "+v"(v.x), "+v"(v.y)); }

// np.max of two values: NaN if either is
__device__ __forceinline__ double fit_nanmax(double a, double b) {
    if (a != a) return a;
    if (b != b) return b;
    return a > b ? a : b;
}

// _update_mean_variance for one feature of one class present in the batch
// (n_new >= 1 rows: new_mu, new_var); var comes in with epsilon taken off.
__device__ __forceinline__ void fit_merge(double n_new, double n_past, double new_mu, double new_var, double& mu,
                                          double& var) {
    if (n_past == 0.0) {
        mu = new_mu;
        var = new_var;
        return;
    }
    const double n_total = n_past + n_new;
    const double total_mu = (n_new * new_mu + n_past * mu) / n_total;
    const double d = mu - new_mu;
    const double total_ssd = (n_past * var + n_new * new_var) + (n_new * n_past / n_total) * (d * d);
    mu = total_mu;
    var = total_ssd / n_total;
}

// Block u: model u's partial_fit on its batch rows[row_offsets[u] .. row_offsets[u+1]).
// VEC2 (D and ld even, X 16-byte aligned): thread t owns features 2t, 2t+1 (one
// 16-byte load per row); else features t and t + 256 (two 8-byte loads).  A
// thread without a feature reads a valid one again and writes nothing.  CM:
// accumulators per feature (C <= CM classes; accumulator CM is the whole batch's).
template <bool VEC2, int CM>
__global__ __launch_bounds__(kFitBS) void k_gnb_partial_fit(GnbFitArgs a) {
    __shared__ int64_t s_off[kFitTile];
    __shared__ int s_lab[kFitTile];
    __shared__ double red[kFitBS / 64];
    const int u = blockIdx.x, t = threadIdx.x;
    const int D = a.D, C = a.C;
    const int64_t lo = a.row_offsets[u], n = a.row_offsets[u + 1] - lo;
    if (n <= 0) return;  // an empty batch leaves the model untouched (block-uniform: before any barrier)
    int f0 = VEC2 ? 2 * t : t, f1 = VEC2 ? 2 * t + 1 : t + kFitBS;
    const bool ok0 = f0 < D, ok1 = f1 < D;
    if (VEC2) {
        if (!ok0) f0 = D - 2, f1 = D - 1;
    } else {
        if (!ok0) f0 = D - 1;
        if (!ok1) f1 = D - 1;
    }
    CE_DASSERT(f0 >= 0 && f0 < D && f1 >= 0 && f1 < D);
    const bool live = (VEC2 ? 2 : 1) * (t & ~63) < D;  // wave-uniform: this wave owns a feature
    double cc[CM];  // read before the barrier; thread 0 writes the new counts after it
#pragma unroll
    for (int k = 0; k < CM; ++k) cc[k] = k < C ? a.class_count[(int64_t)u * C + k] : 0.0;

    // pass 1: column sums per class and of the whole batch, rows per class
    double2 s[CM + 1];
    int64_t cnt[CM];
#pragma unroll
    for (int k = 0; k <= CM; ++k) s[k] = double2{0.0, 0.0};
#pragma unroll
    for (int k = 0; k < CM; ++k) cnt[k] = 0;
    // A row goes to its class's accumulator through a wave-uniform branch -- never
    // through a select that adds 0.0, which would turn a -0.0 sum into +0.0.
    // fit_pin ends every branch: without it the compiler merges the branches into
    // one indexed accumulator array in scratch memory, a dependent round trip per row.
    fit_pass<VEC2>(a, lo, n, f0, f1, live, s_off, s_lab, [&](const double2& x, int c) {
        CE_DASSERT(c >= -1 && c < CM);  // the accumulator index
        if (c >= 0) {
            s[CM].x += x.x;
            s[CM].y += x.y;
            fit_pin(s[CM]);
        }
#pragma unroll
        for (int k = 0; k < CM; ++k)
            if (c == k) {
                s[k].x += x.x;
                s[k].y += x.y;
                ++cnt[k];
                fit_pin(s[k]);
            }
    });
    // sums -> means (np.mean's true divide)
    const double dn = (double)n;
    s[CM].x /= dn;
    s[CM].y /= dn;
#pragma unroll
    for (int k = 0; k < CM; ++k)
        if (cnt[k] > 0) {
            s[k].x /= (double)cnt[k];
            s[k].y /= (double)cnt[k];
        }

    // pass 2 over the same rows (from L2 for one model; with hundreds of models in flight the batch is fetched
    // again): squared deviations from the class mean and the batch mean
    double2 q[CM + 1];
#pragma unroll
    for (int k = 0; k <= CM; ++k) q[k] = double2{0.0, 0.0};
    fit_pass<VEC2>(a, lo, n, f0, f1, live, s_off, s_lab, [&](const double2& x, int c) {
        if (c >= 0) {
            const double ex = x.x - s[CM].x, ey = x.y - s[CM].y;
            q[CM].x += ex * ex;
            q[CM].y += ey * ey;
            fit_pin(q[CM]);
        }
#pragma unroll
        for (int k = 0; k < CM; ++k)
            if (c == k) {
                const double dx = x.x - s[k].x, dy = x.y - s[k].y;
                q[k].x += dx * dx;
                q[k].y += dy * dy;
                fit_pin(q[k]);
            }
    });

    // epsilon: var_smoothing * np.var(X_batch, 0).max() over the D features (NaN if any is)
    double m = -__builtin_inf();
    if (ok0) m = q[CM].x / dn;
    if (ok1) m = fit_nanmax(m, q[CM].y / dn);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fit_nanmax(m, __shfl_xor(m, off));
    if ((t & 63) == 0) red[t >> 6] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < kFitBS / 64; ++w) m = fit_nanmax(m, red[w]);
    const double eps = a.var_smoothing * m;

    // the merge, feature by feature; a class absent from the batch keeps theta and has var - eps + eps
#pragma unroll
    for (int k = 0; k < CM; ++k) {
        if (k >= C) continue;
        double* th = a.theta + ((int64_t)u * C + k) * D;
        double* va = a.var + ((int64_t)u * C + k) * D;
        const double n_new = (double)cnt[k];
        if (ok0) {
            double mu = th[f0], v = va[f0] - eps;
            if (cnt[k] > 0) {
                fit_merge(n_new, cc[k], s[k].x, q[k].x / n_new, mu, v);
                th[f0] = mu;
            }
            va[f0] = v + eps;
        }
        if (ok1) {
            double mu = th[f1], v = va[f1] - eps;
            if (cnt[k] > 0) {
                fit_merge(n_new, cc[k], s[k].y, q[k].y / n_new, mu, v);
                th[f1] = mu;
            }
            va[f1] = v + eps;
        }
    }

    if (t == 0) {  // wave 0 always owns a feature, so its cnt[] are the batch's
#pragma unroll
        for (int k = 0; k < CM; ++k)
            if (cnt[k] > 0) cc[k] = cc[k] + (double)cnt[k];
        // class_count_.sum(): the counts are whole numbers far below 2^53, so every order of summation is exact
        double tot = cc[0];
#pragma unroll
        for (int k = 1; k < CM; ++k)
            if (k < C) tot = tot + cc[k];
#pragma unroll
        for (int k = 0; k < CM; ++k)
            if (k < C) {
                a.class_count[(int64_t)u * C + k] = cc[k];
                a.class_prior[(int64_t)u * C + k] = cc[k] / tot;
            }
        a.epsilon[u] = eps;
    }
}

}  // namespace ce
