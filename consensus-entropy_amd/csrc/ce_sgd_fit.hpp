// ce_sgd_fit.hpp -- SGDClassifier.partial_fit on the device:
// the retrain step of the reference's epoch, mod.partial_fit(X_batch, y_batch) at
// amg_test.py:509, for its 'classifier_sgd' member (deam_classifier.py:214-217:
// loss='log', penalty='l2', learning_rate='optimal', shuffle, no averaging, no
// weights), U independent models in one launch.
//
// The arithmetic is one epoch of sklearn's _plain_sgd64 per binary problem,
// operation for operation (restated with row loops in tests/sgd_fit_ref.py).
// The rows of a problem are visited in the order of SequentialDataset.shuffle
// (Fisher-Yates over sklearn's xorshift); per visited row, with w, wscale = 1,
// intercept b and step counter t:
//   p      = (sum_j w[j] * x[j], added in feature order onto +0.0) * wscale + b
//   eta    = 1 / (alpha * (optimal_init + t - 1))
//   g      = the loss gradient at (y, p), clipped to +-1e12;  update = -eta * g
//   wscale *= max(0, 1 - eta * alpha);  below 1e-9: w *= wscale, wscale = 1
//   update != 0:  w += x * (update / wscale);  b += update
//   t += 1
// and w *= wscale after the last row.  Every operation is a plain IEEE f64 add,
// subtract, multiply or divide (the build has -ffp-contract=off) or glibc's exp.
//
// One block owns one model, one wave one binary problem (K <= 8 waves); all K
// read the model's t before the barrier after which thread 0 advances it.
// A problem is a serial chain over its rows, and within a row the dot product
// is a chain of D dependent adds in feature order.  Lane l keeps features
// 8l .. 8l+7 of w in registers: the products and the update of w run across the
// lanes, and the ordered sum walks them -- lane l takes lane l-1's running sum
// (a DPP wave shift), adds its 8 products one after the other, and after
// ceil(D / 8) steps lane ceil(D / 8) - 1 holds the sum.  The longer a lane's run
// the fewer hops (D adds + 2 moves per 8 features), so one run length serves
// every D.  The rows to come are known (the permutation is built first), so the
// loads of the next rows are in flight while a row's chain runs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_debug.hpp"
#include "ce_glibc_exp.hpp"

namespace ce {

constexpr int kSgdMaxK = 8;        // binary problems of a model = waves of its block
constexpr int kSgdMaxD = 512;      // features: 64 lanes x kSgdRun
constexpr int kSgdRun = 8;         // consecutive features per lane
constexpr int kSgdAhead = 4;       // rows per chunk; two chunks of loads are in flight
constexpr int kSgdPermLds = 8192;  // a model's K permutations stay in LDS up to this many indices (K * n)
constexpr int kSgdGradHalfBinomial = 0, kSgdGradLogDloss = 1;
constexpr int kSgdNonFinite = 1, kSgdNotRun = 2;  // status values

struct SgdFitArgs {
    const double* X;
    int64_t F;
    int D;
    int64_t ld;
    const int64_t* rows;
    const int32_t* labels;
    const int64_t* row_offsets;
    int K;
    double alpha, optimal_init;
    const uint32_t* seeds;
    double* coef;
    double* intercept;
    double* t;
    int32_t* status;
    int32_t* ws;       // permutations that do not fit in LDS: model u's at ws + K * row_offsets[u]
    int64_t ws_slots;  // int32 slots of ws
};

// the running sum of the lane below (lane 0: +0.0)
__device__ __forceinline__ double sgd_from_lane_below(double s) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(s), 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(s), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double sgd_lane_value(double v, int lane) {  // lane: wave-uniform
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                            __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// the loss gradient at (y in {0, 1}, p)
template <int GRAD>
__device__ __forceinline__ double sgd_gradient(double y, double p) {
    if constexpr (GRAD == kSgdGradHalfBinomial) {  // sklearn >= 1.x: cgradient_half_binomial
        if (p > -37.0) {
            const double e = dexp(-p);
            return ((1.0 - y) - y * e) / (1.0 + e);
        }
        return dexp(p) - y;
    } else {  // sklearn 0.24.1: Log.dloss on labels +-1
        const double ys = y > 0.0 ? 1.0 : -1.0;
        const double z = p * ys;
        if (z > 18.0) return dexp(-z) * -ys;
        if (z < -18.0) return -ys;
        return -ys / (dexp(z) + 1.0);
    }
}

// 64 rows of a problem's visiting order, one per lane: the row's element offset in X and its class
struct SgdMeta {
    int64_t off;
    int lab;
};

// kSgdAhead rows: this lane's run of each, and the rows' classes (wave-uniform)
struct SgdChunk {
    double x[kSgdAhead][kSgdRun];
    int lab[kSgdAhead];
};

template <int GRAD>
__global__ __launch_bounds__(64 * kSgdMaxK) void k_sgd_partial_fit(SgdFitArgs a) {
    __shared__ int32_t s_perm[kSgdPermLds];
    const int u = blockIdx.x, k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int D = a.D, K = a.K;
    const int64_t lo = a.row_offsets[u], n64 = a.row_offsets[u + 1] - lo;
    if (n64 <= 0) return;  // an empty batch leaves the model untouched (block-uniform: before any barrier)
    const bool in_lds = (int64_t)K * n64 <= kSgdPermLds;
    if (n64 > 0x7fffffffll || (!in_lds && (!a.ws || (int64_t)K * (lo + n64) > a.ws_slots))) {
        if (threadIdx.x == 0) a.status[u] = kSgdNotRun;  // block-uniform
        return;
    }
    CE_DASSERT(lo >= 0);
    const int n = (int)n64;
    int32_t* perm = in_lds ? s_perm + k * n : a.ws + (int64_t)K * lo + (int64_t)k * n;

    // the visiting order: SequentialDataset.shuffle(seed) of the identity, by one lane
    for (int i = lane; i < n; i += 64) perm[i] = i;
    __syncthreads();
    if (lane == 0) {
        uint32_t seed = a.seeds[(int64_t)u * K + k];
        for (int i = 0; i < n - 1; ++i) {
            if (seed == 0) seed = 1;
            seed ^= seed << 13;
            seed ^= seed >> 17;
            seed ^= seed << 5;
            const int j = i + (int)((seed % 2147483648u) % (uint32_t)(n - i));
            CE_DASSERT(j >= i && j < n);
            const int32_t vi = perm[i], vj = perm[j];
            perm[i] = vj;
            perm[j] = vi;
        }
    }
    const double t0 = a.t[u];  // every wave reads it before the barrier; thread 0 writes it after its last row
    double t = t0;
    __threadfence_block();
    __syncthreads();

    // this lane's run of features; a lane past D reads a valid feature again, multiplies nothing and writes nothing
    const int f0 = lane * kSgdRun;
    const int steps = (D + kSgdRun - 1) / kSgdRun;  // lanes that own a feature
    int f[kSgdRun];
    bool ok[kSgdRun];
    double w[kSgdRun];
    double* coef = a.coef + ((int64_t)u * K + k) * D;
#pragma unroll
    for (int q = 0; q < kSgdRun; ++q) {
        ok[q] = f0 + q < D;
        f[q] = ok[q] ? f0 + q : D - 1;
        w[q] = ok[q] ? coef[f[q]] : 0.0;
    }
    double b = a.intercept[(int64_t)u * K + k];
    double wscale = 1.0;
    const int pos = K == 1 ? 1 : k;  // the positive class of this problem
    const double alpha = a.alpha, oi = a.optimal_init;

    auto load_meta = [&](int r0) {
        int i = r0 + lane;
        i = i < n ? i : n - 1;  // past the end: the last row again, which nothing visits twice
        int idx = perm[i];
        CE_DASSERT(idx >= 0 && idx < n);
        idx = idx < 0 ? 0 : (idx < n ? idx : n - 1);
        int64_t row = a.rows[lo + idx];
        CE_DASSERT(row >= 0 && row < a.F);
        row = row < 0 ? 0 : (row < a.F ? row : a.F - 1);  // a bad row reads a wrong frame, never outside X
        return SgdMeta{row * a.ld, a.labels[lo + idx]};
    };
    SgdMeta m_cur = load_meta(0), m_next = load_meta(64);
    // chunk c = rows c * kSgdAhead ..; called for c = 0, 1, 2, ... in turn.  Every load is issued
    // unconditionally: loads under a branch would each wait for their own.
    auto issue = [&](int c, SgdChunk& ch) {
        const int r0 = c * kSgdAhead;
        if (r0 > 0 && (r0 & 63) == 0) {  // wave-uniform: the next 64 rows' offsets, 64 rows before they are needed
            m_cur = m_next;
            m_next = load_meta(r0 + 64);
        }
#pragma unroll
        for (int j = 0; j < kSgdAhead; ++j) {
            const int src = (r0 + j) & 63;
            const int64_t off = ((int64_t)__builtin_amdgcn_readlane((int)(m_cur.off >> 32), src) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)m_cur.off, src);
            ch.lab[j] = __builtin_amdgcn_readlane(m_cur.lab, src);
            const double* xr = a.X + off;
#pragma unroll
            for (int q = 0; q < kSgdRun; ++q) ch.x[j][q] = xr[f[q]];
        }
    };
    auto visit = [&](const double (&x)[kSgdRun], int lab) {
        const double y = lab == pos ? 1.0 : 0.0;
        double pr[kSgdRun];
#pragma unroll
        for (int q = 0; q < kSgdRun; ++q) pr[q] = ok[q] ? w[q] * x[q] : 0.0;
        // the ordered sum: after step l, lane l holds the sum of features 0 .. 8l+7.  The products past D
        // are +0.0 and come after every feature; a sum that started at +0.0 is never -0.0, so they leave it as it is.
        double s = 0.0;
        for (int l = 0; l < steps; ++l) {
            s = sgd_from_lane_below(s);
#pragma unroll
            for (int q = 0; q < kSgdRun; ++q) s += pr[q];
        }
        const double p = sgd_lane_value(s, steps - 1) * wscale + b;
        const double eta = 1.0 / (alpha * (oi + t - 1.0));
        double g = sgd_gradient<GRAD>(y, p);
        if (g < -1e12) g = -1e12;
        else if (g > 1e12) g = 1e12;
        const double update = -eta * g;
        const double shrink = 1.0 - eta * alpha;
        wscale *= shrink > 0.0 ? shrink : 0.0;
        if (wscale < 1e-9) {  // wave-uniform, as everything from p on
#pragma unroll
            for (int q = 0; q < kSgdRun; ++q) w[q] *= wscale;
            wscale = 1.0;
        }
        if (update != 0.0) {
            const double c = update / wscale;
#pragma unroll
            for (int q = 0; q < kSgdRun; ++q) w[q] += x[q] * c;
            b += update;
        }
        t += 1.0;
    };

    SgdChunk c0, c1;
    issue(0, c0);
    const int chunks = (n + kSgdAhead - 1) / kSgdAhead;
    for (int c = 0; c < chunks; c += 2) {
        issue(c + 1, c1);
#pragma unroll
        for (int j = 0; j < kSgdAhead; ++j)
            if (c * kSgdAhead + j < n) visit(c0.x[j], c0.lab[j]);
        issue(c + 2, c0);
#pragma unroll
        for (int j = 0; j < kSgdAhead; ++j)
            if ((c + 1) * kSgdAhead + j < n) visit(c1.x[j], c1.lab[j]);
    }

    // reset_wscale, and sklearn's under-/overflow check (it raises; here the model's flag is set)
    bool bad = lane == 0 && !__builtin_isfinite(b);
#pragma unroll
    for (int q = 0; q < kSgdRun; ++q) {
        w[q] *= wscale;
        if (ok[q]) {
            coef[f[q]] = w[q];
            bad |= !__builtin_isfinite(w[q]);
        }
    }
    if (lane == 0) a.intercept[(int64_t)u * K + k] = b;
    if (__ballot(bad) != 0 && lane == 0) a.status[u] = kSgdNonFinite;
    if (threadIdx.x == 0) a.t[u] = t0 + (double)n;  // t_ += n: once per model, not once per problem
}

}  // namespace ce
