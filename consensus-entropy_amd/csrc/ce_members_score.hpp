// ce_members_score.hpp -- the evaluate step of an epoch for the linear members
// (SURVEY.md §8(f)5c): after the retrain, amg_test.py:513-515 (and :411-413
// before epoch 0) has every user's model predict that user's TEST frames and
// scores the labels,
//   this_mod_pred = mod.predict(X_test.values)
//   f1_score(y_test_enc.values, this_mod_pred, average='weighted')
// Here: one launch per member that labels every test frame row with the model
// of the user who owns it and counts (true class, predicted class) per user
// (the score kernels), and one launch from the counts to every user's weighted
// F1 (k_f1_weighted_users).
//
// The score kernels are the users form of mod.predict: the walk is
// ce_members_users.hpp's (users_runs / users_walk, unchanged: the block share,
// the cut at user boundaries, one user's parameters staged per run, rows out of
// range and excluded songs skipped) over the geometry of the TEST songs, and per
// frame the scores are the ones the proba kernels form -- GaussianNB: jll[c],
// the same operations in the same order as k_gnb_proba_users / k_gnb_users260 up
// to and including jll[c] = lp[c] + n_ij (no logsumexp, no exp); SGD: the
// decision value, the butterfly of the lanes' fma chains plus the intercept, as
// sgd_expit forms its argument.  predict is the argmax of THOSE (not of the
// rounded probabilities): np.argmax's rule (the first maximum; a NaN wins at
// its first occurrence), and score > 0 for a binary SGD model (NaN: class 0).
//
// Counts: a block keeps C * C int32 counters in LDS for the user of its run,
// bumped by the one lane per frame that holds (y, pred), and adds them to
// cm[u, y, pred] (int64) with atomicAdd where the tables change hands (inside
// stage, behind its first barrier) and once more after the walk.  Integer adds
// commute: cm is the same on every run.  A row whose label is outside [0, C) is
// not counted and nothing is written for it.
#pragma once
#include "ce_members_users.hpp"

namespace ce {

struct ScoreOut {
    const int32_t* y;          // [F] by row of X: the encoded class, 0 .. C-1
    unsigned long long* cm;    // [U, C, C] counts (int64), zero before the launch
    int32_t* pred;             // [F] by row of X, or nullptr
    double* scores;            // [F, C] (row pitch lds), or nullptr
    int64_t lds;
};

// np.argmax over s[0 .. C): the first maximum; a NaN wins at its first occurrence
template <int N>
__device__ __forceinline__ int np_argmax(const double (&s)[N], int C) {
    int best = 0;
    double mp = s[0];
    if (mp != mp) return 0;
    for (int c = 1; c < C; ++c) {
        if (!(s[c] <= mp)) {
            mp = s[c];
            best = c;
            if (mp != mp) break;
        }
    }
    return best;
}

// The block's counters of the run's user: flush() where the tables change hands
// (every thread calls it behind a barrier that ends the previous run's bumps; a
// barrier follows before the next run's), and last() after the walk.
struct ScoreCounts {
    int* lcm;  // [C * C] in LDS
    unsigned long long* cm;
    int CC, cur;
    __device__ __forceinline__ void flush(int u) {
        if ((int)threadIdx.x < CC) {
            const int v = lcm[threadIdx.x];
            if (cur >= 0 && v) atomicAdd(cm + (int64_t)cur * CC + threadIdx.x, (unsigned long long)v);
            lcm[threadIdx.x] = 0;
        }
        cur = u;
    }
    __device__ __forceinline__ void last() {
        __syncthreads();  // block-uniform: the walk's returns are
        if (cur >= 0 && (int)threadIdx.x < CC) {
            const int v = lcm[threadIdx.x];
            if (v) atomicAdd(cm + (int64_t)cur * CC + threadIdx.x, (unsigned long long)v);
        }
    }
};

// One frame's outputs from the lanes of its 8-lane group: every lane holds the
// same s[0 .. NS) and pred.  Lane 0 counts and writes pred, lane j < NS column j.
template <int N>
__device__ __forceinline__ void score_store(const ScoreOut& o, int* lcm, int C, bool act, int64_t row, int j,
                                            const double (&s)[N], int NS, int pred) {
    if (!act) return;
    const int yv = o.y[row];
    if (yv < 0 || yv >= C) return;
    if (j == 0) {
        atomicAdd(lcm + yv * C + pred, 1);
        if (o.pred) o.pred[row] = pred;
    }
    if (o.scores && j < NS) {
        double v = s[0];
        for (int c = 1; c < NS; ++c)
            if (c == j) v = s[c];
        o.scores[row * o.lds + j] = v;
    }
}

// GaussianNB, 8 lanes per frame, one model per user: k_gnb_proba_users up to the jll.
template <int NX, int DF>
__global__ __launch_bounds__(256) void k_gnb_score_users(GnbArgs a, UsersGeom ug, PwPlan pl, ScoreOut o) {
    extern __shared__ __attribute__((aligned(16))) double msm[];
    __shared__ double hs1[kMaxMemberC];
    __shared__ int lcm[kMaxMemberC * kMaxMemberC];
    const int CD = a.C * a.D;
    double* th = msm;
    double* vr = msm + CD;
    double* rv = msm + 2 * CD;
    const int lane = threadIdx.x & 63, j = lane & 7, g = lane >> 3, w = threadIdx.x >> 6;
    const double* lp = a.log_prior;
    ScoreCounts cnt{lcm, o.cm, a.C * a.C, -1};
    auto stage = [&](int u) {
        __syncthreads();  // the previous user's frames are done with the tables and the counters
        cnt.flush(u);
        const double* tu = a.theta + (int64_t)u * CD;
        const double* vu = a.var + (int64_t)u * CD;
        for (int t = threadIdx.x; t < CD; t += blockDim.x) {
            th[t] = tu[t];
            vr[t] = vu[t];
            rv[t] = 1.0 / vu[t];
        }
        __syncthreads();
        if (w * 8 < a.C) {  // wave-uniform: the waves holding groups 0..C-1
            const int gid = w * 8 + g, c = gid < a.C ? gid : 0;
            double t[NX];
#pragma unroll
            for (int m = 0; m < NX; ++m) {
                const int f = 8 * m + j;
                t[m] = f < a.D ? glog(2. * M_PI * vr[c * a.D + f]) : 0.0;
            }
            const double s1 = group_sum<NX, DF>(t, pl);
            if (gid < a.C && j == 0) hs1[gid] = -0.5 * s1;
        }
        lp = a.log_prior + (int64_t)u * a.C;
        __syncthreads();
    };
    auto frames = [&](bool act, int64_t row) {
        double x[NX];
#pragma unroll
        for (int m = 0; m < NX; ++m) {
            const int f = 8 * m + j;
            x[m] = (act && f < a.D) ? a.X[row * a.ld + f] : 0.0;
        }
        double jll[kMaxMemberC];
        for (int c = 0; c < a.C; ++c) {
            double t[NX];
#pragma unroll
            for (int m = 0; m < NX; ++m) {
                const int f = 8 * m + j, fc = f < a.D ? f : 0;
                const double d = x[m] - th[c * a.D + fc];
                t[m] = f < a.D ? div_by_recip(d * d, vr[c * a.D + fc], rv[c * a.D + fc]) : 0.0;
            }
            const double s2 = group_sum<NX, DF>(t, pl);
            double n_ij = hs1[c];
            n_ij -= 0.5 * s2;
            jll[c] = lp[c] + n_ij;
        }
        score_store(o, lcm, a.C, act, row, j, jll, a.C, np_argmax(jll, a.C));
    };
    users_walk(ug, a.F, stage, frames);
    cnt.last();
}

// GaussianNB for the reference's shape (D = ld = 260, KC classes): the feature-
// streamed frame loop of k_gnb_users260 up to the jll.
template <int KC, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE))) void k_gnb_score_users260(GnbArgs a,
                                                                                                       UsersGeom ug,
                                                                                                       ScoreOut o) {
    constexpr int D = 260, NX = 33;
    static_assert(pw_plan(D).nleaves == 3 && pw_plan(D).lstart[1] == 128 && pw_plan(D).lstart[2] == 192 &&
                      pw_plan(D).llen[2] == 68,
                  "the leaf layout this kernel hard-codes");
    __shared__ __attribute__((aligned(16))) f64x2 tr[KC * D];  // {theta, RN(1/var)}
    __shared__ double vr[KC * D];
    __shared__ double lgv[KC * D];  // log(2 pi var): every thread computes its share, wave 0 sums them
    __shared__ double hs1[KC], lpr[KC];
    __shared__ int lcm[KC * KC];
    const int lane = threadIdx.x & 63, j = lane & 7, g = lane >> 3;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: the group positions stay scalar
    ScoreCounts cnt{lcm, o.cm, KC * KC, -1};
    auto stage = [&](int u) {
        __syncthreads();  // the previous user's frames are done with the tables and the counters
        cnt.flush(u);
        const double* tu = a.theta + (int64_t)u * KC * D;
        const double* vu = a.var + (int64_t)u * KC * D;
#pragma unroll 1  // one log live at a time: the run's first group (x) is in registers across the restage
        for (int t = threadIdx.x; t < KC * D; t += blockDim.x) {
            const double v = vu[t];
            tr[t] = f64x2{tu[t], 1.0 / v};
            vr[t] = v;
            lgv[t] = glog(2. * M_PI * v);
        }
        if (threadIdx.x < KC) lpr[threadIdx.x] = a.log_prior[(int64_t)u * KC + threadIdx.x];
        __syncthreads();
        if (w == 0) {  // -0.5 * np.sum(np.log(2 pi var_c)): group c < KC sums class c, leaf by leaf
            const int c = g < KC ? g : 0;
            const double* v = lgv + c * D + j;
            auto lg = [&](int m) { return v[8 * m]; };
            double L[3];
            const int m0[3] = {0, 16, 24}, m1[3] = {16, 24, 32};
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                double r = lg(m0[l]);
#pragma unroll 1
                for (int m = m0[l] + 1; m < m1[l]; ++m) r += lg(m);
                r = r + __shfl_xor(r, 1);
                r = r + __shfl_xor(r, 2);
                r = r + __shfl_xor(r, 4);
                L[l] = r;
            }
            const double tl = j < 4 ? lg(32) : 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) L[2] += __shfl(tl, (lane & ~7) + k);
            const double s1 = 0.0 + (L[0] + (L[1] + L[2]));
            if (g < KC && j == 0) hs1[g] = -0.5 * s1;
        }
        __syncthreads();
    };
    int64_t s0 = 0, s1 = 0, q0 = 0, row = 0;  // the run's songs; the wave's current group and this lane's frame in it
    bool act = false;
    double x[NX];
    // the wave's next group at or after q with a frame to compute (q >= e: none left)
    auto next = [&](int64_t& q, int64_t e, bool& ac, int64_t& ro) {
        for (;; q += 32) {
            ro = 0;
            ac = users_frame(ug, a.F, s0, s1, q + g, e, ro);
            if (!ac) ro = 0;  // a valid row to load (F > 0), never stored
            if (q >= e || __ballot(ac) != 0) return;
        }
    };
    // the run's first group: its loads are in flight while the tables are restaged
    auto pre = [&](int u, int64_t p, int64_t e) {
        s0 = ug.item_offsets[u], s1 = ug.item_offsets[u + 1];
        q0 = p + w * 8;
        next(q0, e, act, row);
        if (q0 >= e) return;  // wave-uniform
        const double* xr = a.X + row * a.ld;
#pragma unroll
        for (int m = 0; m < NX; ++m) x[m] = (m < NX - 1 || j < 4) ? __builtin_nontemporal_load(xr + 8 * m + j) : 0.0;
    };
    auto run = [&](int, int64_t, int64_t e) {
        while (q0 < e) {
            int64_t qn = q0 + 32, rown;
            bool actn;
            next(qn, e, actn, rown);
            const double* xn = a.X + rown * a.ld;
            // as in k_gnb_stream260: an opaque per-iteration base keeps the table reads in their column
            int jo = j;
            asm volatile("" : "+v"(jo));
            double r[KC][3], tl[KC];
#pragma unroll
            for (int m = 0; m < NX; ++m) {
                const bool live = m < NX - 1 || j < 4;  // column 32: features 256..259 only
                const double xm = x[m];
                if (live) x[m] = __builtin_nontemporal_load(xn + 8 * m + j);
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    const int fc = live ? c * D + 8 * m + jo : c * D;
                    const f64x2 pr = tr[fc];
                    const double d = xm - pr.x;
                    const double t = live ? div_by_recip(d * d, vr[fc], pr.y) : 0.0;
                    if (m == 0 || m == 16 || m == 24) r[c][m == 0 ? 0 : (m == 16 ? 1 : 2)] = t;
                    else if (m < 16) r[c][0] += t;
                    else if (m < 24) r[c][1] += t;
                    else if (m < 32) r[c][2] += t;
                    else tl[c] = t;
                    if constexpr (WPE >= 4) asm volatile("" ::: "memory");
                }
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    if (m < 16) asm volatile("" : "+v"(r[c][0]));
                    else if (m < 24) asm volatile("" : "+v"(r[c][1]));
                    else if (m < 32) asm volatile("" : "+v"(r[c][2]));
                    else asm volatile("" : "+v"(tl[c]));
                }
                asm volatile("" ::: "memory");
            }
            double jll[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                double L[3];
#pragma unroll
                for (int l = 0; l < 3; ++l) {
                    double v = r[c][l];
                    v = v + __shfl_xor(v, 1);
                    v = v + __shfl_xor(v, 2);
                    v = v + __shfl_xor(v, 4);
                    L[l] = v;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) L[2] += __shfl(tl[c], (lane & ~7) + k);
                const double s2 = 0.0 + (L[0] + (L[1] + L[2]));
                double n_ij = hs1[c];
                n_ij -= 0.5 * s2;
                jll[c] = lpr[c] + n_ij;
            }
            score_store(o, lcm, KC, act, row, j, jll, KC, np_argmax(jll, KC));
            q0 = qn, act = actn, row = rown;
        }
    };
    users_runs(ug, pre, stage, run);
    cnt.last();
}

// SGDClassifier, 8 lanes per frame, one model per user: k_sgd_proba_users up to
// the decision values.  LDS: the staged user's coef [K][D], then its intercept [K].
template <int NX>
__global__ __launch_bounds__(256) void k_sgd_score_users(SgdArgs a, UsersGeom ug, ScoreOut o) {
    extern __shared__ __attribute__((aligned(16))) double msm[];
    __shared__ int lcm[kMaxMemberC * kMaxMemberC];
    const int KD = a.K * a.D;
    double* ic = msm + KD;
    const int lane = threadIdx.x & 63, j = lane & 7;
    ScoreCounts cnt{lcm, o.cm, a.C * a.C, -1};
    auto stage = [&](int u) {
        __syncthreads();  // the previous user's frames are done with the table and the counters
        cnt.flush(u);
        const double* cu = a.coef + (int64_t)u * KD;
        for (int t = threadIdx.x; t < KD; t += blockDim.x) msm[t] = cu[t];
        if ((int)threadIdx.x < a.K) ic[threadIdx.x] = a.intercept[(int64_t)u * a.K + threadIdx.x];
        __syncthreads();
    };
    auto frames = [&](bool act, int64_t row) {
        double x[NX];
#pragma unroll
        for (int m = 0; m < NX; ++m) {
            const int f = 8 * m + j;
            x[m] = (act && f < a.D) ? a.X[row * a.ld + f] : 0.0;
        }
        double s[kMaxMemberC];
        for (int c = 0; c < a.K; ++c) {
            double d = 0.0;
#pragma unroll
            for (int m = 0; m < NX; ++m) {
                const int f = 8 * m + j;
                if (f < a.D) d = fma(x[m], msm[c * a.D + f], d);
            }
            d = d + __shfl_xor(d, 1);  // sgd_expit's argument: the group's butterfly, then the intercept
            d = d + __shfl_xor(d, 2);
            d = d + __shfl_xor(d, 4);
            d += ic[c];
            s[c] = d;
        }
        const int pred = a.K == 1 ? (s[0] > 0.0 ? 1 : 0) : np_argmax(s, a.K);
        score_store(o, lcm, a.C, act, row, j, s, a.K, pred);
    };
    users_walk(ug, a.F, stage, frames);
    cnt.last();
}

// sklearn 1.7.2's f1_score(y_true, y_pred, average='weighted') from one user's
// counts, one thread per user.  true_c = sum_p cm[c, p], pred_c = sum_y cm[y, c],
// tp_c = cm[c, c] (integer sums); a class is present iff true_c + pred_c > 0
// (unique_labels(y_true, y_pred)); f_c = (2 tp_c) / (true_c + pred_c); the terms
// f_c * true_c of the present classes, ascending, are added one after the other
// onto 0.0 (fewer than 8) or by numpy's 8-accumulator tree (8 of them), and the
// sum is divided by sum_c true_c.  A user without a counted row gets NaN.
// prf_or_null [U, C, 4]: precision, recall, f_c, support (0.0 on a zero
// denominator; zeros for an absent class).
__global__ __launch_bounds__(256) void k_f1_weighted_users(const long long* __restrict__ cm, int U, int C,
                                                           double* __restrict__ f1, double* __restrict__ prf) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= U) return;
    const long long* m = cm + (int64_t)u * C * C;
    double t[kMaxMemberC];
    int n = 0;
    long long total = 0;
    for (int c = 0; c < C; ++c) {
        long long tc = 0, pc = 0;
        for (int k = 0; k < C; ++k) {
            tc += m[c * C + k];
            pc += m[k * C + c];
        }
        const long long tp = m[c * C + c];
        total += tc;
        double f = 0.0;
        if (tc + pc > 0) {
            f = (2.0 * (double)tp) / ((double)tc + (double)pc);
            t[n++] = f * (double)tc;
        }
        if (prf) {
            double* o = prf + ((int64_t)u * C + c) * 4;
            o[0] = pc > 0 ? (double)tp / (double)pc : 0.0;
            o[1] = tc > 0 ? (double)tp / (double)tc : 0.0;
            o[2] = f;
            o[3] = (double)tc;
        }
    }
    double s = 0.0;
    if (n == 8) {
        s = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
    } else {
        for (int i = 0; i < n; ++i) s += t[i];
    }
    f1[u] = total > 0 ? s / (double)total : __builtin_nan("");
}

}  // namespace ce
