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
// The score kernels are the users form of mod.predict over the geometry of the
// TEST songs.  k_gnb_score_users260 and k_sgd_score_users ARE the bodies of
// ce_members_users.hpp (gnb_users260, sgd_users8: the walk, the staging, the
// per-frame jll / decision values) with the score finish below in place of the
// proba finish, so their scores are the values the proba kernels form before
// their logsumexp / expit, from the same text.  k_gnb_score_users (the general
// GaussianNB form) is a kernel of its own over k_gnb_proba_users' functions
// (gnb_stage8, gnb_jll8 of ce_members.hpp) and its x[] load.  predict is the argmax of THOSE values (not of the rounded
// probabilities): np.argmax's rule (the first maximum; a NaN wins at its first
// occurrence), and score > 0 for a binary SGD model (NaN: class 0).
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

// The score finish of the users bodies (ce_members_users.hpp): the counters are
// flushed where the tables change hands and once more after the walk, and a
// frame's values are labelled by np.argmax and stored.
struct ScoreFin {
    ScoreOut o;
    ScoreCounts cnt;
    int C;
    __device__ __forceinline__ void restage(int u) { cnt.flush(u); }
    __device__ __forceinline__ void done() { cnt.last(); }
    template <int N>
    __device__ __forceinline__ void frame(const double (&s)[N], int n, bool act, int64_t row) {
        score_store(o, cnt.lcm, C, act, row, threadIdx.x & 7, s, n, np_argmax(s, n));
    }
};

// SGD: a binary model (K = 1 decision value) predicts class 1 where it is > 0 (NaN: class 0).
struct SgdScoreFin : ScoreFin {
    __device__ __forceinline__ double value(double d) { return d; }
    __device__ __forceinline__ void frame(const double (&s)[kMaxMemberC], int K, bool act, int64_t row) {
        const int pred = K == 1 ? (s[0] > 0.0 ? 1 : 0) : np_argmax(s, K);
        score_store(o, cnt.lcm, C, act, row, threadIdx.x & 7, s, K, pred);
    }
};

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
    const int lane = threadIdx.x & 63, j = lane & 7;
    const double* lp = a.log_prior;
    ScoreCounts cnt{lcm, o.cm, a.C * a.C, -1};
    auto stage = [&](int u) {
        __syncthreads();  // the previous user's frames are done with the tables and the counters
        cnt.flush(u);
        gnb_stage8<NX, DF>(th, vr, rv, hs1, a.theta + (int64_t)u * CD, a.var + (int64_t)u * CD, a.C, a.D, pl);
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
        gnb_jll8<NX, DF>(jll, x, th, vr, rv, hs1, lp, a.C, a.D, pl);
        score_store(o, lcm, a.C, act, row, j, jll, a.C, np_argmax(jll, a.C));
    };
    users_walk(ug, a.F, stage, frames);
    cnt.last();
}

template <int KC, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE))) void k_gnb_score_users260(GnbArgs a,
                                                                                                       UsersGeom ug,
                                                                                                       ScoreOut o) {
    __shared__ int lcm[KC * KC];
    ScoreFin fin{o, {lcm, o.cm, KC * KC, -1}, KC};
    gnb_users260<KC, WPE>(a, ug, fin);
}

template <int NX>
__global__ __launch_bounds__(256) void k_sgd_score_users(SgdArgs a, UsersGeom ug, ScoreOut o) {
    __shared__ int lcm[kMaxMemberC * kMaxMemberC];
    SgdScoreFin fin{{o, {lcm, o.cm, a.C * a.C, -1}, a.C}};
    sgd_users8<NX>(a, ug, fin);
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
