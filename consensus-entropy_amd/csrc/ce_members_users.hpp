// ce_members_users.hpp -- the users form of the linear members' predict_proba
// (SURVEY.md §8(f)5): after the retrain kernels (ce_gnb_fit.hpp, ce_sgd_fit.hpp)
// every user has a model of their own, and the predict step of the epoch
// (amg_test.py:435) has every frame row predicted by the model of the user who
// owns it -- one launch per member for all users.
//
// The geometry is the sessions' (frame_geometry): stacked song g owns the CSR
// positions frame_offsets[g] .. frame_offsets[g+1] (position p is row
// frame_perm[p] of X, or row p), user u the stacked songs item_offsets[u] ..
// item_offsets[u+1], so user u owns the contiguous run of positions
// first(u) .. first(u+1), first(u) = frame_offsets[item_offsets[u]].  The
// kernels walk POSITIONS: block b takes an equal, contiguous share of them
// (a multiple of 32: 4 waves x 8 frames), cuts it at the users' boundaries
// (a search over first(), read straight from the two offset arrays: no
// derived table, nothing read back) and stages one user's parameters in LDS at
// a time, restaging at a block-wide barrier when the share crosses into the
// next user.  A wave's 8 frames are 8 consecutive positions of ONE user.
//
// The GaussianNB 260 form and SGD are one body each: the walk with that
// family's staging and per-frame values, templated on a finish that says what
// is done with the values.  Their proba kernels here and their score kernels in
// ce_members_score.hpp are the same body with two finishes, so the scores are
// the proba kernels' intermediates bit for bit by construction.  The general
// GaussianNB form (k_gnb_proba_users, k_gnb_score_users) is two kernels.
// Against the one-model kernels (ce_members.hpp): the 8-lane staging, jll and
// proba finish and SGD's decision value are the same functions; the 8-lane
// x[] load and the 260 form restate the one-model kernels' text, and the tests
// hold the two to the same bits.
//
// A position whose row is outside [0, F) is neither read nor written; with an
// exclusion bitmap over the stacked songs, the rows of an excluded song are
// never written, and a wave whose 8 frames are all excluded (or out of range)
// skips their loads and arithmetic.
#pragma once
#include "ce_members.hpp"

namespace ce {

struct UsersGeom {
    const int64_t* item_offsets;   // [U + 1]: user u's stacked songs
    const int64_t* frame_offsets;  // [T + 1]: song g's CSR positions
    const int64_t* frame_perm;     // position -> row of X, or nullptr (the position is the row)
    const uint32_t* excl;          // bitmap over the stacked songs, or nullptr
    int U;
};

// first CSR position of user u (u = U: one past the last user's)
__device__ __forceinline__ int64_t users_first(const UsersGeom& g, int u) {
    return g.frame_offsets[g.item_offsets[u]];
}

// This lane's frame at position q of a run ending at e (user's songs s0 .. s1):
// false when q is past the run, its row is outside [0, F) or its song is
// excluded; row: the row of X (valid only when true).
__device__ __forceinline__ bool users_frame(const UsersGeom& ug, int64_t F, int64_t s0, int64_t s1, int64_t q,
                                            int64_t e, int64_t& row) {
    if (q >= e) return false;
    row = ug.frame_perm ? ug.frame_perm[q] : q;
    if (row < 0 || row >= F) return false;
    if (!ug.excl) return true;
    int64_t lo = s0, hi = s1;  // the song owning q: frame_offsets[lo] <= q < frame_offsets[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (ug.frame_offsets[mid] <= q) lo = mid;
        else hi = mid;
    }
    return !((ug.excl[lo >> 5] >> (lo & 31)) & 1u);
}

// The walk every kernel shares: the block's share of the positions, cut into
// runs of one user.  For the run of user u at positions p .. e: pre(u, p, e)
// (what can be issued before the tables change hands: the first loads),
// stage(u) (user u's parameters into LDS; it owns its barriers, every thread
// of the block calls it), then run(u, p, e) (the frames; no barrier inside).
// ROUND: what a share is a multiple of (the linear members' pass of 4 waves x 8
// frames; the XGBoost member's 64-frame tile, ce_xgb_users.hpp).
template <int ROUND = 32, class Pre, class Stage, class Run>
__device__ __forceinline__ void users_runs(const UsersGeom& ug, Pre&& pre, Stage&& stage, Run&& run) {
    const int64_t pb = users_first(ug, 0), pe = users_first(ug, ug.U);
    int64_t per = (pe - pb + gridDim.x - 1) / gridDim.x;
    per = (per + ROUND - 1) & ~(int64_t)(ROUND - 1);
    int64_t p = pb + (int64_t)blockIdx.x * per;
    const int64_t p1 = p + per < pe ? p + per : pe;
    if (p >= p1) return;  // block-uniform
    // the user owning p: first(u) <= p < first(hi).  Every wave searches on its
    // own, 64 candidates a round (a probe is two dependent loads: two rounds up
    // to 4096 users instead of a dozen bisection steps)
    int u = 0;
    for (int hi = ug.U; hi - u > 1;) {
        const int step = (hi - u + 63) >> 6;
        const int cand = u + (int)(threadIdx.x & 63) * step;
        const bool le = cand < hi && users_first(ug, cand) <= p;
        const int k = 63 - __builtin_clzll(__ballot(le) | 1ull);  // lanes 0 .. k: first() ascends
        u += k * step;
        hi = hi < u + step ? hi : u + step;
    }
    while (p < p1) {  // block-uniform: one run of one user per turn
        int64_t ue = users_first(ug, u + 1);
        while (ue <= p && u + 1 < ug.U) ue = users_first(ug, ++u + 1);  // users without a frame
        const int64_t e = ue < p1 ? ue : p1;
        if (e <= p) return;  // offsets that do not ascend: no run to take (block-uniform)
        pre(u, p, e);
        stage(u);
        run(u, p, e);
        p = e;
    }
}

// users_runs with a run taken one 8-frame group per wave at a time.
// frames(act, row): this lane's frame (8 lanes each); row is 0 where !act.
template <class Stage, class Frames>
__device__ __forceinline__ void users_walk(const UsersGeom& ug, int64_t F, Stage&& stage, Frames&& frames) {
    const int lane = threadIdx.x & 63, g = lane >> 3, w = threadIdx.x >> 6;
    users_runs(ug, [](int, int64_t, int64_t) {}, stage, [&](int u, int64_t p, int64_t e) {
        const int64_t s0 = ug.item_offsets[u], s1 = ug.item_offsets[u + 1];
        for (int64_t q0 = p + w * 8; q0 < e; q0 += 32) {
            int64_t row = 0;
            const bool act = users_frame(ug, F, s0, s1, q0 + g, e, row);
            if (__ballot(act) == 0) continue;  // wave-uniform: nothing to load, compute or store
            frames(act, act ? row : 0);
        }
    });
}

// ---- what the score finishes share (ce_members_score.hpp, ce_xgb_users.hpp) ----
// np.argmax over s[0 .. C): the first maximum; a NaN wins at its first occurrence
template <class T, int N>
__device__ __forceinline__ int np_argmax(const T (&s)[N], int C) {
    int best = 0;
    T mp = s[0];
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

// ---- the kernels' bodies -------------------------------------------------------
// A body is the walk with one family's staging and per-frame values; what is
// done with the values is its finish `fin`, a small struct of three hooks:
//   fin.restage(u)             the tables are about to change hands to user u (every
//                              thread, behind the barrier that ends the previous run)
//   fin.frame(s, n, act, row)  one frame's n values s[] -- GaussianNB: the jll, SGD:
//                              the decision values -- in every lane of its 8-lane group
//   fin.done()                 after the walk (every thread of the block)
// SGD's finish has a fourth, fin.value(d): what of a decision value goes into
// s[] -- its expit (proba) or itself (score).  It is taken class by class
// inside the loop, as k_sgd_proba8 does: a frame() that applies expit to the
// whole s[] afterwards compiles to another register count (20 VGPRs off) for
// every k_sgd_proba_users<NX>.

// GaussianNB for the reference's shape (D = 260, KC = C classes), one model per
// user: k_gnb_stream260's feature-streamed frame loop (ce_members.hpp -- the
// column loop outermost, each term straight into its numpy accumulator, the
// register x[m] refilled with the wave's NEXT group as soon as it is consumed)
// inside a run of one user.  The next group is the wave's next one WITH a frame
// to compute (excluded groups are stepped over before anything is loaded); past
// the run's end the refill reads row 0, and the first group of the next run
// loads afresh after the restage.
template <int KC, int WPE, class Fin>
__device__ __forceinline__ void gnb_users260(const GnbArgs& a, const UsersGeom& ug, Fin& fin) {
    constexpr int D = kD260, NX = kNX260;
    __shared__ __attribute__((aligned(16))) f64x2 tr[KC * D];  // {theta, RN(1/var)}
    __shared__ double vr[KC * D];
    __shared__ double lgv[KC * D];  // log(2 pi var): every thread computes its share, wave 0 sums them
    // the user's log-prior sits in LDS too: read from global memory inside the frame loop, its wait
    // would also wait for the next group's loads, which are queued before it
    __shared__ double hs1[KC], lpr[KC];
    const int lane = threadIdx.x & 63, j = lane & 7, g = lane >> 3;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: the group positions stay scalar
    auto stage = [&](int u) {
        __syncthreads();  // the previous user's frames are done with the tables
        fin.restage(u);
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
        if (w == 0) {  // -0.5 * np.sum(np.log(2 pi var_c)): group c < KC sums class c
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
            fin.frame(jll, KC, act, row);
            q0 = qn, act = actn, row = rown;
        }
    };
    users_runs(ug, pre, stage, run);
    fin.done();
}

// SGDClassifier(loss='log'), 8 lanes per frame, one model per user: a.coef
// [U, K, D], a.intercept [U, K].  LDS: the staged user's coef [K][D], then its
// intercept [K].
template <int NX, class Fin>
__device__ __forceinline__ void sgd_users8(const SgdArgs& a, const UsersGeom& ug, Fin& fin) {
    extern __shared__ __attribute__((aligned(16))) double msm[];
    const int KD = a.K * a.D;
    double* ic = msm + KD;
    const int lane = threadIdx.x & 63, j = lane & 7;
    auto stage = [&](int u) {
        __syncthreads();  // the previous user's frames are done with the table
        fin.restage(u);
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
        double d[kMaxMemberC];
        for (int c = 0; c < a.K; ++c) d[c] = fin.value(sgd_decision8(x, msm, ic, c, a.D));
        fin.frame(d, a.K, act, row);
    };
    users_walk(ug, a.F, stage, frames);
    fin.done();
}

// ---- the proba finishes and their kernels ---------------------------------------
struct NoCounts {  // nothing to do at a restage or after the walk
    __device__ __forceinline__ void restage(int) {}
    __device__ __forceinline__ void done() {}
};

struct GnbProbaFin260 : NoCounts {
    double* out;
    int64_t ldo;
    template <int KC>
    __device__ __forceinline__ void frame(const double (&jll)[KC], int, bool act, int64_t row) {
        const int j = threadIdx.x & 7;
        double mx = jll[0];
#pragma unroll
        for (int c = 1; c < KC; ++c) mx = jll[c] > mx ? jll[c] : mx;
        if (!__builtin_isfinite(mx)) mx = 0.0;
        // one transcendental at a time, as in k_gnb_stream260
        double s = -0.0;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            s += gexp(jll[c] - mx);
            asm volatile("" : "+v"(s));
        }
        const double lse = glog(0.0 + s) + mx;
        if (act && j < KC) {
            double jl = jll[0];
#pragma unroll
            for (int c = 1; c < KC; ++c)
                if (c == j) jl = jll[c];
            out[row * ldo + j] = gexp(jl - lse);  // lane j's class only
        }
    }
};

struct SgdProbaFin : NoCounts {
    const SgdArgs& a;
    __device__ __forceinline__ double value(double d) { return expit(d); }
    __device__ __forceinline__ void frame(double (&d)[kMaxMemberC], int K, bool act, int64_t row) {
        sgd_store(a, d, K, act ? row : a.F, threadIdx.x & 7);  // row F: no store
    }
};

// The general GaussianNB form is not a body with a finish: k_gnb_proba_users here
// and k_gnb_score_users (ce_members_score.hpp) are two kernels over the same
// functions of ce_members.hpp (gnb_stage8, gnb_jll8).
// GaussianNB, 8 lanes per frame, one model per user: a.theta / a.var [U, C, D],
// a.log_prior [U, C].  LDS as k_gnb_proba8: theta, var, 1/var [C][D] and the
// per-class -0.5 * np.sum(np.log(2 pi var_c)) of the staged user.
template <int NX, int DF>  // DF: the feature count when fixed at compile time (0: a.D, runtime plan)
__global__ __launch_bounds__(256) void k_gnb_proba_users(GnbArgs a, UsersGeom ug, PwPlan pl) {
    extern __shared__ __attribute__((aligned(16))) double msm[];
    __shared__ double hs1[kMaxMemberC];
    const int CD = a.C * a.D;
    double* th = msm;
    double* vr = msm + CD;
    double* rv = msm + 2 * CD;
    const int lane = threadIdx.x & 63, j = lane & 7;
    const double* lp = a.log_prior;
    auto stage = [&](int u) {
        __syncthreads();  // the previous user's frames are done with the tables
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
        gnb_proba8(jll, a.C, act, a.out, a.ldo, row);
    };
    users_walk(ug, a.F, stage, frames);
}

template <int KC, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE))) void k_gnb_users260(GnbArgs a, UsersGeom ug) {
    GnbProbaFin260 fin{{}, a.out, a.ldo};
    gnb_users260<KC, WPE>(a, ug, fin);
}

template <int NX>
__global__ __launch_bounds__(256) void k_sgd_proba_users(SgdArgs a, UsersGeom ug) {
    SgdProbaFin fin{{}, a};
    sgd_users8<NX>(a, ug, fin);
}

}  // namespace ce
