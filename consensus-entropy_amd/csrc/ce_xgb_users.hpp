// ce_xgb_users.hpp -- the users form of the XGBoost member (SURVEY.md §8(f)5b /
// 5c): after epoch 0 every user's forest is the shared pretrained trees plus
// the rounds that user's own mod.fit(xgb_model=) appended (amg_test.py:507),
// and every later predict_proba(X_train) (:435, :467) and predict(X_test)
// (:513) has each frame row predicted by the forest of the user who owns it --
// one launch for all users.
//
// Many forests over one lane table: `table` [2][TT][64] holds TT perfect trees
// of one depth (ce_xgb_lane_table's format: the shared base trees once, then
// every user's own), tree_ids [L] names a table row per logical tree, and
// group_offsets [U * G + 1] is a CSR over tree_ids: user u's group g owns the
// logical trees tree_ids[group_offsets[u G + g] .. group_offsets[u G + g + 1]),
// in the order the reference adds them to preds[g].  So user u's forest is a
// forest of ce_xgb_walk.hpp whose goff is group_offsets + u G, and the margin
// chain (split_margins: the wave split, the ordered phases) is that header's
// text over the layout UsersForest below.
//
// The geometry is the sessions' (UsersGeom, ce_members_users.hpp).  A block
// takes a contiguous share of the CSR positions (a multiple of the 64-frame
// tile), cuts it at the users' boundaries (users_runs) and walks one tile
// after another: a tile is up to 64 consecutive positions of ONE user, so
// every forest read of the walk is wave-uniform.  A position whose row is
// outside [0, F) is neither read nor written, the rows of an excluded song are
// never written, and a tile whose positions are all excluded or out of range
// is skipped before its loads.  Every load of the staging is unconditional: an
// inactive slot of a tile loads the row of the tile's first active slot (a
// valid row, and no missing value the tile does not hold) and is never stored.
//
// Against the one-forest kernels nothing of the arithmetic is stated here a
// second time: the staging (stage_rows, stage_rows_pairs: ce_xgb.hpp) takes the
// tile's rows through a functor, the walk (table_walk8: ce_xgb_walk.hpp) the
// table row of a logical tree through UsersForest::row, and the probabilities
// are xgb_proba's (ce_xgb.hpp).  This header holds what differs: the geometry,
// the tile's rows and the finishes.
#pragma once
#include <algorithm>

#include "ce_members_users.hpp"  // UsersGeom, users_runs, users_frame, ScoreCounts, np_argmax
#include "ce_xgb_walk.hpp"

namespace ce {

// Lane tables read through tree_ids: LaneTableForest with logical tree k at
// table row ids[k] (a wave-uniform scalar load; the debug build checks < TT).
struct UsersForest : XgbGeom {
    const uint2* table;     // [TT][64], fx with default_left in bit 31
    const uint2* table_nd;  // [TT][64], fx without it
    const int32_t* ids;     // [L]
    int TT;

    __device__ __forceinline__ int64_t row(int k) const {
        CE_DASSERT(k >= 0 && k < goff_end);
        const int t = ids[k];
        CE_DASSERT(t >= 0 && t < TT);
        return (int64_t)t * 64;
    }
    template <bool MISS, bool VALS>
    __device__ __forceinline__ void walk8(const float* xs, int D, int t0, int t1, int lane, int (&li)[8],
                                          float (&v)[8]) const {
        (void)D;
        table_walk8<MISS, VALS>(*this, MISS ? table : table_nd, xs, t0, t1, lane, li, v);
    }
    __device__ __forceinline__ float value(int t, int li) const {
        CE_DASSERT(li >= 0 && li <= NI);
        return __uint_as_float(table[row(t) + NI + 1 + li].y);
    }
};

struct XgbUsersForests {
    const uint2* table;    // [2][TT][64]
    const int32_t* ids;    // [L]
    const int32_t* goff;   // [U * G + 1]
    int TT, depth;
    int64_t L;
};

// lane l's value of v, l wave-uniform
__device__ __forceinline__ int64_t readlane64(int64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// dynamic LDS: the one-forest kernels' tile (xs, mg, the missing-value votes:
// ce_xgb_lds_bytes), then the tile's rows [64] and the score finish's counters
constexpr int kXgbUsersExtraLds = 64 * (int)sizeof(int64_t) + kXgbMaxGroups * kXgbMaxGroups * (int)sizeof(int);

// A finish that declares `using takes_margins = void` is handed the margins
// themselves, before the objective's transform (the fit's start margins,
// ce_xgb_fit.hpp): fin.margins(mg, G, lane, q) for the frame at CSR position q.
template <class Fin, class = void>
struct fin_takes_margins : std::false_type {};
template <class Fin>
struct fin_takes_margins<Fin, typename Fin::takes_margins> : std::true_type {};

// The body: the users walk, one tile after another, with a finish `fin`:
//   fin.restage(u)      the block moves to user u (every thread, behind a barrier)
//   fin.row(p, C, row)  one frame's probabilities (wave 0, the lane of the frame)
//   fin.done()          after the walk (every thread of the block)
template <int XDT, int KF, class Fin>
__device__ __forceinline__ void xgb_users(const XgbArgs& a, const XgbUsersForests& f, const UsersGeom& ug, Fin& fin) {
    extern __shared__ float xsm[];
    float* xs = xsm;                  // [D][kXgbCol] swizzled
    float* mg = xsm + a.D * kXgbCol;  // [G][64] margins
    uint32_t* nanw = reinterpret_cast<uint32_t*>(mg + a.G * 64);  // [16] the tile's missing-value votes
    int64_t* rowl = reinterpret_cast<int64_t*>(nanw + 16);        // [64] the tile's rows (-1: not to be written)
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = w / a.S, s = w - g * a.S;
    CE_DASSERT(f.depth <= kXgbLaneDepth);
    auto stage = [&](int u) {
        __syncthreads();  // the previous user's frames are counted
        fin.restage(u);
    };
    auto run = [&](int u, int64_t p, int64_t e) {
        const int64_t s0 = ug.item_offsets[u], s1 = ug.item_offsets[u + 1];
        const int32_t* goff = f.goff + (int64_t)u * a.G;
#ifdef CE_DEBUG
        for (int k = 0; k < a.G; ++k) CE_DASSERT(goff[k] >= 0 && goff[k] <= goff[k + 1] && goff[k + 1] <= f.L);
#endif
        const UsersForest fl{XgbGeom{goff, f.depth, (1 << f.depth) - 1, (int)f.L}, f.table,
                             f.table + (int64_t)f.TT * 64, f.ids, f.TT};
        for (int64_t q0 = p; q0 < e; q0 += kXgbTile) {
            // every wave works out the tile's 64 frames for itself (lane = frame): the same
            // answer in every wave, so the skip is block-uniform and no barrier hands them on
            // An optimisation barrier: the compiler may not hoist what it computes from the lane
            // (the LDS addresses of the staging and the walk) out of the tile loop, where those
            // values would stay in registers across every walk.  Chosen from the compiler's
            // resource report alone, not timed: scratch per lane with / without it is 60 / 88 B
            // for the reference's shape (f64, KF = 5), lower in 21 of the 24 instantiations and
            // higher in the three f64 KF = 8 ones (profiles/xgb_users_codeobj.json).
            int lane = threadIdx.x & 63;
            asm volatile("" : "+v"(lane));
            int64_t row = 0;
            const bool act = users_frame(ug, a.F, s0, s1, q0 + lane, e, row);
            const uint64_t m = __ballot(act);
            if (m == 0) continue;  // nothing to load, walk or store
            const int64_t rows = act ? row : readlane64(row, __builtin_ctzll(m));
            // rowl, nanw and mg are free: every wave is past the previous tile's last phase barrier,
            // wave 0 (the only reader after it) past its finish
            if (w == 0) rowl[lane] = act ? row : -1;
            const auto row_of = [&](int r) { return readlane64(rows, r); };  // every lane holds the row of slot `lane`
            bool has_nan;
            if constexpr (XDT == CE_F64) {
                if (a.D >= 2)
                    has_nan = stage_rows_pairs<(KF + 1) / 2>(static_cast<const double*>(a.X), a.D, a.ld, row_of, xs, w, lane);
                else
                    has_nan = stage_rows<XDT, KF>(a.X, a.D, a.ld, row_of, xs, w, lane);
            } else {
                has_nan = stage_rows<XDT, KF>(a.X, a.D, a.ld, row_of, xs, w, lane);
            }
            {
                const bool wn = __ballot(has_nan) != 0;
                if (lane == 0) nanw[w] = wn ? 1u : 0u;
            }
            __syncthreads();
            bool any_nan = false;
            for (int k = 0; k < (int)(blockDim.x >> 6); ++k) any_nan |= nanw[k] != 0u;
            if (any_nan)
                split_margins<UsersForest, true>(a, fl, xs, mg, g, s, lane);
            else
                split_margins<UsersForest, false>(a, fl, xs, mg, g, s, lane);
            if (w == 0) {
                const int64_t ro = rowl[lane];
                if (ro >= 0) {
                    if constexpr (fin_takes_margins<Fin>::value) {
                        fin.margins(mg, a.G, lane, q0 + lane);
                    } else {
                        float pr[kXgbMaxGroups];
                        xgb_proba(mg, a.G, lane, pr);
                        fin.row(pr, a.C, ro);
                    }
                }
            }
        }
    };
    users_runs<kXgbTile>(ug, [](int, int64_t, int64_t) {}, stage, run);
    fin.done();
}

// ---- the finishes ---------------------------------------------------------------
template <int ODT>
struct XgbProbaFin : NoCounts {
    void* out;
    int64_t ldo;
    __device__ __forceinline__ void row(const float (&p)[kXgbMaxGroups], int C, int64_t ro) {
        for (int c = 0; c < C; ++c) {
            if constexpr (ODT == CE_F64)
                static_cast<double*>(out)[ro * ldo + c] = (double)p[c];
            else
                static_cast<float*>(out)[ro * ldo + c] = p[c];
        }
    }
};

struct XgbScoreOut {
    const int32_t* y;        // [F] by row of X
    unsigned long long* cm;  // [U, C, C] counts (int64), zero before the launch
    int32_t* pred;           // [F] by row of X, or nullptr
    float* proba;            // [F, C] (row pitch ldp), or nullptr
    int64_t ldp;
};

// XGBClassifier.predict's rule (xgboost/sklearn.py:981-985) on the float32
// probabilities: np.argmax of the row (multi:softprob; not of the margins), or
// p > 0.5 (binary:logistic; a NaN is class 0).
struct XgbScoreFin {
    XgbScoreOut o;
    ScoreCounts cnt;
    int G;
    __device__ __forceinline__ void restage(int u) { cnt.flush(u); }
    __device__ __forceinline__ void done() { cnt.last(); }
    __device__ __forceinline__ void row(const float (&p)[kXgbMaxGroups], int C, int64_t ro) {
        const int yv = o.y[ro];
        if (yv < 0 || yv >= C) return;
        const int pred = G == 1 ? (p[1] > 0.5f ? 1 : 0) : np_argmax(p, C);
        atomicAdd(cnt.lcm + yv * C + pred, 1);
        if (o.pred) o.pred[ro] = pred;
        if (o.proba)
            for (int c = 0; c < C; ++c) o.proba[ro * o.ldp + c] = p[c];
    }
};

// KF as k_xgb_lanes: the row's 64-feature chunks the staging loads.  The forest
// arrays are __restrict__ kernel arguments of their own: only so does the
// compiler know that the finish's stores leave them alone and keep every
// forest read of the later tiles a scalar load.
template <int XDT, int ODT, int KF>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_xgb_users(
    XgbArgs a, UsersGeom ug, const uint2* __restrict__ table, const int32_t* __restrict__ tree_ids,
    const int32_t* __restrict__ group_offsets, int TT, int depth, int64_t L) {
    XgbProbaFin<ODT> fin{{}, a.out, a.ldo};
    xgb_users<XDT, KF>(a, XgbUsersForests{table, tree_ids, group_offsets, TT, depth, L}, ug, fin);
}

template <int XDT, int KF>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_xgb_score_users(
    XgbArgs a, UsersGeom ug, XgbScoreOut o, const uint2* __restrict__ table, const int32_t* __restrict__ tree_ids,
    const int32_t* __restrict__ group_offsets, int TT, int depth, int64_t L) {
    extern __shared__ float xsm[];
    int* lcm = reinterpret_cast<int*>(xsm + a.D * kXgbCol + a.G * 64 + 16 + 128);  // behind the tile's rows
    XgbScoreFin fin{o, {lcm, o.cm, a.C * a.C, -1}, a.G};
    xgb_users<XDT, KF>(a, XgbUsersForests{table, tree_ids, group_offsets, TT, depth, L}, ug, fin);
}

}  // namespace ce

// ---- the launch shape, shared by every TU that launches this walk -------------------
// (ce_xgb_users.hip: predict and score; ce_xgb_fit.hip: the fit's start margins)
extern "C" size_t ce_xgb_lds_bytes(int32_t D, int32_t G);

namespace ce {

// waves per group: fill a 16-wave block
inline int xgb_users_splits(int G) { return std::max(1, 16 / G); }

inline size_t xgb_users_lds(int D, int G) { return ce_xgb_lds_bytes(D, G) + kXgbUsersExtraLds; }

// One block per 64 rows of X: a well-formed geometry names at most F positions,
// so a share is one tile (two where it straddles two users); the kernel divides
// the real count, which only the device knows, among the blocks launched.
inline unsigned xgb_users_grid(int64_t F) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((F + kXgbTile - 1) / kXgbTile, 1 << 20));
}

template <class K, class... Args>
inline void xgb_users_launch(K kern, int64_t F, int D, int G, int S, ce_stream_t stream, Args... args) {
    const size_t lds = xgb_users_lds(D, G);
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(xgb_users_grid(F)), dim3(64 * G * S), lds, (hipStream_t)stream, args...);
}

// f(kf) with the staging width of D as a compile-time value (k_xgb_lanes' ladder)
template <class Fn>
inline void with_kf(int D, Fn&& fn) {
    if (D <= 128) fn(std::integral_constant<int, 2>());
    else if (D <= 256) fn(std::integral_constant<int, 4>());
    else if (D <= 320) fn(std::integral_constant<int, 5>());
    else fn(std::integral_constant<int, 8>());
}

}  // namespace ce
