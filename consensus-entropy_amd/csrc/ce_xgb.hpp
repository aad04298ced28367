// ce_xgb.hpp -- on-device XGBClassifier.predict_proba (the
// 'classifier_xgb' committee member: amg_test.py:435 / :467 ->
// xgboost/sklearn.py:991-1029 -> libxgboost 1.3.3, requirements.txt:50): the
// tile layout, its staging and the objective's transform.  The forest layouts,
// the margin chain and the kernels are in ce_xgb_walk.hpp.
//
// What the reference computes (xgboost 1.3.3 CPU predictor, restated):
//   * DMatrix(X): X (f64 DataFrame values) cast to float32 (round to nearest);
//     NaN = missing (sklearn.py:1020, missing=np.nan);
//   * per row, margins preds[g] start at the base margin (base_score for
//     multi:softprob; ProbToMargin(base_score) = -logf(1/b - 1) for
//     binary:logistic) and every tree, IN MODEL ORDER, adds its leaf to the
//     margin of its group tree_info[t]: preds[g] += leaf (float32, sequential);
//   * a tree is walked from the root: missing feature -> the default child,
//     else fvalue < split_cond ? left : right (RegTree::GetNext);
//   * multi:softprob: Softmax over the row (fmaxf maximum; e_c = expf(m_c - max);
//     wsum += e_c in float32 from 0; e_c /= wsum); binary:logistic:
//     p = 1 / (1 + expf(-m)), returned as [1 - p, p] (sklearn.py:1027-1029).
//   * expf is glibc's (ce_glibc_expf.hpp).
//
// Layout (packed on the host by ce_amd.xgb.XgbForest): every tree is padded to
// a perfect binary tree of the forest's maximum depth d (an early leaf's
// subtree repeats its value, so either branch below it reaches the same leaf);
// internal node i has children 2i+1 / 2i+2.  Trees are stored group-major
// (group g owns trees [goff[g], goff[g+1]), model order kept inside a group,
// which is exactly the order the reference adds them to preds[g]).
//   nodes  [T][2^d - 1] x {feature | default_left << 31, split_cond bits}
//   leaves [T][2^d] f32
//
// Kernel (k_xgb_walk, k_xgb_lanes): one block of G x S waves per 64-frame tile.
// The tile's features are staged ONCE as float32 in LDS, feature-major [D][64]
// swizzled (lane = frame).  Each group's trees are split over S waves whose
// partial chains are joined in model order (split_margins); every wave walks 8
// trees at a time so 8 independent node-fetch -> LDS-read -> compare chains are
// in flight per lane.  Bound: those chains (latency for the gather walk, VALU
// for the lane tables: DESIGN.md §5); X bytes from HBM, D * sizeof(x) per frame,
// are read once; T * d node steps per frame.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/ce.h"
#include "ce_debug.hpp"
#include "ce_glibc_expf.hpp"

namespace ce {

constexpr int kXgbTile = 64;      // frames per block
// LDS tile: feature-major columns of 64 floats, frame r of feature f at f*64 +
// (r ^ (f & 63)) -- the XOR swizzle keeps the staging writes (consecutive
// features of one frame) conflict-free, and a column read by 64 lanes is a
// permutation of one column (conflict-free too).  Byte address of (f, lane):
// fbase(f) ^ 4*lane with fbase(f) = 256 f + 4 (f & 63).
constexpr int kXgbCol = 64;
__device__ __forceinline__ uint32_t xs_fbase(uint32_t f) { return f * 256u + ((f & 63u) << 2); }
__device__ __forceinline__ float xs_at(const float* xs, uint32_t fbase, uint32_t lane4) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(xs) + (fbase ^ lane4));
}
constexpr int kXgbMaxDepth = 10;  // packed depth limit (2^10 leaves per tree)
constexpr int kXgbLaneDepth = 5;  // lane-table walk: 2^(d+1) - 1 entries fit one wave
constexpr int kXgbMaxFeat = 512;
constexpr int kXgbMaxGroups = 8;

struct XgbArgs {
    const void* X;
    int64_t F;
    int D;
    int64_t ld;
    int G, C, S;  // groups, classes, waves per group
    float base;
    void* out;
    int64_t ldo;
};

// Stage a tile's 64 frames as float32 into LDS, feature-major [D][64] swizzled
// (kXgbCol); frame r of the tile is row row_of(r) of X, r wave-uniform in
// [0, 64) and the row a valid one for every r.  Wave w takes frames w, w + W,
// ..., its lanes consecutive features of a row (coalesced loads; conflict-free
// writes: bank r ^ lane), 2 rows x 8 feature chunks per lane in flight.  No
// index division: the round-5 loop's e / D cost ~40 VALU per element -- a third
// of the kernel's VALU (PMC r06).  w and lane are the caller's (the users walk
// passes a lane behind its optimisation barrier).
// Returns whether this thread staged a NaN (missing value).
template <int XDT, int KF, class RowOf>  // KF: 64-feature chunks per row, >= ceil(D / 64)
__device__ __forceinline__ bool stage_rows(const void* X, int D, int64_t ld, RowOf row_of, float* xs, int w, int lane) {
    const int W = blockDim.x >> 6;
    bool has_nan = false;
    for (int r0 = w; r0 < kXgbTile; r0 += 2 * W) {  // wave-uniform
        // every load unconditional (clamped row / feature): a load under a branch
        // gets its own s_waitcnt vmcnt(0), serialising the 16 round trips
        typename std::conditional<XDT == CE_F64, double, float>::type v[2][KF];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = min(r0 + h * W, kXgbTile - 1);
            const int64_t row = row_of(r);
#pragma unroll
            for (int k = 0; k < KF; ++k) {
                const int f = min(lane + 64 * k, D - 1);
                if constexpr (XDT == CE_F64)
                    v[h][k] = static_cast<const double*>(X)[row * ld + f];
                else
                    v[h][k] = static_cast<const float*>(X)[row * ld + f];
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = r0 + h * W;
#pragma unroll
            for (int k = 0; k < KF; ++k) {
                const int f = lane + 64 * k;
                if (f < D && r < kXgbTile) {
                    const float x = (float)v[h][k];
                    xs[f * kXgbCol + (r ^ lane)] = x;  // (f & 63) == lane
                    has_nan |= __builtin_isnan(x);
                }
            }
        }
    }
    return has_nan;
}

// f64 frames, two features per lane (16-B loads: half the load instructions of
// stage_rows for the same bytes): lane l takes features 2 l, 2 l + 1 of each
// 128-feature chunk; the pair is clamped to start <= D - 2 (D >= 2), so every
// load stays inside the row and is unconditional.  A/B on one box
// (profiles/r06_xgb.json): 3.279 -> 3.245 ms at 4M frames (dense), 3.418 ->
// 3.390 ms (missing values).
template <int KP, class RowOf>  // KP: 128-feature chunks per row, >= ceil(D / 128)
__device__ __forceinline__ bool stage_rows_pairs(const double* X, int D, int64_t ld, RowOf row_of, float* xs, int w,
                                                 int lane) {
    const int W = blockDim.x >> 6;
    bool has_nan = false;
    for (int r0 = w; r0 < kXgbTile; r0 += 2 * W) {  // wave-uniform
        double2 v[2][KP];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = min(r0 + h * W, kXgbTile - 1);
            const int64_t row = row_of(r);
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                const int fl = min(2 * lane + 128 * k, D - 2);
                const double* src = X + row * ld + fl;
                v[h][k] = make_double2(src[0], src[1]);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = r0 + h * W;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                const int f = 2 * lane + 128 * k, fl = min(f, D - 2);
                if (r < kXgbTile) {
                    if (f < D) {  // f > fl only for f = D - 1 (odd D): the pair's second value
                        const float x = (float)(f == fl ? v[h][k].x : v[h][k].y);
                        xs[f * kXgbCol + (r ^ (f & 63))] = x;
                        has_nan |= __builtin_isnan(x);
                    }
                    if (f + 1 < D && f == fl) {
                        const float x = (float)v[h][k].y;
                        xs[(f + 1) * kXgbCol + (r ^ ((f + 1) & 63))] = x;
                        has_nan |= __builtin_isnan(x);
                    }
                }
            }
        }
    }
    return has_nan;
}

// The objective's transform: the float32 probabilities p[0 .. C) of the tile's
// frame `lane` from its G margins mg[g * 64 + lane].
__device__ __forceinline__ void xgb_proba(const float* mg, int G, int lane, float (&p)[kXgbMaxGroups]) {
    if (G == 1) {  // binary:logistic -> [1 - p, p]
        const float m = mg[lane];
        const float p1 = 1.0f / (1.0f + glibc_expf(-m));
        p[0] = 1.0f - p1;
        p[1] = p1;
    } else {  // multi:softprob -> common::Softmax (xgboost src/common/math.h)
        float mx = mg[lane];
        for (int g = 1; g < G; ++g) mx = fmaxf(mg[g * 64 + lane], mx);
        double wsum = 0.0;  // xgboost: double wsum = 0.0f; ... *i /= static_cast<float>(wsum)
        for (int g = 0; g < G; ++g) {
            p[g] = glibc_expf(mg[g * 64 + lane] - mx);
            wsum += p[g];
        }
        const float ws = (float)wsum;
        for (int g = 0; g < G; ++g) p[g] /= ws;
    }
}

// xgb_proba of frame f0 + lane, written to out (wave 0, one frame per lane).
template <int ODT>
__device__ __forceinline__ void transform_store(const float* mg, int G, int C, int64_t f0, int nf, void* out,
                                                int64_t ldo) {
    const int lane = threadIdx.x & 63;
    if (threadIdx.x >= 64 || lane >= nf) return;
    const int64_t fr = f0 + lane;
    float p[kXgbMaxGroups];
    xgb_proba(mg, G, lane, p);
    for (int c = 0; c < C; ++c) {
        if constexpr (ODT == CE_F64)
            static_cast<double*>(out)[fr * ldo + c] = (double)p[c];
        else
            static_cast<float*>(out)[fr * ldo + c] = p[c];
    }
}

}  // namespace ce
