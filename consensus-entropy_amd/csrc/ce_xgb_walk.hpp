// ce_xgb_walk.hpp -- the XGB member's three forest layouts, the wave-split
// margin chain over any of them and the kernels (ce_xgb.hpp: what is computed,
// the packed layout, the LDS tile).  Its kernels are instantiated by ce_xgb.hip
// alone; ce_xgb_users.hpp instantiates the margin chain (split_margins) over a
// layout of its own, UsersForest, for the kernels of ce_xgb_users.hip, and
// walks it with this header's table_walk8.
#pragma once
#include "ce_xgb.hpp"

namespace ce {

// ---- forest layouts: leaf values of 8 consecutive trees of one group --------
// MISS: the tile holds a missing value somewhere (block-uniform).  Without
// one, "missing -> default child" never fires and the test is !(x < split).

// What every layout holds: perfect trees of one depth, NI = 2^depth - 1 inner
// nodes and NI + 1 leaves each, group g's trees [goff[g], goff[g + 1]).
struct XgbGeom {
    const int32_t* goff;  // [G + 1]
    int depth, NI;
    int goff_end;         // T = goff[G] trees (debug bounds checks only)

    // tree j of a batch of 8 from t0; past the run's end t1 its last tree again (in bounds, not added)
    static __device__ __forceinline__ int tree(int t0, int j, int t1) { return t0 + j < t1 ? t0 + j : t1 - 1; }
    // lane idx4 / 4's value of v (the LDS crossbar: no memory access)
    static __device__ __forceinline__ uint32_t bperm(int idx4, uint32_t v) {
        return (uint32_t)__builtin_amdgcn_ds_bpermute(idx4, (int)v);
    }
};
// T is read in the debug build alone: one statement for every kernel
__device__ __forceinline__ XgbGeom xgb_geom(const XgbArgs& a, const int32_t* goff, int depth) {
#ifdef CE_DEBUG
    const int T = goff[a.G];
#else
    const int T = 0;
#endif
    return XgbGeom{goff, depth, (1 << depth) - 1, T};
}

// The packed arrays (ce_xgb_predict_proba's arguments), walked in two ways.
struct PackedForest : XgbGeom {
    const uint2* nodes;   // [T][NI] {feature | default_left << 31, split_cond bits}
    const float* leaves;  // [T][NI + 1]

    // leaf value of tree t at leaf index li
    __device__ __forceinline__ float value(int t, int li) const {
        CE_DASSERT(t >= 0 && t < goff_end && li >= 0 && li <= NI);
        return leaves[(int64_t)t * (NI + 1) + li];
    }
};

// The split test "missing -> default child, else fvalue < split_cond ? left :
// right", worded once per walk because the wording decides the code.
// node_right reads a packed node (feature clamped to D - 1: the packer checks
// < D); lane_right and table_right a table entry whose fx is the feature's LDS
// column base (xs_fbase), default_left in bit 31 when MISS.  table_right's flip
// was chosen by measurement for the hot path.  Giving lane_right
// that form changes the four k_xgb_walk<*, *, true> kernels, node_right as
// lane_right(xs_fbase(ft) | default bit, ...) the four k_xgb_walk<*, *, false>.
template <bool MISS>
__device__ __forceinline__ bool node_right(uint2 nd, const float* xs, int D, int lane) {
    const int ft = min((int)(nd.x & 0x7fffffffu), D - 1);
    const float x = xs_at(xs, xs_fbase((uint32_t)ft), 4u * (uint32_t)lane);
    const float th = __uint_as_float(nd.y);
    if constexpr (MISS)
        return __builtin_isnan(x) ? (nd.x >> 31) == 0u : !(x < th);
    else
        return !(x < th);
}
template <bool MISS>
__device__ __forceinline__ bool lane_right(uint32_t fx, uint32_t th, const float* xs, uint32_t lane4) {
    const float x = xs_at(xs, MISS ? (fx & 0x7fffffffu) : fx, lane4);
    if constexpr (MISS)
        return __builtin_isnan(x) ? (fx >> 31) == 0u : !(x < __uint_as_float(th));
    else
        return !(x < __uint_as_float(th));
}
template <bool MISS>
__device__ __forceinline__ bool table_right(uint32_t fx, uint32_t th, const float* xs, uint32_t lane4) {
    const float x = xs_at(xs, MISS ? (fx & 0x7fffffffu) : fx, lane4);
    // a NaN fails the compare (right), so flip exactly the NaN lanes whose default
    // is left: three compares and two mask ops
    const bool r = !(x < __uint_as_float(th));
    if constexpr (MISS)
        return r != (__builtin_isnan(x) && (int32_t)fx < 0);
    else
        return r;
}

// Perfect-tree walk (any tree of depth <= 10): 8 trees walked together, so 8
// independent node-gather -> LDS-read -> compare chains are in flight.
struct WalkForest : PackedForest {
    // trees [t0, min(t0 + 8, t1)): leaf indices, and (VALS) their leaf values.
    // Level 0 reads the wave-uniform root (a scalar load; its feature read is
    // one LDS column); deeper levels gather per lane.
    template <bool MISS, bool VALS>
    __device__ __forceinline__ void walk8(const float* xs, int D, int t0, int t1, int lane, int (&li)[8],
                                          float (&v)[8]) const {
        int idx[8];
        const uint2* tn[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            tn[j] = nodes + (int64_t)tree(t0, j, t1) * NI;
            idx[j] = 0;
        }
        if (depth >= 1) {
            uint2 r[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = tn[j][0];
#pragma unroll
            for (int j = 0; j < 8; ++j) idx[j] = node_right<MISS>(r[j], xs, D, lane) ? 2 : 1;
        }
        int lev0 = 1;
        if (depth >= 2) {
            // level 1 from the wave-uniform pair {node 1, node 2} (scalar loads) and a
            // per-lane select: one gather instruction fewer per tree (the walk is
            // bound by the texture path's address rate: TA 79 % busy; 4M frames
            // 5.45 -> 4.88 ms).  Level 2 the same way (4 nodes, two
            // selects) was slower (5.18 ms): the extra VALU outweighs the saved gather.
            // nodes 1 and 2 as two 8-B loads: a tree holds 2^d - 1 nodes (odd), so
            // node 1 of every other tree is only 8-byte aligned (the compiler
            // still merges the pair into one scalar load where it can)
            uint2 n1[8], n2[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                n1[j] = tn[j][1];
                n2[j] = tn[j][2];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint2 nd = idx[j] == 1 ? n1[j] : n2[j];
                idx[j] = 2 * idx[j] + 1 + (node_right<MISS>(nd, xs, D, lane) ? 1 : 0);
            }
            lev0 = 2;
        }
        for (int lev = lev0; lev < depth; ++lev) {
            uint2 nd[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                CE_DASSERT(idx[j] >= 0 && idx[j] < NI);  // an inner node
                nd[j] = tn[j][idx[j]];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) idx[j] = 2 * idx[j] + 1 + (node_right<MISS>(nd[j], xs, D, lane) ? 1 : 0);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            li[j] = idx[j] - NI;
            CE_DASSERT(li[j] >= 0 && li[j] <= NI);  // a leaf of a perfect tree of depth `depth`
        }
        if constexpr (VALS) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = value(tree(t0, j, t1), li[j]);
        }
    }
};

// Lane-table walk (perfect trees of depth <= 5: 2^d - 1 nodes + 2^d leaves <=
// 63 entries, the reference's XGBClassifier(max_depth=5)).  A tree's table is
// read with two COALESCED loads -- lane i holds entry i: node i (i < NI) or
// leaf i - NI (NI <= i <= 2 NI) -- and each level fetches every lane's current
// node from the table with ds_bpermute (the LDS crossbar: no memory access,
// no address chain through L2): 2 loads per tree instead of 1 scalar pair + 3
// per-lane gathers + 1 leaf gather on the texture path the walk was bound by
// (TA 74-79 % busy).  The node's feature is kept as its LDS
// column base (xs_fbase, the clamp to D - 1 done once), so a level is two
// bpermutes, one XOR, one ds_read, one compare and the index update.  The
// root (entry 0) is read with v_readlane: wave-uniform.
struct LaneForest : PackedForest {
    // this lane's table entry of tree t: fx = xs_fbase(feature) (| default_left << 31
    // when MISS), ty = the split condition's bits; at a leaf entry fx = 0, ty = the
    // leaf value's bits; past the table both 0
    template <bool MISS>
    __device__ __forceinline__ void entry(int t, int D, int lane, uint32_t& fx, uint32_t& ty) const {
        fx = 0u;
        ty = 0u;
        if (lane < NI) {
            const uint2 nd = nodes[(int64_t)t * NI + lane];
            const uint32_t ft = min(nd.x & 0x7fffffffu, (uint32_t)(D - 1));  // packer checks < D
            fx = xs_fbase(ft) | (MISS ? (nd.x & 0x80000000u) : 0u);
            ty = nd.y;
        } else if (lane <= 2 * NI) {
            ty = __float_as_uint(leaves[(int64_t)t * (NI + 1) + (lane - NI)]);
        }
    }
    template <bool MISS, bool VALS>
    __device__ __forceinline__ void walk8(const float* xs, int D, int t0, int t1, int lane, int (&li)[8],
                                          float (&v)[8]) const {
        uint32_t fx[8], ty[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) entry<MISS>(tree(t0, j, t1), D, lane, fx[j], ty[j]);
        const uint32_t lane4 = 4u * (uint32_t)lane;
        int idx4[8];  // 4 x the lane's node index (a ds_bpermute byte address); children 2 idx4 + 4 / + 8
#pragma unroll
        for (int j = 0; j < 8; ++j) idx4[j] = 0;
        if (depth >= 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t f0 = (uint32_t)__builtin_amdgcn_readlane((int)fx[j], 0);
                const uint32_t h0 = (uint32_t)__builtin_amdgcn_readlane((int)ty[j], 0);
                idx4[j] = lane_right<MISS>(f0, h0, xs, lane4) ? 8 : 4;
            }
        }
        for (int lev = 1; lev < depth; ++lev) {
            uint32_t f[8], h[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                f[j] = bperm(idx4[j], fx[j]);
                h[j] = bperm(idx4[j], ty[j]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) idx4[j] = 2 * idx4[j] + (lane_right<MISS>(f[j], h[j], xs, lane4) ? 8 : 4);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            li[j] = (idx4[j] >> 2) - NI;
            CE_DASSERT(li[j] >= 0 && li[j] <= NI);
        }
        if constexpr (VALS) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = __uint_as_float(bperm(idx4[j], ty[j]));
        }
    }
};

// Prebuilt lane tables (ce_xgb_lane_table; depth <= 5): tree t's 64 entries
// [t][64] x {fx, ty} in a 1-based heap -- lane j in [1, 2^d) holds node j - 1
// as {xs_fbase(min(feature, D - 1)) | default_left << 31, split_cond bits},
// lane 2^d + k leaf k as {0, leaf bits}, lane 0 and the rest {0, 0} -- so one
// coalesced dwordx2 load with a scalar base is a tree's whole table (no
// per-lane branches or feature arithmetic), the root comes from a scalar load,
// and a level is child = 2 j + right.  VALU per tree was the limiter of the
// on-the-fly tables (PMC r06: VALU 72 % busy, 80 VALU per tree and wave).  Two
// halves [2][T][64]: the second without the default_left bits, read by tiles
// without a missing value (no mask per node read).
//
// The walk is table_walk8, one text for every forest over such tables: F gives
// the geometry and row(k), the entry offset of logical tree k (LaneTableForest:
// k itself; UsersForest, ce_xgb_users.hpp: through tree_ids).  The rows are
// formed first (tr[8]) and both the coalesced loads and the scalar loads read
// through them: worded so, every kernel of the users form and of the fit is
// byte for byte what it was while the walk stood there a second time
// (profiles/xgb_one_text_codeobj.json); k_xgb_lanes' code moved, within its
// registers, and was timed against the parent's (profiles/xgb_one_text_ab.json).
//
// 4 trees at a time (two rounds per batch of 8): 4 independent chains per
// lane keep every level's 8 bpermutes in flight within the 64-VGPR budget of
// 8 waves per SIMD (8 chains forced the compiler to serialize the split
// conditions' bpermutes behind lgkmcnt(0)); the second round's tables are
// loaded with the first's.
template <bool MISS, bool VALS, class F>
__device__ __forceinline__ void table_walk8(const F& f, const uint2* tb, const float* xs, int t0, int t1, int lane,
                                            int (&li)[8], float (&v)[8]) {
    const uint2* tr[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) tr[j] = tb + f.row(F::tree(t0, j, t1));
    uint2 e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = tr[j][lane];
    const uint32_t lane4 = 4u * (uint32_t)lane;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        int h[4];  // the lane's heap index x 4 (a ds_bpermute byte address): root 4, children 2 h + 4 b
#pragma unroll
        for (int j = 0; j < 4; ++j) h[j] = 4;
        // entries 0..3 of each tree (root 1, level-1 pair 2 / 3): 32 wave-uniform
        // bytes, scalar loads issued together before the first use (one wait)
        uint4 q0[4], q1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint4* p = reinterpret_cast<const uint4*>(tr[4 * g + j]);
            q0[j] = p[0];
            q1[j] = p[1];
        }
        if (f.depth >= 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = table_right<MISS>(q0[j].z, q0[j].w, xs, lane4) ? 12 : 8;
        }
        if (f.depth >= 2) {  // level 1 from the pair {2, 3} and a select
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool rt = h[j] == 12;
                const uint32_t fx = rt ? q1[j].z : q1[j].x, th = rt ? q1[j].w : q1[j].y;
                h[j] = 2 * h[j] + (table_right<MISS>(fx, th, xs, lane4) ? 4 : 0);
            }
        }
        for (int lev = 2; lev < f.depth; ++lev) {
            uint32_t fx[4], th[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                fx[j] = F::bperm(h[j], e[4 * g + j].x);
                th[j] = F::bperm(h[j], e[4 * g + j].y);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = 2 * h[j] + (table_right<MISS>(fx[j], th[j], xs, lane4) ? 4 : 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            li[4 * g + j] = (h[j] >> 2) - (f.NI + 1);
            CE_DASSERT(li[4 * g + j] >= 0 && li[4 * g + j] <= f.NI);
            if constexpr (VALS) v[4 * g + j] = __uint_as_float(F::bperm(h[j], e[4 * g + j].y));
        }
    }
}

struct LaneTableForest : XgbGeom {
    const uint2* table;     // [T][64], fx with default_left in bit 31 (tiles holding a missing value)
    const uint2* table_nd;  // [T][64], fx without it (the other tiles: no mask per node read)

    __device__ __forceinline__ int64_t row(int t) const {
        CE_DASSERT(t >= 0 && t < goff_end);
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

// ---- one block per 64-frame tile: G x S waves ------------------------------
// Wave (g, s) takes a contiguous run of group g's trees: s = 0 the head, its
// leaves added straight into the margin (a batch's leaf loads are added after
// the next batch is evaluated, hiding their latency); s >= 1 one of the S - 1
// tail chunks of at most kXgbChunk trees, whose leaf indices wait in registers
// (16 bits each) until the wave's phase.
// S ordered phases then hand the margin on through LDS (phase s: wave (g, s)
// adds its leaves in model order), so preds[g] is exactly the reference's
// sequential float chain while S times as many waves hide the latency.
constexpr int kXgbChunk = 24;

template <class L, bool MISS>
__device__ __forceinline__ void split_margins(const XgbArgs& a, const L& fl, const float* xs, float* mg, int g,
                                              int s, int lane) {
    const int k0 = fl.goff[g], k1 = fl.goff[g + 1], n = k1 - k0, S = a.S;
    const int c = min(kXgbChunk, (n + S - 1) / S);
    const int head_end = max(k0, k1 - (S - 1) * c);
    float m = a.base;
    uint32_t packed[kXgbChunk / 2] = {};  // tail waves: leaf indices, 16 bits each
    int lo = 0, cnt = 0;
    if (s == 0) {
        float pend[8];
        int npend = 0;
        for (int k = k0; k < head_end; k += 8) {
            int li[8];
            float v[8];
            fl.template walk8<MISS, true>(xs, a.D, k, head_end, lane, li, v);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < npend) m += pend[j];
#pragma unroll
            for (int j = 0; j < 8; ++j) pend[j] = v[j];
            npend = min(8, head_end - k);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < npend) m += pend[j];
    } else {
        lo = head_end + (s - 1) * c;
        const int hi = min(k1, lo + c);
        cnt = max(0, hi - lo);
#pragma unroll
        for (int b = 0; b < kXgbChunk / 8; ++b) {
            if (b * 8 < cnt) {
                int li[8];
                float v[8];
                fl.template walk8<MISS, false>(xs, a.D, lo + b * 8, hi, lane, li, v);
#pragma unroll
                for (int j = 0; j < 8; j += 2) packed[b * 4 + j / 2] = (uint32_t)li[j] | ((uint32_t)li[j + 1] << 16);
            }
        }
    }
    // the tail wave's leaf values, all loaded before the ordered phases (one
    // latency, not one per phase: the phases are a chain of S - 1 hand-offs);
    // slots past cnt re-read the clamped last (tree, leaf) -- in bounds, not added
    float tv[kXgbChunk];
#pragma unroll
    for (int i = 0; i < kXgbChunk; ++i)
        tv[i] = (s > 0 && i < cnt) ? fl.value(lo + i, (packed[i / 2] >> (16 * (i & 1))) & 0xffffu) : 0.0f;
    for (int ph = 0; ph < S; ++ph) {
        if (s == ph && s > 0) {
            m = mg[g * 64 + lane];
#pragma unroll
            for (int i = 0; i < kXgbChunk; ++i)
                if (i < cnt) m += tv[i];
        }
        if (s == ph) mg[g * 64 + lane] = m;
        __syncthreads();
    }
}

template <int XDT, int ODT, class L, int KF = kXgbMaxFeat / 64>
__device__ __forceinline__ void xgb_tile(const XgbArgs& a, const L& fl) {
    extern __shared__ float xsm[];
    float* xs = xsm;                  // [D][kXgbCol] swizzled
    float* mg = xsm + a.D * kXgbCol;  // [G][64] margins
    uint32_t* nanw = reinterpret_cast<uint32_t*>(mg + a.G * 64);  // [waves] the tile's missing-value votes
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = w / a.S, s = w - g * a.S;
    const int64_t f0 = (int64_t)blockIdx.x * kXgbTile;
    const int nf = (int)min<int64_t>(kXgbTile, a.F - f0);
    const auto row_of = [&](int r) { return f0 + min(r, nf - 1); };  // slots past the end repeat the last frame
    bool has_nan;
    if constexpr (XDT == CE_F64 && KF < kXgbMaxFeat / 64) {  // (the lane-table kernel's widths)
        if (a.D >= 2)
            has_nan = stage_rows_pairs<(KF + 1) / 2>(static_cast<const double*>(a.X), a.D, a.ld, row_of, xs, w, lane);
        else
            has_nan = stage_rows<XDT, KF>(a.X, a.D, a.ld, row_of, xs, w, lane);
    } else {
        has_nan = stage_rows<XDT, KF>(a.X, a.D, a.ld, row_of, xs, w, lane);
    }
    // the block's "any NaN" vote through the dynamic LDS (__syncthreads_or keeps
    // a static LDS word, which puts the tile 256 B off address 0: one more VALU
    // per node read)
    {
        const bool wn = __ballot(has_nan) != 0;
        if (lane == 0) nanw[w] = wn ? 1u : 0u;
    }
    __syncthreads();
    bool any_nan = false;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) any_nan |= nanw[k] != 0u;
    if (any_nan)
        split_margins<L, true>(a, fl, xs, mg, g, s, lane);
    else
        split_margins<L, false>(a, fl, xs, mg, g, s, lane);
    transform_store<ODT>(mg, a.G, a.C, f0, nf, a.out, a.ldo);
}

// LANES: the lane-table walk (depth <= 5), else the perfect-tree gather walk
template <int XDT, int ODT, bool LANES>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_xgb_walk(
    XgbArgs a, const uint2* __restrict__ nodes, const float* __restrict__ leaves, const int32_t* __restrict__ goff,
    int depth) {
    const PackedForest pf{xgb_geom(a, goff, depth), nodes, leaves};
    if constexpr (LANES) {
        CE_DASSERT(depth <= kXgbLaneDepth);
        xgb_tile<XDT, ODT>(a, LaneForest{pf});
    } else {
        xgb_tile<XDT, ODT>(a, WalkForest{pf});
    }
}

// KF: the row's 64-feature chunks the staging loads (>= ceil(D / 64); every load
// is unconditional, so a smaller KF drops dead loads: D = 260 takes 5 of 8)
template <int XDT, int ODT, int KF>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_xgb_lanes(
    XgbArgs a, const uint2* __restrict__ table, const uint2* __restrict__ table_nd, const int32_t* __restrict__ goff,
    int depth) {
    CE_DASSERT(depth <= kXgbLaneDepth);
    xgb_tile<XDT, ODT, LaneTableForest, KF>(a, LaneTableForest{xgb_geom(a, goff, depth), table, table_nd});
}

}  // namespace ce
