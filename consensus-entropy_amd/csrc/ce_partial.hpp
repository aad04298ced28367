// ce_partial.hpp -- the block-synchronous stage 1 (any q <= CE_MAX_Q):
//   k_partial<Src>   score items (committee consensus entropy, an entropy
//                    vector, or an hc table row) and keep a per-block top-q in
//                    LDS; one pass over HBM, entropies never written back.
//                    Replaces amg_test.py:441-445 / :451-452 / :479-480.
//   k_partial_wide   the same for wide classes (wide_item, ce_wide_stream.hpp).
// seg_range maps a block to its share of a segment (Seg, ce_topq.hpp).
// ce_launch_partial.o is the only object that instantiates both kernels.
#pragma once
#include "ce_device.hpp"
#include "ce_topq.hpp"  // kBS, Seg, TopQ, write_list
#include "ce_wave.hpp"  // excluded
#include "ce_wide.hpp"
#include "ce_wide_stream.hpp"  // wide_item

namespace ce {

__device__ __forceinline__ void seg_range(const Seg& sg, int64_t& s0, int64_t& lo, int64_t& hi) {
    const int b = blockIdx.x;
    const int u = b / sg.bpu, c = b % sg.bpu;
    int64_t s1;
    if (sg.offsets) {
        s0 = sg.offsets[u];
        s1 = sg.offsets[u + 1];
    } else {
        s0 = 0;
        s1 = sg.N;
    }
    const int64_t len = s1 > s0 ? s1 - s0 : 0;
    int64_t per = (len + sg.bpu - 1) / sg.bpu;
    per = (per + kBS - 1) / kBS * kBS;
    lo = s0 + (int64_t)c * per;
    hi = lo + per < s1 ? lo + per : s1;
    if (lo > hi) lo = hi;
}

// ---------------------------------------------------------------------------
// Stage 1: score + per-block top-q.  One item per thread per round.
// ---------------------------------------------------------------------------
template <class Src, int CAP, bool FINAL>
__global__ __launch_bounds__(kBS) void k_partial(Src src, Seg sg, int q, Cand* __restrict__ wc, double* __restrict__ oval,
                                                 int64_t* __restrict__ oidx) {
    stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
    __shared__ TopQSmem<CAP> sm;
    TopQ<CAP, kBS> tq(sm);
    tq.init();
    CE_DASSERT(q >= 1 && q <= CAP);
    int64_t s0, lo, hi;
    seg_range(sg, s0, lo, hi);
    const int64_t rel = sg.base_idx - s0;
    for (int64_t i0 = lo; i0 < hi; i0 += kBS) {
        const int64_t i = i0 + threadIdx.x;
        const bool valid = i < hi && !(sg.excl && excluded(sg.excl, i));
        uint64_t k = 0;
        if (valid) k = src.key(i);
        tq.offer(k, i + rel, valid);
        tq.end_round(q, kBS);
    }
    const int cnt = tq.finish(q);
    const int64_t slot = (int64_t)blockIdx.x * q;
    write_list<CAP, FINAL>(sm, cnt, q, wc + slot, oval + (FINAL ? slot : 0), oidx + (FINAL ? slot : 0));
}

// Wide-class variant of k_partial (q > 64 / segments): a wave scores 64
// consecutive items (one per lane slot), so a block round is still 256.
template <int DT, int NPL, bool VEC, int CAP, bool FINAL>
__global__ __launch_bounds__(kBS) void k_partial_wide(WideArgs a, PwPlan pl, Seg sg, int q, Cand* __restrict__ wc,
                                                      double* __restrict__ oval, int64_t* __restrict__ oidx) {
    stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
    __shared__ TopQSmem<CAP> sm;
    extern __shared__ __attribute__((aligned(16))) double wsm[];
    TopQ<CAP, kBS> tq(sm);
    tq.init();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* row = wsm + w * wide_lds_doubles(a.C);
    double* scratch = row + a.C;
    int64_t s0, lo, hi;
    seg_range(sg, s0, lo, hi);
    const int64_t rel = sg.base_idx - s0;
    for (int64_t i0 = lo; i0 < hi; i0 += kBS) {
        uint64_t mykey = 0;
        const int64_t wbase = i0 + 64 * w;
        for (int j = 0; j < 64; ++j) {
            const int64_t it = wbase + j;
            if (it >= hi) break;  // wave-uniform
            const double h = wide_item<DT, NPL, VEC>(a, pl, it, row, scratch);
            if (lane == j) mykey = order_key(h);
        }
        const int64_t i = i0 + threadIdx.x;
        tq.offer(mykey, i + rel, i < hi && !(sg.excl && excluded(sg.excl, i)));
        tq.end_round(q, kBS);
    }
    const int cnt = tq.finish(q);
    const int64_t slot = (int64_t)blockIdx.x * q;
    write_list<CAP, FINAL>(sm, cnt, q, wc + slot, oval + (FINAL ? slot : 0), oidx + (FINAL ? slot : 0));
}

}  // namespace ce
