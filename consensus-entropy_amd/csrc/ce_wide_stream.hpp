// ce_wide_stream.hpp -- the wide-class stream (C outside the register-path
// set, up to kWideMaxC; q <= 64): one wave per item (wide_item), the
// software-pipelined vector stream k_stream_wide2 with its approximate
// prefilter (CE_WIDE_PREFILTER), the sampled floor and grid vote in front of
// it (k_wide_seed, k_wide_seed_pick, kWideVoteDen, wide_nsamples,
// wide_sample_pos, wide_vote_heavy), the unpipelined k_stream_wide and the
// per-item entropy k_wide_entropy_v.  The row arithmetic is in ce_wide.hpp.
// ce_launch_stream.o instantiates the stream and seed kernels, ce_abi_core.o
// k_wide_entropy_v; k_partial_wide (ce_partial.hpp) scores with wide_item.
#pragma once
#include "ce_device.hpp"
#include "ce_merge.hpp"   // fold_merge
#include "ce_stream.hpp"  // StreamArgs
#include "ce_topq.hpp"    // kBS, Cand
#include "ce_wave.hpp"
#include "ce_wide.hpp"
#include "ce_ws.hpp"  // kWideVoteSamples, kStreamMaxQ

namespace ce {

// Wide classes on the streaming engine (q <= 64): one wave per item, every
// wave independent, per-wave top-q.  NPL = classes owned per lane (C <= 64*NPL).
template <int DT, int NPL, bool VEC>
__device__ __forceinline__ double wide_item(const WideArgs& a, const PwPlan& pl, int64_t it, double* row,
                                            double* scratch) {
    if constexpr (VEC) {
        constexpr int KCH = NPL / ChunkT<DT>::CPC;
        constexpr int UNR = KCH >= 8 ? 1 : 8 / KCH;
        return wave_item_entropy_vec<DT, KCH, UNR>(a.p, it * a.sN, a.M, a.C, a.sM, a.dM, a.invM, a.pow2, pl, row,
                                                   scratch);
    } else {
        return wave_item_entropy<DT, NPL>(a.p, it * a.sN, a.M, a.C, a.sM, a.sC, a.dM, a.invM, a.pow2, pl, row,
                                          scratch, nullptr);
    }
}

template <int DT, int NPL, bool VEC>
__global__ __launch_bounds__(kBS) void k_stream_wide(WideArgs a, PwPlan pl, StreamArgs sa, int q,
                                                     Cand* __restrict__ wc) {
    stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
    __shared__ WaveLists sm;
    extern __shared__ __attribute__((aligned(16))) double wsm[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* row = wsm + w * wide_lds_doubles(a.C);
    double* scratch = row + a.C;
    const int64_t gw = (int64_t)blockIdx.x * 4 + w;
    int64_t lo = gw * sa.per_wave;
    int64_t hi = lo + sa.per_wave;
    if (hi > a.N) hi = a.N;
    if (lo > hi) lo = hi;
    RegTopQ tq;
    tq.init(q);
    for (int64_t t0 = lo; t0 < hi; t0 += 64) {
        uint64_t mykey = 0;
        for (int j = 0; j < 64; ++j) {
            const int64_t it = t0 + j;
            if (it >= hi) break;  // wave-uniform
            const double h = wide_item<DT, NPL, VEC>(a, pl, it, row, scratch);
            if (lane == j) mykey = order_key(h);
        }
        const int64_t i = t0 + lane;
        tq.offer(mykey, i + sa.base_idx, i < hi);
    }
    block_merge_write<4>(tq, sm, q, wc + (int64_t)blockIdx.x * q, sa.nlists);
}

// Wide classes, vectorised rows (q <= 64): one wave per item, lanes over 16-B
// chunks, software-pipelined over the wave's flat sequence of (item, member
// batch) pairs -- batch t+1 is in flight while batch t is added, and the next
// item's first batch while an item's entropy is computed, so the wave always
// has 2 x UNR x KCH 16-B loads per lane outstanding.  Items per wave are not
// rounded to 64 (a wide item is tens of KB): every wave of the resident grid
// gets work.
// Measured and not kept: a 3-deep ring (0.782-0.784 vs
// 0.790-0.801 of HBM), a 4-wave register cap, the entr pass fed from the LDS
// row, and 16 KiB LDS-DMA tiles per wave (1.5-2.5 % slower on the C5 job).
#ifndef CE_WIDE_PREFILTER
#define CE_WIDE_PREFILTER 1
#endif
// The wide stream's floor and grid, chosen on the device before the stream
// (ce_launch_stream.hip; every wide launch with heavy items that folds its
// lists: single selections, the multi-GPU records, every chunk of a job):
//   k_wide_seed       wide_nsamples(N) items, one per stratum of the pool at a
//                     hashed offset, one wave each: the EXACT entropy (the
//                     stream's own arithmetic) and the approximate one;
//   k_wide_seed_pick  the floor = the better of the samples' q-th best (key,
//                     any position: every one of those q items is in the pool
//                     and re-enters the stream's lists, ties included) and a
//                     chunked job's running q-th entry; then the vote = the
//                     samples that would still take the exact entropy against it.
// Both grids are launched; the one the vote does not pick exits at its first
// instruction.  The deep-ring grid (one block per CU, 8-batch ring) reads a
// pool whose items nearly all skip at 0.86-0.89 of HBM but one whose items
// mostly take the exact entropy at 0.51, where the occupancy grid keeps
// 0.79-0.82 (profiles/r06_c5_vote.json): it runs iff at most 1/kWideVoteDen
// of the samples are exact.  The sampled floor leaves ~q / kWideVoteSamples of
// any pool above it whatever the pool's order (a rising-entropy pool included),
// so single selections and first chunks get the deep grid too.  The samples
// read 1/16 of a small launch's items and 256 MB of a 128 GB C5 chunk.
constexpr int kWideVoteDen = 16;
// samples of an N-item launch: N / 16, at most kWideVoteSamples (the launcher
// runs the path from 1024 samples on: N >= 16384)
__host__ __device__ __forceinline__ int64_t wide_nsamples(int64_t N) {
    return N / 16 < kWideVoteSamples ? N / 16 : kWideVoteSamples;
}
__device__ __forceinline__ bool wide_vote_heavy(uint32_t v, int64_t N) {
    return (int64_t)v * kWideVoteDen <= wide_nsamples(N);
}
// sample s of ns over [0, N): stratum s at a hashed offset (no periodic pool
// pattern lines up with the samples)
__host__ __device__ __forceinline__ int64_t wide_sample_pos(int64_t s, int64_t ns, int64_t N) {
    const int64_t lo = s * N / ns, hi = (s + 1) * N / ns;
    uint32_t h = (uint32_t)s * 2654435761u;
    h ^= h >> 15;
    h *= 2246822519u;
    h ^= h >> 13;
    return hi > lo ? lo + (int64_t)(h % (uint64_t)(hi - lo)) : lo;
}
template <int DT, int KCH, int UNR>
__global__ __launch_bounds__(kBS) void k_wide_seed(WideArgs a, PwPlan pl, int64_t base_idx,
                                                   const uint32_t* __restrict__ excl, Cand* __restrict__ samp,
                                                   float* __restrict__ sapx) {
    stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
    extern __shared__ __attribute__((aligned(16))) double wsm[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t ns = wide_nsamples(a.N);
    const int64_t s = (int64_t)blockIdx.x * 4 + w;
    if (s >= ns) return;  // wave-uniform (after the block's only barrier)
    CE_DASSERT(a.M % UNR == 0);
    constexpr int CPC = ChunkT<DT>::CPC, EB = 16 / CPC;
    const int K = a.C / CPC;
    double* row = wsm + w * wide_lds_doubles(a.C);
    double* scratch = row + a.C;
    uint32_t off[KCH];
#pragma unroll
    for (int kk = 0; kk < KCH; ++kk) {
        const int ch = lane + 64 * kk;
        off[kk] = 16u * (uint32_t)(ch < K ? ch : K - 1);
    }
    const int64_t i = wide_sample_pos(s, ns, a.N);
    const char* item = static_cast<const char*>(a.p) + i * a.sN * EB;
    double acc[KCH * CPC];
#pragma unroll
    for (int x = 0; x < KCH * CPC; ++x) acc[x] = 0.0;
    WideBatch<DT, KCH, UNR> b;
    for (int m = 0; m < a.M; m += UNR) {  // member order, as the stream adds
        b.issue(item, m, a.sM * EB, off);
        b.add(acc);
    }
    bool special;
    const float ap = wave_approx_entropy<DT, KCH>(acc, K, special);
    const double h = wave_entropy_from_sums<DT, KCH>(acc, K, a.dM, a.invM, a.pow2, pl, row, scratch);
    if (lane == 0) {
        const bool out = excl != nullptr && excluded(excl, i);
        samp[s] = Cand{out ? 0ull : order_key(h), i + base_idx};
        sapx[s] = out ? -__builtin_inff() : (special ? __builtin_inff() : ap);  // -inf: never exact; +inf: always
    }
}
// one block of 16 waves (a template: defined in a header that several
// translation units include, instantiated in one)
template <int NS>
__global__ __launch_bounds__(1024) void k_wide_seed_pick(const Cand* __restrict__ samp, const float* __restrict__ sapx,
                                                         int ns, int q, const Cand* __restrict__ extra,
                                                         Cand* __restrict__ seed, uint32_t* __restrict__ vote) {
    __shared__ WaveListsT<16> sm;
    __shared__ Cand lst[kStreamMaxQ];
    __shared__ Cand pick;
    __shared__ uint32_t cnt;
    CE_DASSERT(ns <= NS && q >= 1 && q <= kStreamMaxQ && blockDim.x == 1024);
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    // the samples' top q (per-wave register lists over 64-sample rounds, then the
    // block's merge tree): lst[q - 1] is the q-th best
    RegTopQ tq;
    tq.init(q);
    for (int j0 = w * 64; j0 < ns; j0 += 1024) {  // wave-uniform
        const int j = j0 + lane;
        const Cand c = j < ns ? samp[j] : Cand{0ull, -1};
        tq.offer(c.key, c.idx, j < ns && c.key != 0);
    }
    block_merge_write<16>(tq, sm, q, lst, 1);
    if (t == 0) cnt = 0u;
    __syncthreads();
    if (t == 0) {
        // the q-th best sample as a floor admitting every item of its key (each of
        // the q samples is in the pool and re-enters the stream's lists, ties
        // included); a chunked job's running list's q-th entry is a floor too
        const Cand s = lst[q - 1];
        Cand f = (s.idx >= 0 && s.key != 0) ? Cand{s.key, INT64_MAX} : Cand{0ull, -1};
        if (extra != nullptr) {
            const Cand e = extra[q - 1];
            if (e.idx >= 0 && e.key != 0 && (f.idx < 0 || better(e.key, e.idx, f.key, f.idx))) f = e;
        }
        pick = f;
    }
    __syncthreads();
    const Cand f = pick;
    // the vote: samples the prefilter would still send to the exact entropy
    uint32_t mine = 0;
    for (int j = t; j < ns; j += 1024) {
        bool exact = true;
        if (f.idx >= 0 && f.key != 0)
            exact = !(sapx[j] == -__builtin_inff()) &&
                    !(f.key == ~0ull || (double)sapx[j] < key_to_val(f.key) * 1.4426950408889634 - 2.0 * kWideApproxErr2);
        mine += exact ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if (lane == 0 && mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (t == 0) {
        seed[0] = f;
        vote[0] = cnt;
    }
}

template <int DT, int KCH, int UNR, int NB = 2>
__global__ __launch_bounds__(kBS) void k_stream_wide2(WideArgs a, PwPlan pl, StreamArgs sa, int q,
                                                      Cand* __restrict__ wc) {
    // the device-side grid choice (k_wide_seed_pick's vote): the other grid runs
    if (sa.vote && wide_vote_heavy(*sa.vote, sa.N) != (sa.vote_heavy != 0)) return;
    stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
    CE_DASSERT((int)gridDim.x <= sa.nlists && q >= 1 && q <= kStreamMaxQ && a.M % UNR == 0);
    __shared__ WaveLists sm;
    extern __shared__ __attribute__((aligned(16))) double wsm[];
    constexpr int CPC = ChunkT<DT>::CPC, EB = 16 / CPC;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* row = wsm + w * wide_lds_doubles(a.C);
    double* scratch = row + a.C;
    const int64_t gw = (int64_t)blockIdx.x * 4 + w;
    // the wave's items: cnt items lo0, lo0 + stride, ...  -- grid-cyclic (wave
    // g takes items g, g + W, ...: the items in flight at any moment are one
    // contiguous sweep; C5 job 0.754-0.770 -> 0.779-0.781 of HBM against a
    // contiguous run per wave on one box, profiles/r03_tile_order.json)
    const int64_t W = (int64_t)gridDim.x * 4;
    const int64_t lo0 = gw, stride = W;
    const int64_t cnt = a.N > gw ? (a.N - gw + W - 1) / W : 0;
    RegTopQ tq;
    tq.init(q);
#if CE_WIDE_PREFILTER
    // the floor (k_wide_seed_pick: sampled items, or a chunked job's running
    // list -- sa.extra, the top q of every chunk so far): an item not better
    // than it cannot enter the top q, so the prefilter skips from the first
    // item on
    if (sa.seed || sa.extra) {
        CE_DASSERT(q >= 1 && q <= kStreamMaxQ);
        const Cand e = sa.seed ? sa.seed[0] : sa.extra[q - 1];
        if (e.idx >= 0 && e.key != 0) tq.init(q, e.key, e.idx);
    }
#endif
    const char* base = static_cast<const char*>(a.p);
    const int64_t sNb = a.sN * EB, sMb = a.sM * EB;
    const int K = a.C / CPC;
    const int NBM = a.M / UNR;  // member batches per item (UNR divides M, host)
    double acc[KCH * CPC];
#pragma unroll
    for (int e = 0; e < KCH * CPC; ++e) acc[e] = 0.0;
    uint64_t mykey = 0;
    int64_t myidx = 0;
    // issue cursor (item ordinal, batch) and consume cursor
    int64_t ii = 0, ci = 0;
    int ib = 0, cb = 0;
    uint32_t off[KCH];  // this lane's chunk offsets in a member row (clamped into the row)
#pragma unroll
    for (int kk = 0; kk < KCH; ++kk) {
        const int ch = lane + 64 * kk;
        off[kk] = 16u * (uint32_t)(ch < K ? ch : K - 1);
    }
    WideBatch<DT, KCH, UNR> buf[NB];  // ring: NB - 1 batches in flight while one is added
    auto issue = [&](WideBatch<DT, KCH, UNR>& X) {
        X.issue(base + (lo0 + ii * stride) * sNb, ib * UNR, sMb, off);
        if (++ib == NBM) {
            ib = 0;
            ++ii;
        }
    };
    auto consume = [&](const WideBatch<DT, KCH, UNR>& X) {
        X.add(acc);
        if (++cb == NBM) {  // item ci complete
            cb = 0;
            // approximate prefilter (wave-uniform): an item whose approximate
            // entropy is more than 2 kWideApproxErr2 below the wave's current
            // threshold (its q-th best exact key, or the running floor) cannot
            // enter the top q -- its exact entropy is below the threshold -- and
            // skips the exact entropy (the row sums through LDS, C glibc logs)
            bool skip = false;
#if CE_WIDE_PREFILTER
            if (tq.tk != 0) {
                bool special;
                const float ap = wave_approx_entropy<DT, KCH>(acc, K, special);
                if (!special)
                    skip = tq.tk == ~0ull ||  // q NaN entropies held: only a NaN ties
                           (double)ap < key_to_val(tq.tk) * 1.4426950408889634 - 2.0 * kWideApproxErr2;
            }
#endif
            double h = 0.0;
            if (!skip) h = wave_entropy_from_sums<DT, KCH>(acc, K, a.dM, a.invM, a.pow2, pl, row, scratch);
#pragma unroll
            for (int e = 0; e < KCH * CPC; ++e) acc[e] = 0.0;
            const int j = (int)(ci & 63);
            if (lane == j) {
                mykey = skip ? 0ull : order_key(h);
                myidx = lo0 + ci * stride;
            }
            if (j == 63 || ci == cnt - 1) {
                bool ok = lane <= j;
                if (sa.excl) ok = ok && !excluded(sa.excl, lane <= j ? myidx : lo0 + ci * stride);
                tq.offer(mykey, myidx + sa.base_idx, ok);
                mykey = 0;
            }
            ++ci;
        }
    };
#pragma unroll
    for (int b = 0; b < NB - 1; ++b)
        if (ii < cnt) issue(buf[b]);
    while (ci < cnt) {
#pragma unroll
        for (int s = 0; s < NB; ++s) {  // compile-time ring slots: no register-array indexing
            if (ii < cnt) issue(buf[(s + NB - 1) % NB]);
            consume(buf[s]);
            if (ci >= cnt) break;
        }
    }
    block_merge_write<4>(tq, sm, q, wc + (int64_t)blockIdx.x * q, sa.nlists, nullptr, nullptr, 4, sa.ctr != nullptr);
    if (sa.ctr) fold_merge<4>(sa.ctr, sa.oval, sa.oidx, sa.ocand, q, wc, sm, sa.extra);
}

template <int DT, int NPL, bool VEC>
__global__ __launch_bounds__(kBS) void k_wide_entropy_v(WideArgs a, PwPlan pl, double* __restrict__ ent) {
    stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
    extern __shared__ __attribute__((aligned(16))) double wsm[];
    const int w = threadIdx.x >> 6;
    double* row = wsm + w * wide_lds_doubles(a.C);
    double* scratch = row + a.C;
    for (int64_t i = (int64_t)blockIdx.x * 4 + w; i < a.N; i += (int64_t)gridDim.x * 4) {
        const double h = wide_item<DT, NPL, VEC>(a, pl, i, row, scratch);
        if ((threadIdx.x & 63) == 0) ent[i] = h;
    }
}

}  // namespace ce
