// ce_merge.hpp -- stage 2: merges of best-first candidate lists into the top q.
//
// As device functions, inlined into the last block of a stage-1 grid (the
// fold: fold_merge -> merge_lists_lean / merge_lists_block over a FoldSrc),
// and as kernels over a ListSrc (records or (val, idx) arrays):
//   k_merge_reg      q <= 64: register lists floored at the head bound
//   k_finish_heads   q <= kHeadsMaxQ: LDS buffer floored at the q-th best head
//   k_finish         any q <= CE_MAX_Q: LDS buffer floored at the full lists' worst
//   k_merge_wave     a few lists per segment, one wave per segment
// ce_launch_finish.o is the only object that instantiates the four kernels;
// the fold is instantiated inside the streaming, wide and frames kernels.
#pragma once
#include "ce_device.hpp"
#include "ce_topq.hpp"
#include "ce_wave.hpp"
#include "ce_ws.hpp"  // kStreamMaxQ

namespace ce {

constexpr int kFinBS = 1024;      // stage-2 block: 16 waves

// A source of best-first candidate lists: Cand records (the workspace, the
// ranks' all-gathered records) or (val, idx) arrays (ce_topq_merge).
template <bool FROM_VALS>
struct ListSrc {
    const Cand* c;
    const double* val;
    const int64_t* idx;
    __device__ __forceinline__ void get(int64_t j, uint64_t& k, int64_t& i) const {
        if constexpr (FROM_VALS) {
            i = idx[j];
            k = order_key(val[j]);
        } else {
            const Cand x = c[j];
            k = x.key;
            i = x.idx;
        }
    }
};

// Merge nl best-first lists of q candidates (empty slots, idx < 0, at each
// list's tail) with the W waves of ONE block into the top-q, written as final
// (oval, oidx) or as records (ocand).  Exact floor from the list heads: the
// q-th best head T_w among a wave's lists is reached by q distinct lists, so
// every global top-q candidate is >= T = the best T_w; only lists whose head
// is >= T (~q of them) are read past their head, and only their entries >= T
// enter the register lists.  One round of head loads (nl / (64 W) per lane)
// plus ~q list loads per block instead of all nl * q candidates.
// bk / bi: W-entry LDS scratch; L: the block-merge scratch.
// The grid's lists followed by one extra list elsewhere (a chunked job's
// running top-q): list g < na at a[g*q..], list na at extra[0..q).
struct FoldSrc {
    const Cand* a;
    int64_t na_q;  // na * q
    const Cand* extra;
    __device__ __forceinline__ void get(int64_t j, uint64_t& k, int64_t& i) const {
        // the grid's lists were handed off in this launch: sc1 loads only
        const Cand x = j < na_q ? load_cand_wt(a + j) : extra[j - na_q];
        k = x.key;
        i = x.idx;
    }
};

template <int W, class Src>
__device__ inline void merge_lists_block(Src src, int64_t seg0, int nl, int q, WaveListsT<W>& L,
                                         uint64_t* bk, int64_t* bi, double* oval, int64_t* oidx, Cand* ocand) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    RegTopQ hq;
    hq.init(q);
    for (int g0 = w * 64; g0 < nl; g0 += W * 64) {
        const int g = g0 + lane;
        uint64_t hk = 0;
        int64_t hid = -1;
        src.get(seg0 + (int64_t)(g < nl ? g : nl - 1) * q, hk, hid);  // clamped: no branch around a load
        hq.offer(hk, hid, g < nl && hid >= 0);
    }
    if (lane == 0) {
        bk[w] = readlane64(hq.k, q - 1);
        bi[w] = (int64_t)readlane64((uint64_t)hq.i, q - 1);
    }
    __syncthreads();
    uint64_t fk = 0;
    int64_t fi = INT64_MAX;
    for (int v = 0; v < W; ++v)
        if (bi[v] != INT64_MAX && better(bk[v], bi[v], fk, fi)) {
            fk = bk[v];
            fi = bi[v];
        }
    if (fi != INT64_MAX) fi += 1;  // admit candidates >= T: strictly better than (T.key, T.idx + 1)
    RegTopQ tq;
    tq.init(q, fk, fi);
    for (int g0 = w * 64; g0 < nl; g0 += W * 64) {
        const int g = g0 + lane;
        uint64_t hk = 0;
        int64_t hid = -1;
        src.get(seg0 + (int64_t)(g < nl ? g : nl - 1) * q, hk, hid);  // L1/L2-hot: read in phase 1
        uint64_t m = __ballot(g < nl && hid >= 0 && better(hk, hid, fk, fi));
        while (m) {  // wave-uniform: each list whose head reaches the floor
            const int s = __builtin_ctzll(m);
            m &= m - 1;
            const int64_t base = seg0 + (int64_t)(g0 + s) * q;
            uint64_t ck = 0;
            int64_t ci = -1;
            src.get(base + (lane < q ? lane : q - 1), ck, ci);
            tq.offer(ck, ci, lane < q && ci >= 0);
        }
    }
    block_merge_write<W>(tq, L, q, ocand, 0, ocand ? nullptr : oval, oidx);
}

// Arrival ticket of a stage-1 grid (a.ctr != nullptr: stage 2 folded into
// stage 1): after its list is written (write-through), every block arrives;
// the last to arrive resets the counter and merges the grid's lists into the
// final output / records.
// The best (k, i) of each group of GS lanes in all its lanes (butterfly).
template <int GS>
__device__ __forceinline__ void group_best(uint64_t& k, int64_t& i) {
    uint64_t pk;
    int64_t pi;
#define CE_GB(J)                    \
    if constexpr (GS > J) {         \
        pk = k;                     \
        pi = i;                     \
        xor_cand<J>(pk, pi);        \
        if (better(pk, pi, k, i)) { \
            k = pk;                 \
            i = pi;                 \
        }                           \
    }
    CE_GB(1) CE_GB(2) CE_GB(4) CE_GB(8)
#undef CE_GB
}

// The fold's merge, one block of W waves over nl <= 64 * W * kLeanJ lists
// handed off in this launch (sc1 loads), in two rounds of loads:
//   1. every thread loads the heads of its lists (t, t + 64W, ...); the best
//      head per group of W lanes gives 64 group bests -- heads of 64 distinct
//      lists -- and the one of rank q-1 is an exact floor T (q lists hold an
//      entry >= T, so every global top-q candidate is >= T); none when fewer
//      than q groups hold a list;
//   2. every thread walks the lists it loaded whose head is >= T: a list's
//      entries >= T are a prefix of it (best-first), read 8 at a time, and
//      appended to a survivor list; every survivor takes the output slot of
//      its rank among the survivors.
// The walk reads only the prefixes (for q = 10 on random data: ~q survivors
// in ~q lists, one round of loads), so q up to 64 stays on this path (round 3
// loaded every entry of every qualifying list, nq * q, and fell back for any
// q > 16).  More than 64 * W survivors (floods of ties at T): the
// register-list merge (merge_lists_block) -- round 2 measured it at ~20 us as
// the last block of the 100M-item grid (sequential per-list loads, sort
// networks on cold lists).
constexpr int kLeanJ = 8;
template <int W>
struct LeanMergeSmem {
    uint64_t gk[64];
    int64_t gi[64];
    int part[W][64];
    int nsurv, ticket;
    uint64_t bk[W];
    int64_t bi[W];
};

template <int W, class Src>
__device__ inline void merge_lists_lean(Src src, int nl, int q, WaveListsT<W>& L, LeanMergeSmem<W>& sm,
                                        double* oval, int64_t* oidx, Cand* ocand) {
    constexpr int BS = 64 * W, GS = W;  // lanes per group: 64 groups
    constexpr int CAP = 64 * W;         // survivors held (the block-merge scratch)
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    uint64_t* sk = &L.key[0][0];  // survivors: the block-merge scratch, 64 W slots
    int64_t* si = &L.idx[0][0];
    // 1. heads, all loads in flight
    uint64_t hk[kLeanJ];
    int64_t hi[kLeanJ];
#pragma unroll
    for (int j = 0; j < kLeanJ; ++j) {
        hk[j] = 0;
        hi[j] = INT64_MAX;
        const int g = tid + BS * j;
        if (g < nl) src.get((int64_t)g * q, hk[j], hi[j]);
    }
    uint64_t bk = 0;
    int64_t bi = INT64_MAX;
#pragma unroll
    for (int j = 0; j < kLeanJ; ++j) {
        if (hi[j] < 0) hi[j] = INT64_MAX;  // empty list: no head
        if (hi[j] != INT64_MAX && better(hk[j], hi[j], bk, bi)) {
            bk = hk[j];
            bi = hi[j];
        }
    }
    group_best<GS>(bk, bi);
    if ((tid & (GS - 1)) == 0) {
        sm.gk[tid / GS] = bk;
        sm.gi[tid / GS] = bi;
    }
    if (tid == 0) sm.nsurv = 0;
    __syncthreads();
    {
        const uint64_t mk = sm.gk[lane];
        const int64_t mi = sm.gi[lane];
        int r = 0;
#pragma unroll
        for (int j = 0; j < 64 / W; ++j) {
            const int o = w * (64 / W) + j;
            r += better(sm.gk[o], sm.gi[o], mk, mi);
        }
        sm.part[w][lane] = r;
    }
    __syncthreads();
    uint64_t fk = 0;  // no floor: admit everything
    int64_t fi = INT64_MAX;
    {
        int r = 0;
#pragma unroll
        for (int j = 0; j < W; ++j) r += sm.part[j][lane];
        const uint64_t hit = __ballot(r == q - 1 && sm.gi[lane] != INT64_MAX);
        if (hit) {
            const int sl = __builtin_ctzll(hit);
            fk = sm.gk[sl];
            fi = sm.gi[sl];
        }
    }
    // 2. the prefix >= T of every list whose head is >= T, 8 entries per round.
    // Rolled, re-reading the head (L2-hot) instead of indexing hk / hi: a runtime
    // index would put them in scratch, an unrolled walk raises the register
    // peak of every streaming kernel this merge is inlined into.
#pragma unroll 1
    for (int j = 0; j < kLeanJ; ++j) {
        const int g = tid + BS * j;
        if (g >= nl) break;
        const int64_t base = (int64_t)g * q;
        uint64_t h0;
        int64_t i0;
        src.get(base, h0, i0);
        if (i0 < 0 || better(fk, fi, h0, i0)) continue;
#pragma unroll 1
        for (int e0 = 0; e0 < q; e0 += 8) {
            uint64_t ck[8];
            int64_t ci[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) src.get(base + (e0 + u < q ? e0 + u : q - 1), ck[u], ci[u]);  // clamped
            int take = 0;  // the leading entries of this round that are >= T
#pragma unroll
            for (int u = 0; u < 8; ++u)
                take += (take == u && e0 + u < q && ci[u] >= 0 && !better(fk, fi, ck[u], ci[u])) ? 1 : 0;
            const int s0 = take ? atomicAdd(&sm.nsurv, take) : 0;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u < take && s0 + u < CAP) {
                    sk[s0 + u] = ck[u];
                    si[s0 + u] = ci[u];
                }
            if (take < 8) break;
        }
    }
    __syncthreads();
    const int ns = sm.nsurv;
    if (ns > CAP) {  // block-uniform: floods of ties at T -> the register-list merge
        merge_lists_block<W>(src, 0, nl, q, L, sm.bk, sm.bi, oval, oidx, ocand);
        return;
    }
    if (tid < ns) {
        const uint64_t mk = sk[tid];
        const int64_t mi = si[tid];
        int r = 0;
        for (int j = 0; j < ns; ++j) r += better(sk[j], si[j], mk, mi);
        if (r < q) {
            if (ocand) {
                ocand[r] = Cand{mk, mi};
            } else {
                oval[r] = key_to_val(mk);
                oidx[r] = mi;
            }
        }
    }
    for (int r = ns + tid; r < q; r += BS) {  // fewer candidates than q: padding
        if (ocand) {
            ocand[r] = Cand{0ull, -1};
        } else {
            oval[r] = __longlong_as_double(0x7ff8000000000000ll);
            oidx[r] = -1;
        }
    }
}

template <int W>
__device__ inline void fold_merge(uint32_t* ctr, double* oval, int64_t* oidx, Cand* ocand, int q, const Cand* wc0,
                                  WaveListsT<W>& L, const Cand* extra = nullptr, uint32_t* claim = nullptr) {
    __shared__ LeanMergeSmem<W> ms;
    if (!arrive_last(ctr, gridDim.x, &ms.ticket)) return;  // block-uniform
    // claim: the grid's tile-claim word (k_stream_nmc).  Every block has arrived,
    // so every claim of the launch has returned: back to zero for the next launch
    // (write-through, like the lists)
    if (claim && threadIdx.x == 0) __hip_atomic_store(claim, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // extra (a chunked job's running list) may be ocand itself: every input is
    // read before the outputs are written (barriers in between)
    const int nl = (int)gridDim.x + (extra ? 1 : 0);
    const FoldSrc src{wc0, (int64_t)gridDim.x * q, extra};
    if (nl <= 64 * W * kLeanJ)
        merge_lists_lean<W>(src, nl, q, L, ms, oval, oidx, ocand);
    else
        merge_lists_block<W>(src, 0, nl, q, L, ms.bk, ms.bi, oval, oidx, ocand);
}

// ---------------------------------------------------------------------------
// Stage 2: merge `nl` lists of q slots (per segment = blockIdx.x) into top-q.
// A list's worst entry bounds the answer from below: with T = the best of the
// full lists' worst entries, at least q candidates are >= T, so only
// candidates >= T can be selected -- the filter is exact and usually leaves
// ~q survivors.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void wave_best(uint64_t& k, int64_t& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t k2 = __shfl_xor(k, off);
        const int64_t i2 = __shfl_xor(i, off);
        if (better(k2, i2, k, i)) {
            k = k2;
            i = i2;
        }
    }
}

// ocand != nullptr: the top-q as candidate records instead of (val, idx).
template <bool FROM_VALS, int CAP, int BS, int IPT>
__global__ __launch_bounds__(BS) void k_finish(ListSrc<FROM_VALS> src, int nl, int q,
                                               double* __restrict__ oval, int64_t* __restrict__ oidx,
                                               Cand* __restrict__ ocand) {
    __shared__ TopQSmem<CAP> sm;
    __shared__ uint64_t wk[BS / 64];
    __shared__ int64_t wi[BS / 64];
    const int64_t seg0 = (int64_t)blockIdx.x * nl * q;
    const int64_t L = (int64_t)nl * q;
    // 1. T = best over FULL lists of the list's worst entry; lists are
    //    best-first, so a list is full iff slot q-1 is used and that slot is
    //    its worst entry: one load per list.
    uint64_t tk = 0;
    int64_t ti = INT64_MAX;  // "nothing": admits every candidate
    for (int g = threadIdx.x; g < nl; g += BS) {
        uint64_t k;
        int64_t i;
        src.get(seg0 + (int64_t)g * q + q - 1, k, i);
        if (i >= 0 && better(k, i, tk, ti)) {
            tk = k;
            ti = i;
        }
    }
    wave_best(tk, ti);
    if (lane_id() == 0) {
        wk[threadIdx.x >> 6] = tk;
        wi[threadIdx.x >> 6] = ti;
    }
    __syncthreads();
    tk = wk[0];
    ti = wi[0];
    for (int w = 1; w < BS / 64; ++w)
        if (better(wk[w], wi[w], tk, ti)) {
            tk = wk[w];
            ti = wi[w];
        }
    // admit candidates >= T: strictly better than (T.key, T.idx + 1)
    TopQ<CAP, BS> tq(sm);
    tq.init(tk, ti == INT64_MAX ? INT64_MAX : ti + 1);
    // 2. filter every candidate; IPT independent loads per thread in flight
    //    (addresses clamped, never a branch around a load)
    for (int64_t b0 = 0; b0 < L; b0 += (int64_t)BS * IPT) {
        uint64_t k[IPT];
        int64_t id[IPT];
#pragma unroll
        for (int u = 0; u < IPT; ++u) {
            int64_t j = b0 + (int64_t)u * BS + threadIdx.x;
            const bool in = j < L;
            src.get(seg0 + (in ? j : L - 1), k[u], id[u]);
            if (!in) id[u] = -1;
        }
#pragma unroll
        for (int u = 0; u < IPT; ++u) {
            if (b0 + (int64_t)u * BS >= L) break;  // block-uniform
            tq.offer(k[u], id[u], id[u] >= 0);
            tq.end_round(q, BS);
        }
    }
    const int cnt = tq.finish(q);
    const int64_t slot = (int64_t)blockIdx.x * q;
    if (ocand) write_list<CAP, false>(sm, cnt, q, ocand + slot, nullptr, nullptr);
    else write_list<CAP, true>(sm, cnt, q, nullptr, oval + slot, oidx + slot);
}

// Stage 2 for q <= kHeadsMaxQ (the common case, q = 10).  The lists are
// best-first, so list heads are each list's best entry; T1 = the q-th best
// head is an exact lower bound (q distinct lists hold an entry >= T1) and a
// tight one: the global top-q sit in ~q different lists, so only ~q
// candidates survive the filter.  Cost: one 1024-entry bitonic sort of the
// heads + one pass over the (prefetched) candidates + a tiny final sort.
constexpr int kHeadsBS = 1024;
constexpr int kHeadsMaxQ = 512;

template <bool FROM_VALS, int IPT>
__global__ __launch_bounds__(kHeadsBS) void k_finish_heads(ListSrc<FROM_VALS> src, int nl, int q,
                                                           double* __restrict__ oval, int64_t* __restrict__ oidx,
                                                           Cand* __restrict__ ocand) {
    __shared__ TopQSmem<2048> sm;
    const int64_t seg0 = (int64_t)blockIdx.x * nl * q;
    const int64_t L = (int64_t)nl * q;
    const int tid = threadIdx.x;
    // prefetch this thread's first IPT candidates (clamped, unconditional)
    uint64_t k[IPT];
    int64_t id[IPT];
#pragma unroll
    for (int u = 0; u < IPT; ++u) {
        const int64_t j = (int64_t)u * kHeadsBS + tid;
        src.get(seg0 + (j < L ? j : L - 1), k[u], id[u]);
        if (j >= L) id[u] = -1;
    }
    // best head among this thread's lists (distinct threads -> distinct lists)
    uint64_t hk = 0;
    int64_t hi = INT64_MAX;
    for (int g = tid; g < nl; g += kHeadsBS) {
        uint64_t kk;
        int64_t ii;
        src.get(seg0 + (int64_t)g * q, kk, ii);
        if (ii >= 0 && better(kk, ii, hk, hi)) {
            hk = kk;
            hi = ii;
        }
    }
    TopQ<2048, kHeadsBS> tq(sm);
    uint64_t tk = 0;
    int64_t ti = INT64_MAX;
    if (q <= kHeadsBS / 64) {
        // q <= 16: each wave's best head (shuffle reduction) comes from a list
        // of its own; the q-th best of those 16 is the bound.
        wave_best(hk, hi);
        const int w = tid >> 6;
        if ((tid & 63) == 0) {
            sm.key[w] = hk;
            sm.idx[w] = hi;
        }
        __syncthreads();
        if (tid < kHeadsBS / 64) {
            int rank = 0;
            for (int v = 0; v < kHeadsBS / 64; ++v) rank += better(sm.key[v], sm.idx[v], sm.key[tid], sm.idx[tid]);
            if (rank == q - 1) {
                sm.red[0] = sm.key[tid];
                sm.red[1] = (uint64_t)sm.idx[tid];
            }
        }
        __syncthreads();
        const int64_t t1 = (int64_t)sm.red[1];
        if (t1 != INT64_MAX) {  // >= q non-empty lists
            tk = sm.red[0];
            ti = t1 + 1;  // admit candidates >= T1
        }
    } else {
        sm.key[tid] = hk;
        sm.idx[tid] = hi;
        tq.sort_buffer(kHeadsBS);  // barrier inside, before the first compare
        __syncthreads();
        if (q <= kHeadsBS && sm.idx[q - 1] != INT64_MAX) {
            tk = sm.key[q - 1];
            ti = sm.idx[q - 1] + 1;
        }
    }
    __syncthreads();
    tq.init(tk, ti);
    for (int64_t b0 = 0; b0 < L; b0 += (int64_t)kHeadsBS * IPT) {
        if (b0 > 0) {
#pragma unroll
            for (int u = 0; u < IPT; ++u) {
                const int64_t j = b0 + (int64_t)u * kHeadsBS + tid;
                src.get(seg0 + (j < L ? j : L - 1), k[u], id[u]);
                if (j >= L) id[u] = -1;
            }
        }
#pragma unroll
        for (int u = 0; u < IPT; ++u) {
            if (b0 + (int64_t)u * kHeadsBS >= L) break;  // block-uniform
            tq.offer(k[u], id[u], id[u] >= 0);
            tq.end_round(q, kHeadsBS);
        }
    }
    const int cnt = tq.finish(q);
    const int64_t slot = (int64_t)blockIdx.x * q;
    if (ocand) write_list<2048, false>(sm, cnt, q, ocand + slot, nullptr, nullptr);
    else write_list<2048, true>(sm, cnt, q, nullptr, oval + slot, oidx + slot);
}

// Stage 2 for q <= 64.  The lists are best-first, so a list's head is its
// best entry.  Phase 1: each of the 16 waves sorts the heads of its share of
// the lists (one per lane) in registers; its q-th best head T_w is an exact
// lower bound (q distinct lists have an entry >= T_w), and so is T = the best
// T_w.  Phase 2: the waves stream all candidates (64 consecutive per wave per
// step, PF steps in flight) through register top-q lists floored at T -- only
// candidates >= T (~q of them) are ever inserted -- and the lists are
// tree-merged.  Output: final (val, idx), or candidate records (wc) for an
// exchange between ranks.
template <bool FROM_VALS>
__global__ __launch_bounds__(1024) void k_merge_reg(ListSrc<FROM_VALS> src, int nl, int q,
                                                    double* __restrict__ oval, int64_t* __restrict__ oidx,
                                                    Cand* __restrict__ ocand) {
    __shared__ WaveListsT<16> sm;
    __shared__ uint64_t bk[16];
    __shared__ int64_t bi[16];
    constexpr int PF = 10;  // 16 x 64 x 10: 1024 lists of q = 10 in one round of loads
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t seg0 = (int64_t)blockIdx.x * nl * q;
    const int64_t L = (int64_t)nl * q;
    CE_DASSERT(nl >= 1 && q >= 1 && q <= kStreamMaxQ);
    // the first round of candidate loads goes out before the head phase
    uint64_t k[PF];
    int64_t id[PF];
    auto load_round = [&](int64_t c0) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int64_t j = c0 + (int64_t)u * 16 * 64 + lane;
            src.get(seg0 + (j < L ? j : L - 1), k[u], id[u]);  // clamped: no branch around a load
            if (j >= L) id[u] = -1;
        }
    };
    load_round((int64_t)w * 64);
    // phase 1: the head bound (only worth a sort when there are many lists)
    uint64_t fk = 0;
    int64_t fi = INT64_MAX;
    if (nl > 64) {
        RegTopQ hq;
        hq.init(q);
        for (int g0 = w * 64; g0 < nl; g0 += 16 * 64) {
            const int g = g0 + lane;
            uint64_t hk = 0;
            int64_t hid = -1;
            src.get(seg0 + (int64_t)(g < nl ? g : nl - 1) * q, hk, hid);
            hq.offer(hk, hid, g < nl && hid >= 0);
        }
        const uint64_t qk = readlane64(hq.k, q - 1);
        const int64_t qi = (int64_t)readlane64((uint64_t)hq.i, q - 1);
        if (lane == 0) {
            bk[w] = qk;
            bi[w] = qi;
        }
        __syncthreads();
        for (int v = 0; v < 16; ++v)
            if (bi[v] != INT64_MAX && better(bk[v], bi[v], fk, fi)) {
                fk = bk[v];
                fi = bi[v];
            }
        if (fi != INT64_MAX) fi += 1;  // admit candidates >= T: strictly better than (T.key, T.idx + 1)
    }
    RegTopQ tq;
    tq.init(q, fk, fi);
    for (int64_t c0 = (int64_t)w * 64; c0 < L; c0 += (int64_t)16 * 64 * PF) {
        if (c0 != (int64_t)w * 64) load_round(c0);
#pragma unroll
        for (int u = 0; u < PF; ++u) tq.offer(k[u], id[u], id[u] >= 0);
    }
    const int64_t slot = (int64_t)blockIdx.x * q;
    if (ocand)
        block_merge_write<16>(tq, sm, q, ocand + slot, 0);
    else
        block_merge_write<16>(tq, sm, q, nullptr, 0, oval + slot, oidx + slot);
}

// Per-segment merge of a few lists (batched users: bpu lists of q each): one
// wave per segment streams its nl*q candidates through a register top-q.
template <bool FROM_VALS>
__global__ __launch_bounds__(256) void k_merge_wave(ListSrc<FROM_VALS> src, int segs, int nl, int q,
                                                    double* __restrict__ oval, int64_t* __restrict__ oidx) {
    const int seg = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (seg >= segs) return;  // wave-uniform; no block barrier below
    const int64_t L = (int64_t)nl * q, seg0 = (int64_t)seg * L;
    RegTopQ tq;
    tq.init(q);
    for (int64_t c0 = 0; c0 < L; c0 += 64) {
        const int64_t j = c0 + lane;
        uint64_t k;
        int64_t id;
        src.get(seg0 + (j < L ? j : L - 1), k, id);
        tq.offer(k, id, j < L && id >= 0);
    }
    if (lane < q) {
        const bool ok = tq.i != INT64_MAX;
        oval[(int64_t)seg * q + lane] = ok ? key_to_val(tq.k) : __longlong_as_double(0x7ff8000000000000ll);
        oidx[(int64_t)seg * q + lane] = ok ? tq.i : -1;
    }
}

}  // namespace ce
