// ce_wave.hpp -- wave-level (wave64) building blocks of every list kernel:
// lane exchange without the LDS crossbar, the bitonic sort / merge of 64
// (key, position) pairs across a wave, the per-wave register top-q (RegTopQ),
// the block's merge of its wave lists (WaveListsT, block_merge_write) with the
// write-through hand-off of a list to another block of the same launch
// (store_cand_wt / load_cand_wt / arrive_last), the exclusion-bitmap test and
// the no-op hook.  Device functions only, no kernel: the streaming, wide,
// small-pool, frames, sort, merge and member kernels all build on these.
#pragma once
#include "ce_device.hpp"
#include "ce_topq.hpp"  // Cand

namespace ce {

// ---------------------------------------------------------------------------
// Per-wave top-q held in registers (q <= 64): lane L holds the L-th best
// (order key, position) of the wave so far, best first; empty slots hold the
// sentinel (0, INT64_MAX), worse than every real candidate (no finite, inf or
// NaN entropy maps to key 0).  The threshold is slot q-1, read into scalar
// registers.  A candidate that beats it is rare once the stream is warm: one
// or a few are inserted in place (ballot for the position + one lane shift);
// a large batch (the first tiles) is bitonic-sorted across the wave and
// merged with the list -- shuffles only, no LDS, no barrier.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// (k, i) from lane `src` (per-lane index) -- ds_bpermute on the four halves
__device__ __forceinline__ void shfl_cand(uint64_t& k, int64_t& i, int src) {
    const int a = src << 2;
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)(uint32_t)k);
    const uint32_t k1 = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)(uint32_t)(k >> 32));
    const uint32_t i0 = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)(uint32_t)(uint64_t)i);
    const uint32_t i1 = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)(uint32_t)((uint64_t)i >> 32));
    k = ((uint64_t)k1 << 32) | k0;
    i = (int64_t)(((uint64_t)i1 << 32) | i0);
}

// Lane exchange "value of lane ^ J" without the LDS crossbar (ds_bpermute
// throughput, not latency, bounded the sort networks): DPP quad_perm for J =
// 1, 2; row_half_mirror (lane ^ 7) then quad reverse (lane ^ 3) for J = 4;
// row_ror:8 for J = 8; the gfx950 permlane16/32 swaps for J = 16, 32.
template <int J>
__device__ __forceinline__ uint32_t xor_lane(uint32_t v) {
    if constexpr (J == 1) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
    } else if constexpr (J == 2) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
    } else if constexpr (J == 4) {
        const int t = __builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);  // row_half_mirror
        return (uint32_t)__builtin_amdgcn_update_dpp(0, t, 0x1B, 0xF, 0xF, false);      // quad_perm [3,2,1,0]
    } else if constexpr (J == 8) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);  // row_ror:8
    } else if constexpr (J == 16) {
        const auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false);
        return (threadIdx.x & 16) ? p[0] : p[1];
    } else {
        static_assert(J == 32, "lane exchange distance");
        const auto p = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return (threadIdx.x & 32) ? p[0] : p[1];
    }
}

// value of lane - 1 (DPP wave_shr:1)
__device__ __forceinline__ uint64_t lane_above(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x138, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x138, 0xF, 0xF, false);
    return ((uint64_t)hi << 32) | lo;
}

template <int J>
__device__ __forceinline__ void xor_cand(uint64_t& k, int64_t& i) {
    const uint32_t k0 = xor_lane<J>((uint32_t)k), k1 = xor_lane<J>((uint32_t)(k >> 32));
    const uint32_t i0 = xor_lane<J>((uint32_t)(uint64_t)i), i1 = xor_lane<J>((uint32_t)((uint64_t)i >> 32));
    k = ((uint64_t)k1 << 32) | k0;
    i = (int64_t)(((uint64_t)i1 << 32) | i0);
}

// One compare-exchange stage of a bitonic network across the wave: partner
// lane ^ J; `desc` = this lane's block sorts best-first.
template <int J>
__device__ __forceinline__ void cx_stage(uint64_t& k, int64_t& i, bool desc) {
    const int lane = threadIdx.x & 63;
    uint64_t pk = k;
    int64_t pi = i;
    xor_cand<J>(pk, pi);
    const bool lower = (lane & J) == 0;
    const bool pb = better(pk, pi, k, i);
    const bool take = (lower == desc) ? pb : !pb;
    if (take) {
        k = pk;
        i = pi;
    }
}

template <int S, int J>
__device__ __forceinline__ void sort_stages(uint64_t& k, int64_t& i) {
    cx_stage<J>(k, i, ((threadIdx.x & 63) & S) == 0);
    if constexpr (J > 1) sort_stages<S, J / 2>(k, i);
}

template <int S>
__device__ __forceinline__ void sort_levels(uint64_t& k, int64_t& i) {
    sort_stages<S, S / 2>(k, i);
    if constexpr (S < 64) sort_levels<S * 2>(k, i);
}

// The wave's best (k, i) in every lane (6 butterfly stages).
template <int J>
__device__ __forceinline__ void best_stages(uint64_t& k, int64_t& i) {
    uint64_t pk = k;
    int64_t pi = i;
    xor_cand<J>(pk, pi);
    if (better(pk, pi, k, i)) {
        k = pk;
        i = pi;
    }
    if constexpr (J < 32) best_stages<J * 2>(k, i);
}
__device__ __forceinline__ void wave_best64(uint64_t& k, int64_t& i) { best_stages<1>(k, i); }

// Each 16-lane row's best (k, i) in all its lanes (4 butterfly stages).
__device__ __forceinline__ void row_best16(uint64_t& k, int64_t& i) {
    uint64_t pk;
    int64_t pi;
#define CE_RB(J)                          \
    pk = k;                               \
    pi = i;                               \
    xor_cand<J>(pk, pi);                  \
    if (better(pk, pi, k, i)) {           \
        k = pk;                           \
        i = pi;                           \
    }
    CE_RB(1) CE_RB(2) CE_RB(4) CE_RB(8)
#undef CE_RB
}

// Sort the wave's 64 (k, i) best-first (21 stages).
__device__ __forceinline__ void wave_sort64(uint64_t& k, int64_t& i) { sort_levels<2>(k, i); }

// (k, i) := best 64 of the two best-first lists (k, i) and (bk, bi), best-first.
__device__ __forceinline__ void wave_merge64(uint64_t& k, int64_t& i, uint64_t bk, int64_t bi) {
    const int lane = threadIdx.x & 63;
    shfl_cand(bk, bi, 63 - lane);  // reversed: list max(A[L], B[63-L]) is bitonic
    if (better(bk, bi, k, i)) {
        k = bk;
        i = bi;
    }
    sort_stages<64, 32>(k, i);  // half-cleaners 32 .. 1, all best-first
}

// no-op callback of CommitteeSrc::keys / rows_small (ce_src.hpp)
struct NoHook {
    __device__ __forceinline__ void operator()() const {}
};

// bit i of an exclusion bitmap (SelectionSession: items already queried)
__device__ __forceinline__ bool excluded(const uint32_t* b, int64_t i) { return (b[i >> 5] >> (i & 31)) & 1u; }

struct RegTopQ {
    uint64_t k;   // this lane's slot
    int64_t i;
    uint64_t tk;  // threshold = the better of slot q-1 and the floor (wave-uniform)
    int64_t ti;
    uint64_t fk;  // floor: a known exact lower bound (only candidates beating it can be selected)
    int64_t fi;
    int q;

    __device__ __forceinline__ void init(int q_, uint64_t fk_ = 0, int64_t fi_ = INT64_MAX) {
        k = 0;
        i = INT64_MAX;
        tk = fk = fk_;
        ti = fi = fi_;
        q = q_;
    }

    __device__ __forceinline__ void refresh() {
        const uint64_t sk = readlane64(k, q - 1);
        const int64_t si = (int64_t)readlane64((uint64_t)i, q - 1);
        const bool s_better = better(sk, si, fk, fi);
        tk = s_better ? sk : fk;
        ti = s_better ? si : fi;
    }

    // the list holds no candidate (wave-uniform)
    __device__ __forceinline__ bool empty() const { return readlane64((uint64_t)i, 0) == (uint64_t)INT64_MAX; }

    // insert one wave-uniform candidate that beats the threshold
    __device__ __forceinline__ void insert(uint64_t ck, int64_t ci) {
        const int lane = threadIdx.x & 63;
        const uint64_t below = __ballot(better(ck, ci, k, i));  // slots the candidate beats: a suffix
        const int p = __builtin_ctzll(below);
        const uint64_t uk = lane_above(k);  // lane 0 never takes it
        const int64_t ui = (int64_t)lane_above((uint64_t)i);
        if (lane > p) {
            k = uk;
            i = ui;
        } else if (lane == p) {
            k = ck;
            i = ci;
        }
    }

    __device__ __forceinline__ void offer(uint64_t ck, int64_t ci, bool valid) {
        const bool pass = valid && better(ck, ci, tk, ti);
        uint64_t mask = __ballot(pass);
        if (mask == 0) return;  // wave-uniform: the common case
        if (__popcll(mask) <= 8) {
            do {
                const int s = __builtin_ctzll(mask);
                mask &= mask - 1;
                const uint64_t sk = readlane64(ck, s);
                const int64_t si = (int64_t)readlane64((uint64_t)ci, s);
                if (better(sk, si, tk, ti)) {  // re-check: earlier inserts raised the bar
                    insert(sk, si);
                    refresh();
                }
            } while (mask);
        } else {
            uint64_t bk = pass ? ck : 0ull;
            int64_t bi = pass ? ci : INT64_MAX;
            wave_sort64(bk, bi);
            if (empty()) {
                k = bk;
                i = bi;
            } else {
                wave_merge64(k, i, bk, bi);
            }
            refresh();
        }
    }
};

// kStreamMaxQ (64: one list slot per lane): ce_ws.hpp

// block-merge scratch: the wave lists, 64 slots each
template <int WAVES>
struct WaveListsT {
    uint64_t key[WAVES][64];
    int64_t idx[WAVES][64];
};
using WaveLists = WaveListsT<4>;

// Merge the block's WAVES wave lists (registers, best-first) into the
// block's top-q and write it: to the workspace (wc) or as final (val, idx)
// outputs.  A tree over the waves: at level s, waves w = s mod 2s park their
// list in LDS and waves w = 0 mod 2s merge it in (7 shuffle stages); every
// LDS slot is written once and read once, one barrier per level.
// nw = waves taking part (a power of two <= WAVES; default all of them).
// Cross-block hand-off inside one launch (MI355X_MICROARCH.md, "Valid forms",
// the table's first row): every handed-off byte is stored write-through (sc1:
// relaxed agent-scope atomic stores), every storing wave waits for its stores
// (s_waitcnt vmcnt(0)), the block syncs and ONE lane adds to the problem's
// arrival counter (agent scope); the block whose add returns the last ticket
// reads the bytes with sc1 loads only (relaxed agent-scope atomic loads).  No
// L2 write-back or invalidate: a __threadfence() per block (buffer_wbl2 +
// buffer_inv) made the 1000-block batched launch 118 us instead of ~14.
__device__ __forceinline__ void store_cand_wt(Cand* p, uint64_t k, int64_t i) {
    __hip_atomic_store(&p->key, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&p->idx, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ Cand load_cand_wt(const Cand* p) {
    Cand c;
    c.key = __hip_atomic_load(&p->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c.idx = __hip_atomic_load(&p->idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return c;
}
// Every thread of the block calls it after its write-through stores; true in
// every thread of the block whose arrival is the n-th.  The counter wraps
// itself: global_atomic_inc with limit n - 1 returns 0..n-1 and stores 0 after
// the n-th arrival, so the counter is zero again once every block has arrived
// (and stays in [0, n) even when a misuse -- two launches sharing one
// workspace -- interleaves their arrivals: it does not stay broken).
__device__ __forceinline__ bool arrive_last(uint32_t* ctr, uint32_t n, int* lds_ticket) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) *lds_ticket = (int)__builtin_amdgcn_atomic_inc32(ctr, n - 1, __ATOMIC_RELAXED, "agent");
    __syncthreads();
    const int t = *lds_ticket;
    CE_DASSERT(t >= 0 && t < (int)n);
    return t == (int)n - 1;
}

// wt: the list at wc is read inside this launch (a fold / tile merge): store
// it write-through (store_cand_wt).
template <int WAVES>
__device__ inline void block_merge_write(const RegTopQ& tq, WaveListsT<WAVES>& L, int q, Cand* wc, int nlists,
                                         double* oval = nullptr, int64_t* oidx = nullptr, int nw = WAVES,
                                         bool wt = false) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // empty lists for the workspace slots no block of this (occupancy-sized)
    // grid owns: b + gridDim.x, b + 2*gridDim.x, ...
    for (int64_t s = (int64_t)blockIdx.x + gridDim.x; s < nlists; s += gridDim.x)
        for (int r = threadIdx.x; r < q; r += blockDim.x) wc[(s - blockIdx.x) * q + r] = Cand{0ull, -1};
    uint64_t k = tq.k;
    int64_t i = tq.i;
    for (int s = 1; s < WAVES && s < nw; s <<= 1) {  // block-uniform bound
        if ((w & (2 * s - 1)) == s) {
            L.key[w][lane] = k;
            L.idx[w][lane] = i;
        }
        __syncthreads();
        if ((w & (2 * s - 1)) == 0) {
            const uint64_t bk = L.key[w + s][lane];
            const int64_t bi = L.idx[w + s][lane];
            if (readlane64((uint64_t)bi, 0) != (uint64_t)INT64_MAX) {  // partner list not empty
                if (readlane64((uint64_t)i, 0) == (uint64_t)INT64_MAX) {
                    k = bk;  // own list empty: take the partner's as is
                    i = bi;
                } else {
                    wave_merge64(k, i, bk, bi);
                }
            }
        }
    }
    if (w == 0 && lane < q) {
        const bool ok = i != INT64_MAX;
        if (oval) {
            oval[lane] = ok ? key_to_val(k) : __longlong_as_double(0x7ff8000000000000ll);
            oidx[lane] = ok ? i : -1;
        } else if (wt) {
            store_cand_wt(wc + lane, ok ? k : 0ull, ok ? i : -1);
        } else {
            wc[lane] = Cand{ok ? k : 0ull, ok ? i : -1};
        }
    }
}

}  // namespace ce
