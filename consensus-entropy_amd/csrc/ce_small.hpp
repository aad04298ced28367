// ce_small.hpp -- pools of a few thousand items (BASELINE configs[0..2]: one
// reference-sized pool, the hc table, the [mc; hc] mix, 500 users in one
// launch), each problem (the pool, a user, the mix) selected by ONE block:
//
// Per block (amg_test.py:441-445 on the problem's items):
//   1. the log table's loads are issued, then the member loads of the
//      thread's item slots (item lo + tid + BS*v: each wave's loads coalesced);
//      each item's exact consensus row (f64 means) is formed as soon as its
//      own loads have landed, and kept in registers; from it an APPROXIMATE
//      entropy -- f32 copies, one hardware reciprocal, one hardware log2 per
//      class -- within e = kApproxErr2PerClass * C of the exact one (log2
//      units; ce_device.hpp), as a 32-bit key;
//   2. the max approximate key of each group of BS/64 lanes (DPP) -> 64 group
//      maxima (distinct items) in LDS; every thread counts, for one of them,
//      the maxima above / not below it over a 1/W slice; the value T of rank
//      q-1 has q distinct items at or above it;
//   3. survivors = items whose approximate entropy is >= T - 2 e,
//      plus every "special" row (negative / non-finite means, a sum outside
//      [2^-100, 2^100]: NaN / -inf entropies and the like, which the
//      approximation does not cover): a superset of the exact top q (q items
//      are exactly >= T - eps, so an item below T - eps cannot be among them,
//      and its approximation is below T - 2 eps).  Their rows go to LDS (one
//      atomic per wave);
//   4. the survivors' EXACT entropies (glibc log, scipy's quotients:
//      bit-identical to the reference), P = C rounded up to 2/4/8 lanes per
//      survivor, one class per lane (the wave issues each instruction once
//      for all lanes: one log chain instead of C in a row), terms gathered by
//      lane shuffles and summed in numpy's order; then every survivor counts
//      the survivors that beat it -- (key, ~local slot) triples, a 96-bit
//      subtract's borrow (add_if_beats) -- and writes itself to output slot
//      `rank` (< q).  Up to 64/P survivors (the usual case) are evaluated and
//      ranked by wave 0 alone, with no second block barrier.
// The exact entropy (the ~150-VALU glibc-log row) runs for the ~q survivors
// only, not for every item: the keys phase of round 3 was VALU-bound at two
// blocks per CU (configs[2]).  The local slot v*BS+tid orders a problem's
// items as their positions do, so no position array stays live.
// A problem longer than BS*IPT items (a long user of a ragged batch), or more
// than 64*W survivors (floods of near-ties at the floor), takes per-wave
// register lists + a tree merge instead (block-uniform branches, same answer).
#pragma once
#include "ce_src.hpp"     // kSmallThrottle, NoHook
#include "ce_stream.hpp"  // stream_direct_range
#include "ce_wave.hpp"

namespace ce {

#ifdef CE_PHASE_TIMING
// diagnostic build only (-DCE_PHASE_TIMING): per-block wall-clock stamps (100 MHz)
// [0] start, [1] wave 0's keys done, [2] floor, [3] append, [4] rank, [5] exact keys (wave 0),
// [6 + w] wave w's keys done (w < 8)
__device__ uint64_t g_phase[8192][16];
// [14], [15]: shader-clock counter at [0] and [4] (the clock rate over the block)
#define CE_STAMP(b, k)                                        \
    if (threadIdx.x == 0 && (b) < 8192) {                     \
        g_phase[b][k] = wall_clock64();                       \
        if ((k) == 0 || (k) == 4) g_phase[b][14 + (k) / 4] = clock64(); \
    }
#define CE_WSTAMP(b) \
    if ((threadIdx.x & 63) == 0 && (threadIdx.x >> 6) < 8 && (b) < 8192) g_phase[b][6 + (threadIdx.x >> 6)] = wall_clock64();
#else
#define CE_STAMP(b, k)
#define CE_WSTAMP(b)
#endif

// Geometry: block p selects problem p -- segment A (committee items: one
// pool [0, n) or user p's [offsets[p], offsets[p+1])) and, for the mix,
// segment B (the hc rows [0, nB), positions n + row).
struct TileArgs {
    const int64_t* offsets;  // [P+1] problem offsets (batched users), or nullptr: one problem
    int64_t n;               // segment-A items (offsets == nullptr)
    int64_t nB;              // segment-B rows (mix), 0 otherwise
    int64_t base_idx;        // position of item 0 (offsets == nullptr)
};

template <int WAVES, int C>
struct TileSmem {
    static constexpr int CAP = 64 * WAVES;  // one survivor per thread
    uint32_t gm[64];                        // group maxima of the approximate keys
    int part[WAVES][64];                    // partial counts (above | not below << 16)
    int cnt;                                // survivors appended
    uint4 cs[CAP + 8];                      // survivors' exact (~local slot, key lo, key hi, -), + 8 zero triples
    union {
        struct {
            double m[C][CAP];               // survivors' exact rows
            uint32_t nl[CAP];               // ... and ~local slots
        } sv;
        WaveListsT<WAVES> lists;            // fallback tree merge
    };
};

// Rows of this thread's IPT items lo + tid + BS*v of [lo, hi) into slots
// [OFF, OFF + IPT): the exact row in m, its approximate key in ak (0: no item
// -- past the end, excluded -- or a special row) and sp (special).  COMMIT:
// `tab` is committed once the first data is awaited -- exactly one tile_rows
// call of a block commits.  Slots outside [OFF, OFF + IPT) are left as they are.
// TAG: 0 for k_select_tiles, 1 for k_select_tiles_mix -- each kernel family its
// own instantiation (and so its own `sink` and row loaders): sharing one moved
// the inliner's choices and with them the ISA of the single-mix kernels.
template <class Src, int IPT, int UNR, int BS, int K, int C, int OFF, bool COMMIT, int THR = kSmallThrottle, int TAG = 0>
__device__ __forceinline__ void tile_rows(const Src& src, int64_t lo, int64_t hi, const uint32_t* excl,
                                          LogTablePrefetch& tab, double (&m)[K][C], uint32_t (&ak)[K],
                                          bool (&sp)[K]) {
    static_assert(OFF + IPT <= K && Src::kC == C, "");
    const int tid = threadIdx.x, w = tid >> 6;
    const int64_t len = hi - lo;
    int64_t items[IPT];
    int nlive = 0;  // this wave's item slots holding at least one real item (a prefix)
#pragma unroll
    for (int v = 0; v < IPT; ++v) {
        const int64_t j = tid + (int64_t)BS * v;
        items[v] = lo + (j < len ? j : (len > 0 ? len - 1 : 0));
        nlive += (int64_t)BS * v + 64 * w < len;
        ak[OFF + v] = 0;
        sp[OFF + v] = false;
#pragma unroll
        for (int c = 0; c < C; ++c) m[OFF + v][c] = 0.0;
    }
    auto sink = [&](int u, const double (&row)[C]) {
#pragma unroll
        for (int c = 0; c < C; ++c) m[OFF + u][c] = row[c];
        bool s;
        const uint32_t a = approx_key<C>(row, s);
        ak[OFF + u] = s ? 0u : a;
        sp[OFF + u] = s;
    };
    if (len > 0) {  // block-uniform
        auto commit = [&]() { tab.commit(); };
        if constexpr (COMMIT) src.template rows_small<UNR, IPT, decltype(sink)&, decltype(commit), THR>(items, nlive, sink, commit);
        else src.template rows_small<UNR, IPT, decltype(sink)&, NoHook, THR>(items, nlive, sink);
    } else if constexpr (COMMIT) {
        tab.commit();
    }
#pragma unroll
    for (int v = 0; v < IPT; ++v) {
        bool ok = tid + (int64_t)BS * v < len;
        if (excl) ok = ok && !excluded(excl, items[v]);
        if (!ok) {
            ak[OFF + v] = 0;
            sp[OFF + v] = false;
        }
    }
}

// r + 1 when triple a beats triple m, (~local slot, key lo, key hi) each: the
// borrow of the 96-bit difference m - a (higher key first, then lower slot) --
// three subtracts and an add-with-carry, no compare masks or scalar ops.
__device__ __forceinline__ int add_if_beats(int r, const uint4& m, const uint4& a) {
    int out;
    uint32_t t;
    asm("v_sub_co_u32 %1, vcc, %2, %5\n\t"
        "v_subb_co_u32 %1, vcc, %3, %6, vcc\n\t"
        "v_subb_co_u32 %1, vcc, %4, %7, vcc\n\t"
        "v_addc_co_u32 %0, vcc, 0, %8, vcc"
        : "=v"(out), "=&v"(t)
        : "v"(m.x), "v"(m.y), "v"(m.z), "v"(a.x), "v"(a.y), "v"(a.z), "v"(r)
        : "vcc");
    return out;
}

// The max of each group of GS lanes in the group's lanes: DPP mirrors within
// quads, half rows and rows (one v_max per step).
template <int GS>
__device__ __forceinline__ uint32_t group_max(uint32_t k) {
#define CE_GM(J, CTL)                                                                              \
    if constexpr (GS > J) {                                                                        \
        const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)k, CTL, 0xF, 0xF, false); \
        k = k > o ? k : o;                                                                         \
    }
    CE_GM(1, 0xB1) CE_GM(2, 0x4E) CE_GM(4, 0x141) CE_GM(8, 0x140)  // quad [1,0,3,2], [2,3,0,1]; half-row, row mirror
#undef CE_GM
    return k;
}

// The streaming path's share [wlo, whi) of [a0, a1) for this thread's wave:
// whole iterations of stream_direct_range<.., 2, ..> (2 items per lane), dealt
// to the W waves in order; a wave past the end gets an empty range.
template <int W>
__device__ __forceinline__ void wave_part(int64_t a0, int64_t a1, int64_t& wlo, int64_t& whi) {
    constexpr int64_t kIt = 64 * 2;
    const int w = threadIdx.x >> 6;
    const int64_t its = (a1 - a0 + kIt - 1) / kIt, its_w = (its + W - 1) / W;
    wlo = a0 + (int64_t)w * its_w * kIt;
    whi = wlo + its_w * kIt < a1 ? wlo + its_w * kIt : a1;
    if (wlo > whi) wlo = whi;
}

#define CE_SMALL_FINISH_FRAGMENT  // the two kernels below include ce_small_finish.hpp, nothing else may

// LONG: a problem may exceed BS * IPT items (the per-wave streaming path is
// compiled in).  Launches whose host checks bound the problem (one pool, the
// mix) drop it -- half the code of the kernel.
template <class SrcA, class SrcB, int IPTA, int IPTB, int UNRA, int UNRB, int BS, bool LONG = true>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(LONG ? 4 : BS / 256))) void k_select_tiles(
    SrcA srcA, SrcB srcB, TileArgs ta, int q, double* __restrict__ oval, int64_t* __restrict__ oidx,
    const uint32_t* __restrict__ excl) {
    constexpr int W = BS / 64, GS = BS / 64;  // waves; lanes per group (64 groups)
    constexpr int K = IPTA + IPTB;  // slots: segment A's, then segment B's (both segments in one block)
    static_assert(BS % 64 == 0 && BS >= 128 && GS <= 16 && (GS & (GS - 1)) == 0, "block size");
    constexpr int C = SrcA::kC;
    static_assert(IPTB == 0 || SrcB::kC == C, "both segments' rows have C classes");
    using SM = TileSmem<W, C>;
    __shared__ SM sm;
    CE_STAMP(blockIdx.x, 0)
    LogTablePrefetch tab;
    tab.fetch();
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int p = blockIdx.x;
    const int64_t lo = ta.offsets ? ta.offsets[p] : 0, hi0 = ta.offsets ? ta.offsets[p + 1] : ta.n;
    const int64_t hi = hi0 > lo ? hi0 : lo;
    const int64_t rel = (ta.offsets ? 0 : ta.base_idx) - lo;  // A: position = item + rel
    const int64_t relB = ta.n + ta.base_idx;                  // B: position = row + relB
    // the mix: the block takes every committee item AND every hc row (slots [0, IPTA) and [IPTA, K))
    const bool both = IPTB > 0 && ta.nB > 0;
    double* ov = oval + (int64_t)p * q;
    int64_t* oi = oidx + (int64_t)p * q;
    CE_DASSERT(q >= 1 && q <= 64);

    const bool long_tile = both ? (hi - lo > (int64_t)BS * IPTA || ta.nB > (int64_t)BS * IPTB)
                                : hi - lo > (int64_t)BS * IPTA;
    CE_DASSERT(LONG || !long_tile);
    if (LONG && long_tile) {  // block-uniform: per-wave streams + tree merge
        tab.commit();
        RegTopQ tq;
        tq.init(q);
        int64_t wlo, whi;
        wave_part<W>(lo, hi, wlo, whi);
        stream_direct_range<SrcA, 2, UNRA>(srcA, wlo, whi, rel, q, tq, excl);
        if (both) {
            wave_part<W>(0, ta.nB, wlo, whi);
            if constexpr (IPTB > 0) stream_direct_range<SrcB, 2, UNRB>(srcB, wlo, whi, relB, q, tq, nullptr);
        }
        block_merge_write<W>(tq, sm.lists, q, nullptr, 0, ov, oi);
        return;
    } else {
        // 1. exact rows + approximate keys of this thread's items
        double mrow[K][C];
        uint32_t ak[K];
        bool sp[K];
        tile_rows<SrcA, IPTA, UNRA, BS, K, C, 0, true>(srcA, lo, hi, excl, tab, mrow, ak, sp);
        if constexpr (IPTB > 0)
            if (both) tile_rows<SrcB, IPTB, UNRB, BS, K, C, IPTA, false>(srcB, 0, ta.nB, nullptr, tab, mrow, ak, sp);
        CE_STAMP(blockIdx.x, 1)
        CE_WSTAMP(blockIdx.x)
        const uint32_t ntid = ~(uint32_t)tid;
        // position of local slot L (segment A's slots first, then segment B's)
        auto pos_of = [&](uint32_t L) -> int64_t {
            return L < (uint32_t)(IPTA * BS) ? lo + rel + (int64_t)L : (int64_t)(L - (uint32_t)(IPTA * BS)) + relB;
        };
#include "ce_small_finish.hpp"  // 2.-4. the floor, the survivors' append, the exact entropies and ranks
    }
}

// ---- the batched mix: two segments per block, U blocks ----------------------
// What block p of k_select_tiles_mix selects: segment A's items [lo, hi) of
// srcA (position = item + rel, bitmap exclA over the item index) and segment
// B's rows [loB, hiB) of srcB (position = row + relB, bitmap exclB over the
// row index).  Either range may be empty, either bitmap nullptr.
struct TileGeom {
    int64_t lo, hi, rel;
    int64_t loB, hiB, relB;
    const uint32_t* exclA;
    const uint32_t* exclB;
};

// The selection of one block over its TileGeom: steps 1-4 of the header
// comment, as k_select_tiles runs them, with segment B's range and bitmap per
// block.  Steps 2-4 are ONE text, ce_small_finish.hpp, expanded here and in
// k_select_tiles.  k_select_tiles does not call this function, and steps 2-4
// are not a function either: both changed the ISA of the existing
// instantiations, and configs[2] is pinned to that code
// (profiles/small_dedupe_codeobj.json).  `tab` has been fetched by the kernel;
// it is committed here.  A segment longer than its slots (BS * IPTA items,
// BS * IPTB rows) sends the block down the per-wave streaming path.
template <class SrcA, class SrcB, int IPTA, int IPTB, int UNRA, int UNRB, int BS>
__device__ __forceinline__ void select_tile(const SrcA& srcA, const SrcB& srcB, const TileGeom g, const int q,
                                            LogTablePrefetch& tab, TileSmem<BS / 64, SrcA::kC>& sm, double* ov,
                                            int64_t* oi) {
    constexpr int W = BS / 64, GS = BS / 64;  // waves; lanes per group (64 groups)
    constexpr int K = IPTA + IPTB;  // slots: segment A's, then segment B's (both segments in one block)
    static_assert(BS % 64 == 0 && BS >= 128 && GS <= 16 && (GS & (GS - 1)) == 0, "block size");
    constexpr int C = SrcA::kC;
    static_assert(IPTB > 0 && SrcB::kC == C, "both segments' rows have C classes");
    using SM = TileSmem<W, C>;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int64_t lo = g.lo, hi = g.hi, rel = g.rel, relB = g.relB;
    const uint32_t* excl = g.exclA;
    CE_DASSERT(q >= 1 && q <= 64);

    const bool long_tile = hi - lo > (int64_t)BS * IPTA || g.hiB - g.loB > (int64_t)BS * IPTB;
    if (long_tile) {  // block-uniform: per-wave streams over both segments + tree merge
        tab.commit();
        RegTopQ tq;
        tq.init(q);
        int64_t wlo, whi;
        wave_part<W>(lo, hi, wlo, whi);
        stream_direct_range<SrcA, 2, UNRA>(srcA, wlo, whi, rel, q, tq, excl);
        wave_part<W>(g.loB, g.hiB, wlo, whi);
        stream_direct_range<SrcB, 2, UNRB>(srcB, wlo, whi, relB, q, tq, g.exclB);
        block_merge_write<W>(tq, sm.lists, q, nullptr, 0, ov, oi);
        return;
    } else {
        // 1. exact rows + approximate keys of this thread's items
        double mrow[K][C];
        uint32_t ak[K];
        bool sp[K];
        tile_rows<SrcA, IPTA, UNRA, BS, K, C, 0, true, kSmallThrottle, 1>(srcA, lo, hi, excl, tab, mrow, ak, sp);
        // (an empty segment loads nothing and leaves its slots without an item)
        tile_rows<SrcB, IPTB, UNRB, BS, K, C, IPTA, false, kSmallThrottle, 1>(srcB, g.loB, g.hiB, g.exclB, tab, mrow,
                                                                              ak, sp);
        CE_STAMP(blockIdx.x, 1)
        CE_WSTAMP(blockIdx.x)
        const uint32_t ntid = ~(uint32_t)tid;
        // position of local slot L (segment A's slots first, then segment B's)
        auto pos_of = [&](uint32_t L) -> int64_t {
            return L < (uint32_t)(IPTA * BS) ? lo + rel + (int64_t)L
                                             : g.loB + (int64_t)(L - (uint32_t)(IPTA * BS)) + relB;
        };
#include "ce_small_finish.hpp"  // 2.-4. the floor, the survivors' append, the exact entropies and ranks
    }
}
#undef CE_SMALL_FINISH_FRAGMENT

// The batched mix (amg_test.py:473-480 for every user of :345's loop at once):
// block p selects user p's row stack [committee items offsets[p] ..
// offsets[p+1]; hc rows offsets_h[p] .. offsets_h[p+1]] over the rows whose
// bit is clear (excl over the global item index, excl_h over the global row
// index; either may be nullptr).  Positions are user-local: item i -> i,
// hc row j -> N_u + j.  Either segment may be empty; a user longer than the
// tile in either segment streams inside its block (per-wave lists + tree merge).
struct MixTileArgs {
    const int64_t* offsets;    // [U+1] committee items per user
    const int64_t* offsets_h;  // [U+1] hc rows per user
    const uint32_t* excl;
    const uint32_t* excl_h;
};

template <class SrcA, class SrcB, int IPTA, int IPTB, int UNRA, int UNRB, int BS>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(4))) void k_select_tiles_mix(
    SrcA srcA, SrcB srcB, MixTileArgs ta, int q, double* __restrict__ oval, int64_t* __restrict__ oidx) {
    __shared__ TileSmem<BS / 64, SrcA::kC> sm;
    CE_STAMP(blockIdx.x, 0)
    LogTablePrefetch tab;
    tab.fetch();
    const int p = blockIdx.x;
    const int64_t lo = ta.offsets[p], hi0 = ta.offsets[p + 1];
    const int64_t loB = ta.offsets_h[p], hiB0 = ta.offsets_h[p + 1];
    const int64_t hi = hi0 > lo ? hi0 : lo, hiB = hiB0 > loB ? hiB0 : loB;
    // A: position = item - lo; B: position = N_u + (row - loB)
    const TileGeom g{lo, hi, -lo, loB, hiB, (hi - lo) - loB, ta.excl, ta.excl_h};
    select_tile<SrcA, SrcB, IPTA, IPTB, UNRA, UNRB, BS>(srcA, srcB, g, q, tab, sm, oval + (int64_t)p * q,
                                                        oidx + (int64_t)p * q);
}

}  // namespace ce
