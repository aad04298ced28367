// ce_ws.hpp -- the one workspace layout of the C-ABI (include/ce.h).  Plain
// C++17: no HIP, no device types (csrc/ce_ws_sanitize.cpp compiles it alone
// under ASan + UBSan and checks every layout over a grid of sizes).
//
// Every entry point computes ONE WsLayout from its size arguments (ws_topq,
// ws_mc, ws_lists, ws_chunk, ws_mix, ws_batched, ws_batched_mix, ws_frames).  Its `bytes` is
// what the matching ce_*_workspace_bytes returns and what the entry point
// checks the caller's workspace against; its regions are the only way to reach
// workspace memory (ws_ptr, ce_host.hpp), as offsets from the 256-aligned base
// (ws_base).  `bytes` covers every region from any base: it includes the up to
// 255 bytes the alignment of the base skips.
//
// A layout starts with the header of kWsCounters u32 arrival counters (the
// tiled kernels' tickets, one per problem; zero at rest: the caller zero-fills
// the workspace once, every call leaves the counters zero).  The header is the
// same for every entry point, so one workspace can serve any sequence of calls.
// q <= CE_MAX_Q: candidate lists of q 16-byte records follow; q > CE_MAX_Q:
// the sort path's buffers (ce_sort.hpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ce.h"

namespace ce {

constexpr int kMinItemsPerBlock = 64;
constexpr int kMaxBlocks = 1024;        // stage-1 blocks per pool (4 per CU on 256 CUs)
constexpr int kStreamMaxQ = 64;         // the streaming kernels' q: one list slot per lane
constexpr int kWideVoteSamples = 4096;  // the wide stream's floor samples (ce_wide_stream.hpp)
constexpr size_t kCandBytes = 16;       // one candidate record (Cand, ce_topq.hpp)
constexpr int kSortMaxWaves = 4096;
constexpr int64_t kSortMinChunk = 1024;  // items per wave at least (16 steps)

constexpr int kWsCounters = 16384;
constexpr size_t kWsHeader = (size_t)kWsCounters * sizeof(uint32_t);  // 64 KiB
// Who uses which word.  Word 0 is the arrival ticket of every folded launch
// (fold_merge: the streaming, wide and frames kernels; launches that share a
// workspace run one after another on one stream).  The LAST word is the
// streaming kernel's tile-claim word (k_stream_nmc, ce_stream.hpp): waves add to
// it while they stream and the launch's last block stores it back to zero.  It
// is never a ticket: a new ticket user takes a word below kWsClaimSlot, and a
// new claim-like word takes a slot of its own, a cache line (32 words) away
// from every other one.
constexpr int kWsClaimSlot = kWsCounters - 1;

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline uintptr_t ws_base(const void* ws) { return ((uintptr_t)ws + 255) & ~(uintptr_t)255; }

// stage-1 blocks for a pool of n items (host arithmetic only: ws sizing and
// launches agree by construction)
static inline int pool_blocks(int64_t n) {
    // one 64-item tile per wave at least; up to 1024 blocks (4 per CU), so wide
    // items (tens of KB each) still fill the chip
    int64_t g = cdiv(n, (int64_t)kMinItemsPerBlock);
    if (g < 1) g = 1;
    if (g > kMaxBlocks) g = kMaxBlocks;
    return (int)g;
}

// blocks per user of the batched selection: ~1024 items per block (two
// iterations per wave of a 4-wave block), at most ~4096 blocks in all.
// Measured at 500 x 1608 items: 512 items/block 33.2 us, 1024 31.4 us, 2048
// (one block per user, no merge launch) 31.0 us; 256 45 us.
static inline int batched_bpu(int64_t total, int U) {
    if (U < 1) return 1;
    const int64_t avg = cdiv(total, U);
    int64_t bpu = cdiv(avg, (int64_t)1024);
    const int64_t cap = 4096 / U > 1 ? 4096 / U : 1;
    if (bpu > cap) bpu = cap;
    if (bpu < 1) bpu = 1;
    return (int)bpu;
}

// The wide stream's floor + grid vote scratch (k_wide_seed / k_wide_seed_pick):
// the vote word, the seed record, the samples' records and approximate
// entropies, at these offsets of a 256-aligned region of kWideSeedUsed bytes.
// kWideSeedBytes is what a layout's size grows by for it (alignment included).
constexpr size_t kWideSeedVote = 0, kWideSeedSeed = 16, kWideSeedSamp = 256;
constexpr size_t kWideSeedSapx = kWideSeedSamp + (size_t)kWideVoteSamples * kCandBytes;
constexpr size_t kWideSeedUsed = kWideSeedSapx + (size_t)kWideVoteSamples * sizeof(float);
constexpr size_t kWideSeedBytes = 256 + 256 + (size_t)kWideVoteSamples * (kCandBytes + sizeof(float)) + 256;

struct SortGeom {
    int64_t n;      // records
    int64_t chunk;  // records per wave (a multiple of 64)
    int nw;         // waves (= cdiv(n, chunk))
};

static inline SortGeom sort_geom(int64_t n) {
    SortGeom g;
    g.n = n;
    int64_t chunk = cdiv(n < 1 ? 1 : n, (int64_t)kSortMaxWaves);
    if (chunk < kSortMinChunk) chunk = kSortMinChunk;
    g.chunk = (chunk + 63) / 64 * 64;
    g.nw = (int)cdiv(n < 1 ? 1 : n, g.chunk);
    return g;
}

struct Region {
    size_t off = 0, bytes = 0;  // from the 256-aligned base; bytes == 0: the layout has no such region
    size_t end() const { return off + bytes; }
};

struct WsLayout {
    size_t bytes = 0;  // the workspace size this layout needs, from any base
    Region ctr;        // the arrival counters
    // ---- q <= CE_MAX_Q: lists of q records (q >= 1 here)
    int q = 0;
    Region lists;    // stage 1's block lists, list k at slot(k)
    Region seg2;     // the mix's second segment (the hc rows' lists), right behind `lists`
    Region running;  // the chunked job's running-list slot, right behind `lists`
    // (one merge reads lists + seg2, or lists + running, as ONE array of lists)
    Region seed;     // the wide-seed scratch (256-aligned)
    // ---- the entropies: the sort path's, or the frame selection's for 64 < q <= CE_MAX_Q
    Region ent;
    // ---- q > CE_MAX_Q: the sort path (ce_sort.hpp)
    SortGeom g{0, 0, 0};
    Region a, b;   // two buffers of n records
    Region hist;   // 256 digit counts per wave
    Region dtot;   // 256 digit totals
    Region extra;  // records the caller asked for (the chunked job: 2q)

    // list k of `lists` (+ seg2 / running); the k-th run of n records of `extra`
    Region slot(int64_t k) const { return Region{lists.off + (size_t)k * (size_t)q * kCandBytes, (size_t)q * kCandBytes}; }
    Region extra_slot(int64_t k, int64_t n) const {
        return Region{extra.off + (size_t)k * (size_t)n * kCandBytes, (size_t)n * kCandBytes};
    }
};

// the header + nlists lists of max(q, 1) records
static inline WsLayout ws_list_layout(int64_t nlists, int32_t q) {
    WsLayout L;
    L.q = q < 1 ? 1 : q;
    L.ctr = Region{0, kWsHeader};
    L.lists = Region{kWsHeader, (size_t)nlists * (size_t)L.q * kCandBytes};
    L.bytes = L.lists.end() + 256u;
    return L;
}

// the last `bytes` of the lists as a region of its own (lists + it stay one array)
static inline Region ws_split_lists(WsLayout& L, size_t bytes) {
    L.lists.bytes -= bytes;
    return Region{L.lists.end(), bytes};
}

// a 256-aligned region of `used` bytes behind the lists; the size grows by `charged` >= used + 256
static inline Region ws_behind_lists(WsLayout& L, size_t used, size_t charged) {
    const Region r{al256(L.bytes - 256u), used};
    L.bytes += charged;
    return r;
}

// The sort path: the header, then n entropies, two n-record buffers, the digit
// counts and totals, and `extra_cands` records.
static inline WsLayout ws_sort(int64_t n, int64_t extra_cands = 0) {
    if (n < 0) n = 0;
    WsLayout L;
    L.g = sort_geom(n);
    L.ctr = Region{0, kWsHeader};
    size_t p = kWsHeader;
    auto take = [&p](size_t b) {
        const Region r{p, b};
        p += al256(b);
        return r;
    };
    L.ent = take((size_t)n * 8);
    L.a = take((size_t)n * kCandBytes);
    L.b = take((size_t)n * kCandBytes);
    L.hist = take((size_t)256 * L.g.nw * 4);
    L.dtot = take(256 * 8);
    L.extra = take((size_t)(extra_cands > 0 ? extra_cands : 0) * kCandBytes);
    L.bytes = p + 256u;
    return L;
}

// ---- one layout per entry point ------------------------------------------------
// ce_select_mc_partial / ce_select_finish / ce_select_finish_cands (q <= CE_MAX_Q): the lists alone
static inline WsLayout ws_lists(int64_t N, int32_t q) { return ws_list_layout(pool_blocks(N), q); }

// ce_topq: the pool's lists + the wide-seed scratch (ce_select_mc's layout)
static inline WsLayout ws_topq(int64_t N, int32_t q) {
    if (q > CE_MAX_Q) return ws_sort(N);
    WsLayout L = ws_lists(N, q);
    L.seed = ws_behind_lists(L, kWideSeedUsed, kWideSeedBytes);
    return L;
}

// ce_select_mc / _excl / _cands
static inline WsLayout ws_mc(int64_t N, int32_t q) { return ws_topq(N, q); }

// ce_select_mc_chunk: the chunk's lists + the running-list slot; q > CE_MAX_Q:
// 2q extra records (the chunk's top-q and a copy of the running list)
static inline WsLayout ws_chunk(int64_t N, int32_t q) {
    if (q > CE_MAX_Q) return ws_sort(N, 2 * (int64_t)q);
    WsLayout L = ws_list_layout((int64_t)pool_blocks(N) + 1, q);
    L.running = ws_split_lists(L, (size_t)L.q * kCandBytes);
    L.seed = ws_behind_lists(L, kWideSeedUsed, kWideSeedBytes);
    return L;
}

// ce_select_mix: the committee's lists + the hc rows' lists (the size keeps
// kWideSeedBytes of room, so it covers ws_mc of the committee part)
static inline WsLayout ws_mix(int64_t N, int64_t N_h, int32_t q) {
    if (q > CE_MAX_Q) return ws_sort((N > 0 ? N : 0) + (N_h > 0 ? N_h : 0));
    WsLayout L = ws_list_layout((int64_t)pool_blocks(N) + pool_blocks(N_h), q);
    L.seg2 = ws_split_lists(L, (size_t)pool_blocks(N_h) * (size_t)L.q * kCandBytes);
    L.bytes += kWideSeedBytes;
    return L;
}

// ce_select_batched: batched_bpu lists per user
static inline WsLayout ws_batched(int64_t total_items, int32_t U, int32_t q) {
    if (U < 1) U = 1;
    if (q > CE_MAX_Q) return ws_sort(total_items);
    return ws_list_layout((int64_t)batched_bpu(total_items, U) * U, q);
}

// ce_select_batched_mix: per user, the committee's lists (as ws_batched) and
// then the hc rows' lists, one array of lists (it covers ws_batched of the
// committee part, so one workspace serves both calls of a session)
static inline WsLayout ws_batched_mix(int64_t total_items, int64_t total_h, int32_t U, int32_t q) {
    if (U < 1) U = 1;
    if (total_items < 0) total_items = 0;
    if (total_h < 0) total_h = 0;
    if (q > CE_MAX_Q) return ws_sort(total_items + total_h);
    const int64_t nh = (int64_t)batched_bpu(total_h, U) * U;
    WsLayout L = ws_list_layout((int64_t)batched_bpu(total_items, U) * U + nh, q);
    L.seg2 = ws_split_lists(L, (size_t)nh * (size_t)L.q * kCandBytes);
    return L;
}

// ce_select_frames: q <= 64 the streaming kernels' lists; 64 < q <= CE_MAX_Q
// also the N per-song entropies the lists are selected from
static inline WsLayout ws_frames(int64_t N, int32_t q) {
    if (q > CE_MAX_Q) return ws_sort(N);
    WsLayout L = ws_lists(N, q);
    if (q > kStreamMaxQ) {
        const size_t eb = (size_t)(N > 0 ? N : 0) * 8;
        L.ent = ws_behind_lists(L, eb, 256 + eb);
    }
    return L;
}

}  // namespace ce
