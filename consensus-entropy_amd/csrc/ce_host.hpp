// ce_host.hpp -- host side shared by the C-ABI translation units: argument
// checks, typed views of the workspace layout (ce_ws.hpp), the selection
// tails every entry point shares, and the declarations of the launchers
// (each defined in one ce_launch_*.hip).  No kernel template is visible from
// here: an entry point sees argument types and launchers only; what picks
// and launches kernels is in ce_dispatch.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "../../include/ce.h"
#include "ce_abi.hpp"
#include "ce_sort.hpp"
#include "ce_topq.hpp"  // Cand, Seg, the dtype codes
#include "ce_ws.hpp"

using namespace ce;

// ---- workspace views ---------------------------------------------------------
// ce_ws.hpp holds the layout (sizes and region offsets, one WsLayout per entry
// point); these put device types on its regions.  A region is reached only
// through the layout whose `bytes` the entry point checked (check_ws).
static_assert(sizeof(Cand) == kCandBytes, "ce_ws.hpp sizes the lists in Cand records");

template <class T>
static inline T* ws_ptr(void* ws, Region r) {
    return reinterpret_cast<T*>(ws_base(ws) + r.off);
}

static inline int check_ws(const WsLayout& L, const void* ws, size_t ws_bytes) {
    if (!ws || ws_bytes < L.bytes) return fail(CE_EWORKSPACE, "workspace too small");
    return CE_OK;
}

struct WsLists {
    Cand* c;        // candidate lists
    uint32_t* ctr;  // arrival counters (header)
};
static inline WsLists lists_view(const WsLayout& L, void* ws) {
    return WsLists{ws_ptr<Cand>(ws, L.lists), ws_ptr<uint32_t>(ws, L.ctr)};
}

static inline SortWs sort_view(const WsLayout& L, void* ws) {
    return SortWs{ws_ptr<double>(ws, L.ent),    ws_ptr<Cand>(ws, L.a),        ws_ptr<Cand>(ws, L.b),
                  ws_ptr<uint32_t>(ws, L.hist), ws_ptr<uint64_t>(ws, L.dtot), ws_ptr<Cand>(ws, L.extra), L.g};
}

// The wide stream's floor + grid vote scratch (a layout's `seed` region)
constexpr int64_t kWideSeedMinItems = 16 * 1024;  // >= 1024 samples (wide_nsamples: 1/16 of the items)
struct WideSeedWs {
    uint32_t* vote;
    Cand* seed;
    Cand* samp;   // [kWideVoteSamples]
    float* sapx;  // [kWideVoteSamples]
};
static inline WideSeedWs wide_seed_carve(void* seed_region) {
    const uintptr_t p = ws_base(seed_region);
    return WideSeedWs{reinterpret_cast<uint32_t*>(p + kWideSeedVote), reinterpret_cast<Cand*>(p + kWideSeedSeed),
                      reinterpret_cast<Cand*>(p + kWideSeedSamp), reinterpret_cast<float*>(p + kWideSeedSapx)};
}

// Every selection entry point starts here: ce_last_kernel() reads "" unless
// this call notes a kernel.
static inline hipStream_t enter(ce_stream_t stream) {
    note_kernel("%s", "");
    return (hipStream_t)stream;
}

// Any q >= 0, as the reference's -q (amg_test.py:547-553): argsort[::-1][:q]
// returns min(q, N) positions, none for q = 0.  q <= CE_MAX_Q runs on the list
// kernels; above it on the sort path (ce_sort.hpp, its workspace grows with N).
static inline int check_q(int q) {
    if (q < 0) return fail(CE_EINVAL, "q=%d is negative", q);
    return CE_OK;
}

// ---- committee arguments ---------------------------------------------------
struct CommArgs {
    const void* p;
    int dt;
    int64_t N;
    int M, C;
    int64_t sN, sM, sC;
};

static inline int check_comm(const CommArgs& a) {
    if (!a.p && a.N > 0) return fail(CE_EINVAL, "null committee pointer");
    if (a.N < 0 || a.M < 1 || a.C < 1) return fail(CE_EINVAL, "bad shape N=%lld M=%d C=%d", (long long)a.N, a.M, a.C);
    if (a.dt < 0 || a.dt > 2) return fail(CE_EINVAL, "bad dtype %d", a.dt);
    return CE_OK;
}

static inline int elem_bytes(int dt) { return dt == kF64 ? 8 : (dt == kF32 ? 4 : 2); }

static inline int dispatch_err(int rc, const CommArgs& a) {
    if (rc == CE_EUNSUPPORTED)
        return fail(CE_EUNSUPPORTED, "committee shape C=%d dtype=%d has no kernel in this build", a.C, a.dt);
    return rc;
}

// thresholds of the entry points' ladders (the kernels themselves: ce_launch_small.hip)
constexpr int64_t kSmallPoolBytes = 256 * 1024;  // below this one block does the whole selection
constexpr int kSegWaves = 16;     // waves per single-block pool / per user (k_stream_seg)

// ---------------------------------------------------------------------------
// Launchers.  Each is DEFINED in exactly one translation unit (named below),
// so every kernel instantiation lives in one code object of libce_amd.so;
// the entry points (ce_abi_*.hip) only call these.
// ---------------------------------------------------------------------------
// ce_launch_stream.hip: streaming stage 1 (q <= 64): k_stream_nmc (item-major
// LDS-DMA), k_stream_direct (any strides), k_stream_wide2 / k_stream_wide
// (wide classes).  Returns false (nothing launched) when no kernel applies.
CE_HIDDEN bool launch_stream(const CommArgs& a, int G, int q, int64_t base_idx, WsLists w, hipStream_t st,
                             const uint32_t* excl = nullptr);
// The same with stage 2 folded in: the grid's last block merges the block
// lists into the final (oval, oidx), or into q records at ocand (one launch
// for the whole selection).
enum class Stage1 {
    kNone = 0,    // no streaming kernel applies: nothing launched
    kLists = 1,   // launched WITHOUT the fold: the lists are in w, run a finish
    kFolded = 2,  // launched, outputs written
};
struct FoldOut {
    double* oval;
    int64_t* oidx;
    Cand* ocand;
    const Cand* extra;  // one more list to merge (a chunked job's running list), or nullptr
    void* wide_ws;      // the layout's seed region for the wide stream's floor + grid vote, or nullptr
};
CE_HIDDEN Stage1 launch_stream_fold(const CommArgs& a, int G, int q, int64_t base_idx, WsLists w, hipStream_t st,
                                    const uint32_t* excl, FoldOut out);
// ce_launch_partial.hip: block-synchronous stage 1 (any q): committee,
// precomputed entropies, an hc table.
CE_HIDDEN int committee_partial(const CommArgs& a, const Seg& sg, int grid, int q, WsLists w, double* oval,
                                int64_t* oidx, bool fin, hipStream_t st);
CE_HIDDEN void partial_entropies(const double* ent, const Seg& sg, int grid, int q, WsLists w, double* oval,
                                 int64_t* oidx, bool fin, hipStream_t st);
CE_HIDDEN int partial_table(const double* hc, int64_t ld, int C, const Seg& sg, int grid, int q, WsLists w,
                            hipStream_t st);
// ce_launch_finish.hip: stage 2 merges of candidate lists.
CE_HIDDEN void launch_finish_lists(const Cand* c, int segments, int nl, int q, double* oval, int64_t* oidx,
                                   hipStream_t st, Cand* ocand = nullptr);
CE_HIDDEN void launch_finish_vals(const double* vals, const int64_t* idx, int segments, int nl, int q,
                                  double* oval, int64_t* oidx, hipStream_t st);
CE_HIDDEN void launch_merge_wave(const Cand* c, int segs, int nl, int q, double* oval, int64_t* oidx,
                                 hipStream_t st);
// ce_launch_small.hip: pools of a few thousand items, one block per problem
// (k_select_tiles, ce_small.hpp).
// one pool of a.N items (<= kSmallPoolItems); false: too large / no kernel
constexpr int64_t kSmallPoolItems = 4096;
CE_HIDDEN bool launch_small_pool(const CommArgs& a, int64_t base_idx, int q, double* oval, int64_t* oidx,
                                 const uint32_t* excl, WsLists w, hipStream_t st);
// U users (offsets[U+1]) in one launch, one block per user (excl: over the tensor's items, or nullptr)
CE_HIDDEN bool launch_small_users(const CommArgs& a, const int64_t* offsets, int U, int q, double* oval,
                                  int64_t* oidx, const uint32_t* excl, hipStream_t st);
// the mix of U users in one launch (C = 4): user u's committee items offsets[u] .. and hc rows offsets_h[u] ..
CE_HIDDEN bool launch_small_mix_users(const CommArgs& a, const CommArgs& t, const int64_t* offsets,
                                      const int64_t* offsets_h, int U, int q, double* oval, int64_t* oidx,
                                      const uint32_t* excl, const uint32_t* excl_h, hipStream_t st);
// the mix of amg_test.py:473-480 ([mc; hc] rows, C = 4) in one launch
CE_HIDDEN bool launch_small_mix(const CommArgs& a, const CommArgs& t, int q, double* oval, int64_t* oidx,
                                hipStream_t st);
// k_stream_seg over `nblocks` blocks of `threads` (bpu blocks per segment)
CE_HIDDEN bool launch_seg(const CommArgs& a, const int64_t* offsets, int64_t n, int64_t base_idx, int q, int nblocks,
                          int bpu, int threads, double* oval, int64_t* oidx, Cand* wc, const uint32_t* excl,
                          hipStream_t st);

// ce_launch_sort.hip: the sort path for q > CE_MAX_Q (ce_sort.hpp; its workspace: ws_sort, ce_ws.hpp).
// records {order key (0 if excluded), idx0 + i} of ent[0..n) into out
CE_HIDDEN void sort_keys(const double* ent, int64_t n, int64_t idx0, const uint32_t* excl, Cand* out, hipStream_t st);
CE_HIDDEN void sort_keys_users(const double* ent, int64_t n, const int64_t* offsets, int U, const uint32_t* excl,
                               Cand* out, hipStream_t st);
// sorts s.a[0..s.g.n) (generated in ascending position) by key descending, then
// user_passes passes over the user bits; returns the buffer holding the result
CE_HIDDEN const Cand* sort_run(const SortWs& s, int user_passes, hipStream_t st);
CE_HIDDEN int user_sort_passes(int U);
// the first q slots of sorted records as (val, idx) or records (ocand)
CE_HIDDEN void sort_out(const Cand* s, int64_t n, int64_t q, double* oval, int64_t* oidx, Cand* ocand, hipStream_t st);
CE_HIDDEN void sort_out_users(const Cand* s, const int64_t* offsets, int U, int64_t q, double* oval, int64_t* oidx,
                              hipStream_t st);
// merge of nl best-first lists of q slots (records c, or (vals, idx)) by rank
CE_HIDDEN void rank_merge_lists(const Cand* c, const double* vals, const int64_t* idx, int nl, int64_t q, double* oval,
                                int64_t* oidx, Cand* ocand, hipStream_t st);
// ce_abi_core.hip: per-item committee entropy (and optional mean) to HBM, any supported shape
CE_HIDDEN int launch_entropy(const CommArgs& a, double* mean_or_null, double* ent, hipStream_t st);

// The sort path counts records per wave and per digit in 32 bits
// (ce_launch_sort.hip): it takes fewer than 2^32 records per call.
constexpr int64_t kSortMaxRecords = 0xFFFFFFFFll;
static inline int check_sort_n(int64_t n) {
    if (n > kSortMaxRecords)
        return fail(CE_EUNSUPPORTED, "q > %d sorts the pool: it takes < 2^32 items per call (got %lld)", CE_MAX_Q,
                    (long long)n);
    return CE_OK;
}

// entropies ent[0..n) -> the first q slots of the total order (sort path)
static inline void sort_select(const SortWs& s, const double* ent, int64_t n, int64_t idx0, const uint32_t* excl,
                               int64_t q, double* oval, int64_t* oidx, Cand* ocand, hipStream_t st) {
    sort_keys(ent, n, idx0, excl, s.a, st);
    sort_out(sort_run(s, 0, st), n, q, oval, oidx, ocand, st);
}

// q > CE_MAX_Q: the entropies of committee `a` (and then of `t`, the mix's hc
// rows) into the sort workspace, viewed in s
static inline int sort_entropies(const WsLayout& L, void* ws, const CommArgs& a, const CommArgs* t, SortWs& s,
                                 hipStream_t st) {
    int rc = check_sort_n(L.g.n);
    if (rc) return rc;
    s = sort_view(L, ws);
    rc = launch_entropy(a, nullptr, s.ent, st);
    if (!rc && t) rc = launch_entropy(*t, nullptr, s.ent + a.N, st);
    return rc;
}

// an entropy vector -> the top q: the block lists + a merge, or the sort path
// (the caller has run check_sort_n for q > CE_MAX_Q); excl: items whose bit
// is set are out (their ent is not read as a candidate), or nullptr
static inline void select_entropies(const WsLayout& L, void* ws, const double* ent, int64_t N, int q, int64_t base_idx,
                                    double* oval, int64_t* oidx, hipStream_t st, const uint32_t* excl = nullptr) {
    if (q > CE_MAX_Q) {
        sort_select(sort_view(L, ws), ent, N, base_idx, excl, q, oval, oidx, nullptr, st);
        return;
    }
    const int G = pool_blocks(N);
    const WsLists w = lists_view(L, ws);
    Seg sg{nullptr, N, G, base_idx, excl};
    partial_entropies(ent, sg, G, q, w, oval, oidx, G == 1, st);
    if (G > 1) launch_finish_lists(w.c, 1, G, q, oval, oidx, st);
}
