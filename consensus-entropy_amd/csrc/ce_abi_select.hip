// ce_abi_select.hip -- C-ABI (include/ce.h): the fused mc selection (streaming
// stage 1 + merge, single-block small pools), exclusion-bitmap selection, the
// multi-GPU exchange records and chunked pools larger than HBM.
//
// q (any q >= 0, as the reference's -q, amg_test.py:547-553): q <= 64 runs on
// the streaming / single-block kernels (one launch), 64 < q <= CE_MAX_Q on the
// block-synchronous lists (k_partial) + a list merge, q > CE_MAX_Q on the sort
// path (ce_sort.hpp); q = 0 selects nothing.
//
// Every mc entry point (ce_select_mc, _excl, _cands, _partial, _chunk) is the one
// ladder below (mc_check + mc_run) over a sink saying what the call writes; the
// entry points differ in their own argument checks, their layout and their sink.
#include "ce_host.hpp"

using namespace ce;

// ---- the mc ladder -----------------------------------------------------------
extern "C" size_t ce_select_mc_workspace_bytes(int64_t N, int32_t q) { return ws_mc(N, q).bytes; }
extern "C" size_t ce_excl_words(int64_t N) { return N > 0 ? (size_t)((N + 31) / 32) : 0; }
static_assert(sizeof(ce_cand) == sizeof(Cand) && alignof(ce_cand) <= alignof(Cand), "ce_cand must mirror Cand");

// What one run of the ladder writes.
struct McSink {
    enum Out {
        kLists,    // stage 1's lists in the workspace, nothing else (ce_select_mc_partial)
        kFinal,    // the final (oval, oidx): the only sink the single-block kernels serve
        kRecords,  // q candidate records at ocand
    } out;
    double* oval;
    int64_t* oidx;
    Cand* ocand;
    const Cand* running;   // kRecords: a chunked job's running list to merge in, or nullptr
    const uint32_t* excl;  // exclusion bitmap over the pool, or nullptr
};

// the checks every mc entry point shares, in the order the ABI answers them
static int mc_check(const CommArgs& a, int q, const McSink& k, const WsLayout& L, const void* ws, size_t ws_bytes) {
    int rc = check_comm(a);
    if (rc) return rc;
    rc = check_q(q);
    if (rc) return rc;
    if (q > 0 && k.out == McSink::kFinal && (!k.oval || !k.oidx)) return fail(CE_EINVAL, "null output");
    if (q > 0 && k.out == McSink::kRecords && (!k.ocand || (uintptr_t)k.ocand % 16))
        return fail(CE_EINVAL, "ce_cand output must be 16-byte aligned device memory");
    // the workspace contract holds on every path, even the one that does not touch it
    return check_ws(L, ws, ws_bytes);
}

// The launches of a checked selection with q >= 1, best path first: the sort
// path (q > CE_MAX_Q), the single-block kernels, the streaming stage 1 (q <= 64)
// with the merge folded into its last block, else stage 1 (streaming without
// the fold, or block-synchronous) + one merge of the lists.
static int mc_run(const CommArgs& a, int q, int64_t base_idx, const McSink& k, const WsLayout& L, void* ws,
                  hipStream_t st) {
    if (q > CE_MAX_Q) {
        SortWs s;
        const int rc = sort_entropies(L, ws, a, nullptr, s, st);
        if (rc) return rc;
        sort_select(s, s.ent, a.N, base_idx, k.excl, q, k.oval, k.oidx, k.ocand, st);
        return CE_OK;
    }
    const int G = pool_blocks(a.N);
    const WsLists w = lists_view(L, ws);
    const bool final_out = k.out == McSink::kFinal;
    if (final_out && q <= kStreamMaxQ && a.N > 0) {
        // the pool in one block (k_select_tiles)
        if (launch_small_pool(a, base_idx, q, k.oval, k.oidx, k.excl, w, st)) return CE_OK;
        if (a.N * (int64_t)a.M * a.C * elem_bytes(a.dt) <= kSmallPoolBytes) {
            // small pool: ~512 items per 4-wave block on a few CUs (one block: it
            // is the final answer), then one wave merges the blocks' lists
            const int nb = (int)std::min<int64_t>(std::min<int64_t>(cdiv(a.N, 512), 32), G);
            if (launch_seg(a, nullptr, a.N, base_idx, q, nb, nb, 256, k.oval, k.oidx, w.c, k.excl, st)) {
                if (nb > 1) launch_merge_wave(w.c, 1, nb, q, k.oval, k.oidx, st);
                return CE_OK;
            }
        }
    }
    // the streaming stage 1 (it answers kNone for q > 64 or an empty pool); with
    // an output, stage 2 folded into its last block: one launch for the selection
    const Stage1 s1 = k.out == McSink::kLists
                          ? (launch_stream(a, G, q, base_idx, w, st, k.excl) ? Stage1::kLists : Stage1::kNone)
                          : launch_stream_fold(a, G, q, base_idx, w, st, k.excl,
                                               FoldOut{k.oval, k.oidx, k.ocand, k.running, ws_ptr<void>(ws, L.seed)});
    if (s1 == Stage1::kFolded) return CE_OK;
    // not folded: the running list joins the block lists as one more list
    if (k.running && hipMemcpyAsync(ws_ptr<Cand>(ws, L.running), k.running, (size_t)q * sizeof(Cand),
                                    hipMemcpyDeviceToDevice, st) != hipSuccess)
        return fail(CE_ELAUNCH, "running-list copy failed");
    bool done = k.out == McSink::kLists;
    if (s1 == Stage1::kNone) {  // the block-synchronous stage 1 (one block writes the final outputs itself)
        const Seg sg{nullptr, a.N, G, base_idx, k.excl};
        const bool fin = final_out && G == 1;
        const int rc = committee_partial(a, sg, G, q, w, k.oval, k.oidx, fin, st);
        if (rc) return dispatch_err(rc, a);
        done = done || fin;
    }
    if (!done) launch_finish_lists(w.c, 1, G + (k.running ? 1 : 0), q, k.oval, k.oidx, st, k.ocand);
    return CE_OK;
}

static int select_mc_ladder(const char* what, const CommArgs& a, int q, int64_t base_idx, const McSink& k,
                            const WsLayout& L, void* ws, size_t ws_bytes, hipStream_t st) {
    int rc = mc_check(a, q, k, L, ws, ws_bytes);
    if (rc || q == 0) return rc;
    rc = mc_run(a, q, base_idx, k, L, ws, st);
    return rc ? rc : check_launch(what);
}

extern "C" int ce_select_mc(const void* p, ce_dtype dt, int64_t N, int32_t M, int32_t C, int64_t sN, int64_t sM,
                            int64_t sC, int32_t q, int64_t base_idx, void* ws, size_t ws_bytes, double* val_out,
                            int64_t* idx_out, ce_stream_t stream) {
    return select_mc_ladder("ce_select_mc", CommArgs{p, (int)dt, N, M, C, sN, sM, sC}, q, base_idx,
                            McSink{McSink::kFinal, val_out, idx_out, nullptr, nullptr, nullptr}, ws_mc(N, q), ws,
                            ws_bytes, enter(stream));
}

extern "C" int ce_select_mc_excl(const void* p, ce_dtype dt, int64_t N, int32_t M, int32_t C, int64_t sN,
                                 int64_t sM, int64_t sC, const uint32_t* excl, int32_t q, int64_t base_idx, void* ws,
                                 size_t ws_bytes, double* val_out, int64_t* idx_out, ce_stream_t stream) {
    if (!excl && N > 0) return fail(CE_EINVAL, "null exclusion bitmap");
    return select_mc_ladder("ce_select_mc", CommArgs{p, (int)dt, N, M, C, sN, sM, sC}, q, base_idx,
                            McSink{McSink::kFinal, val_out, idx_out, nullptr, nullptr, excl}, ws_mc(N, q), ws, ws_bytes,
                            enter(stream));
}

// ce_select_mc writing the pool's q candidate records (the multi-GPU send
// buffer): for q <= 64 in ONE launch (stage 2 folded into stage 1's last block).
extern "C" int ce_select_mc_cands(const void* p, ce_dtype dt, int64_t N, int32_t M, int32_t C, int64_t sN, int64_t sM,
                                  int64_t sC, int32_t q, int64_t base_idx, void* ws, size_t ws_bytes, ce_cand* out,
                                  ce_stream_t stream) {
    return select_mc_ladder("ce_select_mc_cands", CommArgs{p, (int)dt, N, M, C, sN, sM, sC}, q, base_idx,
                            McSink{McSink::kRecords, nullptr, nullptr, reinterpret_cast<Cand*>(out), nullptr, nullptr},
                            ws_mc(N, q), ws, ws_bytes, enter(stream));
}

// The two stages as separate launches (q <= CE_MAX_Q), over the lists alone (ws_lists).
static int two_stage_q(int q, const char* whole) {
    return fail(CE_EUNSUPPORTED, "two-stage selection needs q <= %d (%s takes any q)", CE_MAX_Q, whole);
}

extern "C" int ce_select_mc_partial(const void* p, ce_dtype dt, int64_t N, int32_t M, int32_t C, int64_t sN,
                                    int64_t sM, int64_t sC, int32_t q, int64_t base_idx, void* ws,
                                    size_t ws_bytes, ce_stream_t stream) {
    const hipStream_t st = enter(stream);
    if (q > CE_MAX_Q) return two_stage_q(q, "ce_select_mc");
    if (q <= 0) return check_q(q);
    return select_mc_ladder("ce_select_mc_partial", CommArgs{p, (int)dt, N, M, C, sN, sM, sC}, q, base_idx,
                            McSink{McSink::kLists, nullptr, nullptr, nullptr, nullptr, nullptr}, ws_lists(N, q), ws,
                            ws_bytes, st);
}

// stage 2 of the two: the merge of the pool's lists into (val, idx) or records
static int finish_lists_of(const char* what, int64_t N, int q, void* ws, size_t ws_bytes, double* oval, int64_t* oidx,
                           Cand* ocand, hipStream_t st) {
    const WsLayout L = ws_lists(N, q);
    const int rc = check_ws(L, ws, ws_bytes);
    if (rc) return rc;
    launch_finish_lists(lists_view(L, ws).c, 1, pool_blocks(N), q, oval, oidx, st, ocand);
    return check_launch(what);
}

extern "C" int ce_select_finish(int64_t N, int32_t q, void* ws, size_t ws_bytes, double* val_out, int64_t* idx_out,
                                ce_stream_t stream) {
    const hipStream_t st = enter(stream);
    int rc = check_q(q);
    if (rc) return rc;
    if (q > CE_MAX_Q) return two_stage_q(q, "ce_select_mc");
    if (q == 0) return CE_OK;
    if (N < 0 || !val_out || !idx_out) return fail(CE_EINVAL, "bad finish arguments");
    return finish_lists_of("ce_select_finish", N, q, ws, ws_bytes, val_out, idx_out, nullptr, st);
}

// ---- exchange records (multi-GPU) -------------------------------------------
extern "C" int ce_select_finish_cands(int64_t N, int32_t q, void* ws, size_t ws_bytes, ce_cand* out,
                                      ce_stream_t stream) {
    const hipStream_t st = enter(stream);
    int rc = check_q(q);
    if (rc) return rc;
    if (q > CE_MAX_Q) return two_stage_q(q, "ce_select_mc_cands");
    if (q == 0) return CE_OK;
    if (N < 0 || !out) return fail(CE_EINVAL, "bad finish arguments");
    if ((uintptr_t)out % 16) return fail(CE_EINVAL, "ce_cand output must be 16-byte aligned");
    return finish_lists_of("ce_select_finish_cands", N, q, ws, ws_bytes, nullptr, nullptr, reinterpret_cast<Cand*>(out),
                           st);
}

extern "C" int ce_merge_cands(const ce_cand* c, int32_t nlists, int32_t q, double* val_out, int64_t* idx_out,
                              ce_stream_t stream) {
    const hipStream_t st = enter(stream);
    int rc = check_q(q);
    if (rc) return rc;
    if (q == 0) return CE_OK;
    if (nlists < 1 || !c || !val_out || !idx_out) return fail(CE_EINVAL, "bad merge arguments");
    if ((uintptr_t)c % 16) return fail(CE_EINVAL, "ce_cand input must be 16-byte aligned");
    const Cand* cc = reinterpret_cast<const Cand*>(c);
    if (q > CE_MAX_Q)  // no workspace here: the lists merge by rank (binary searches)
        rank_merge_lists(cc, nullptr, nullptr, nlists, q, val_out, idx_out, nullptr, st);
    else
        launch_finish_lists(cc, 1, nlists, q, val_out, idx_out, st);
    return check_launch("ce_merge_cands");
}

// ---- chunked pools (larger than HBM) ----------------------------------------
__global__ void k_cand_empty(Cand* __restrict__ c, int q) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < q; r += gridDim.x * blockDim.x) c[r] = Cand{0ull, -1};
}

extern "C" size_t ce_select_mc_chunk_workspace_bytes(int64_t N, int32_t q) { return ws_chunk(N, q).bytes; }

// The ladder over the chunk with the running list as its sink: stage 1 on the
// chunk (its G block lists), then ONE merge of those G lists plus the running
// list back into `running` -- folded into stage 1's last block for q <= 64,
// else over the running list copied to the layout's running slot.  The running
// list always holds the top-q of every chunk so far (the top-q of a union is
// within the union of the parts' top-qs).  q > CE_MAX_Q: the chunk's top-q by
// the sort path, merged with the running list by rank.
extern "C" int ce_select_mc_chunk(const void* p, ce_dtype dt, int64_t N, int32_t M, int32_t C, int64_t sN,
                                  int64_t sM, int64_t sC, int32_t q, int64_t base_idx, ce_cand* running,
                                  int32_t first, void* ws, size_t ws_bytes, ce_stream_t stream) {
    const hipStream_t st = enter(stream);
    int rc = check_q(q);
    if (rc) return rc;
    if (q == 0) return CE_OK;
    if (!running || (uintptr_t)running % 16)
        return fail(CE_EINVAL, "running list must be 16-byte aligned device memory");
    if (N < 0 || base_idx < 0)
        return fail(CE_EINVAL, "bad chunk N=%lld base_idx=%lld", (long long)N, (long long)base_idx);
    Cand* run = reinterpret_cast<Cand*>(running);
    if (N == 0) {
        if (first)
            hipLaunchKernelGGL(k_cand_empty, dim3((unsigned)std::min<int64_t>(cdiv(q, 256), 4096)), dim3(256), 0, st,
                               run, q);
        return check_launch("ce_select_mc_chunk");
    }
    const WsLayout L = ws_chunk(N, q);
    rc = check_ws(L, ws, ws_bytes);  // (this entry point answers for its workspace before its committee)
    if (rc) return rc;
    const CommArgs a{p, (int)dt, N, M, C, sN, sM, sC};
    if (q <= CE_MAX_Q)
        return select_mc_ladder("ce_select_mc_chunk", a, q, base_idx,
                                McSink{McSink::kRecords, nullptr, nullptr, run, first ? nullptr : run, nullptr}, L, ws,
                                ws_bytes, st);
    // the chunk's top-q into the layout's extra records, then (unless first) a copy of the running list behind it
    Cand* mine = ws_ptr<Cand>(ws, L.extra_slot(0, q));
    const McSink k{McSink::kRecords, nullptr, nullptr, first ? run : mine, nullptr, nullptr};
    rc = mc_check(a, q, k, L, ws, ws_bytes);
    if (!rc) rc = mc_run(a, q, base_idx, k, L, ws, st);
    if (rc) return rc;
    if (!first) {
        if (hipMemcpyAsync(ws_ptr<Cand>(ws, L.extra_slot(1, q)), run, (size_t)q * sizeof(Cand), hipMemcpyDeviceToDevice,
                           st) != hipSuccess)
            return fail(CE_ELAUNCH, "running-list copy failed");
        rank_merge_lists(mine, nullptr, nullptr, 2, q, nullptr, nullptr, run, st);
    }
    return check_launch("ce_select_mc_chunk");
}
