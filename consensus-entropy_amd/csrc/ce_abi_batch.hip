// ce_abi_batch.hip -- C-ABI (include/ce.h): the mix ([mc; hc] row stack) and
// batched users in one launch.
#include "ce_host.hpp"

using namespace ce;


// ---- fused mix ---------------------------------------------------------------
extern "C" size_t ce_select_mix_workspace_bytes(int64_t N, int64_t N_h, int32_t q) { return ws_mix(N, N_h, q).bytes; }

extern "C" int ce_select_mix(const void* p, ce_dtype dt, int64_t N, int32_t M, int32_t C, int64_t sN, int64_t sM,
                             int64_t sC, const double* hc, int64_t N_h, int64_t ld_hc, int32_t q, void* ws,
                             size_t ws_bytes, double* val_out, int64_t* idx_out, ce_stream_t stream) {
    const hipStream_t st = enter(stream);
    CommArgs a{p, (int)dt, N, M, C, sN, sM, sC};
    int rc = check_comm(a);
    if (rc) return rc;
    rc = check_q(q);
    if (rc) return rc;
    if (N_h < 0 || (N_h > 0 && (!hc || ld_hc < C)) || (q > 0 && (!val_out || !idx_out)))
        return fail(CE_EINVAL, "bad hc table / outputs");
    const WsLayout L = ws_mix(N, N_h, q);
    rc = check_ws(L, ws, ws_bytes);
    if (rc) return rc;
    if (q == 0) return CE_OK;
    const CommArgs t{hc, kF64, N_h, 1, C, ld_hc, C, 1};  // the hc table: a one-member f64 committee [N_h, 1, C]
    if (q > CE_MAX_Q) {  // entropies of [mc; hc] (positions 0..N-1, N..N+N_h-1), then the sort path
        SortWs s;
        rc = sort_entropies(L, ws, a, &t, s, st);
        if (rc) return rc;
        sort_select(s, s.ent, N + N_h, 0, nullptr, q, val_out, idx_out, nullptr, st);
        return check_launch("ce_select_mix");
    }
    const int G1 = pool_blocks(N), G2 = pool_blocks(N_h);
    const WsLists w = lists_view(L, ws);
    if (q <= kStreamMaxQ && N > 0 && N_h > 0 && N <= kSmallPoolItems && N_h <= kSmallPoolItems &&
        C == 4) {
        // both segments in ONE block (k_select_tiles)
        if (launch_small_mix(a, t, q, val_out, idx_out, st)) return check_launch("ce_select_mix");
    }
    // both segments on the streaming engine when it applies (q <= 64): the hc
    // table is a committee of M = 1 member ([N_h, 1, C] f64, row stride ld_hc)
    if (!launch_stream(a, G1, q, 0, w, st)) {
        Seg s1{nullptr, N, G1, 0};
        rc = committee_partial(a, s1, G1, q, w, nullptr, nullptr, false, st);
        if (rc) return dispatch_err(rc, a);
    }
    const WsLists w2{ws_ptr<Cand>(ws, L.seg2), w.ctr};
    if (!launch_stream(t, G2, q, N, w2, st)) {
        Seg s2{nullptr, N_h, G2, N};
        // no TableSrc<C> (C outside {2, 3, 4, 8}): the table as the one-member
        // committee it already is for q <= 64 and for the sort path -- the wide
        // kernels, same list layout
        rc = partial_table(hc, ld_hc, C, s2, G2, q, w2, st);
        if (rc == CE_EUNSUPPORTED) rc = committee_partial(t, s2, G2, q, w2, nullptr, nullptr, false, st);
        if (rc) return fail(CE_EUNSUPPORTED, "mix with C=%d has no kernel in this build", C);
    }
    launch_finish_lists(w.c, 1, G1 + G2, q, val_out, idx_out, st);  // lists + seg2: one array of G1 + G2 lists
    return check_launch("ce_select_mix");
}

// ---- batched users (batched_bpu lists per user: ws_batched, ce_ws.hpp) ---------
extern "C" size_t ce_select_batched_workspace_bytes(int64_t total_items, int32_t U, int32_t q) {
    return ws_batched(total_items, U, q).bytes;
}

// ce_select_batched and ce_select_batched_excl: one ladder (tiles, k_stream_seg,
// committee_partial, sort), the bitmap handed down every rung (nullptr: none)
static int select_batched(const char* fn, const void* p, ce_dtype dt, int64_t total_items, int32_t M, int32_t C,
                          int64_t sN, int64_t sM, int64_t sC, const int64_t* offsets, int32_t U,
                          const uint32_t* excl, int32_t q, void* ws, size_t ws_bytes, double* val_out,
                          int64_t* idx_out, ce_stream_t stream) {
    const hipStream_t st = enter(stream);
    CommArgs a{p, (int)dt, total_items, M, C, sN, sM, sC};
    int rc = check_comm(a);
    if (rc) return rc;
    rc = check_q(q);
    if (rc) return rc;
    if (U < 1 || !offsets || (q > 0 && (!val_out || !idx_out))) return fail(CE_EINVAL, "bad batched arguments");
    const WsLayout L = ws_batched(total_items, U, q);
    rc = check_ws(L, ws, ws_bytes);
    if (rc) return rc;
    if (q == 0) return CE_OK;
    if (q > CE_MAX_Q) {  // every user's items contiguous in the total order: sort by (user, key, position)
        if (U >= kSortMaxUsers) return fail(CE_EUNSUPPORTED, "q > %d needs U < %d users", CE_MAX_Q, kSortMaxUsers);
        // a record's position packs (user << kUserShift) | user-local position
        if (total_items >= (int64_t(1) << kUserShift))
            return fail(CE_EUNSUPPORTED, "q > %d needs fewer than 2^%d items in all", CE_MAX_Q, kUserShift);
        SortWs s;
        rc = sort_entropies(L, ws, a, nullptr, s, st);
        if (rc) return rc;
        sort_keys_users(s.ent, total_items, offsets, U, excl, s.a, st);
        sort_out_users(sort_run(s, user_sort_passes(U), st), offsets, U, q, val_out, idx_out, st);
        return check_launch(fn);
    }
    const int bpu = batched_bpu(total_items, U);
    const int64_t nl = (int64_t)bpu * U;
    const WsLists w = lists_view(L, ws);
    if (q <= kStreamMaxQ) {
        // one block per user (k_select_tiles; a user longer than its block streams inside it)
        if (launch_small_users(a, offsets, U, q, val_out, idx_out, excl, st)) return check_launch(fn);
    }
    if (q <= kStreamMaxQ) {
        // bpu 4-wave blocks per user, then one wave per user merges its bpu lists
        if (launch_seg(a, offsets, 0, 0, q, (int)nl, bpu, bpu == 1 && U < 64 ? 64 * kSegWaves : 256, val_out, idx_out,
                       w.c, excl, st)) {
            if (bpu > 1) launch_merge_wave(w.c, U, bpu, q, val_out, idx_out, st);
            return check_launch(fn);
        }
    }
    Seg sg{offsets, total_items, bpu, 0, excl};
    const bool fin = bpu == 1;
    rc = committee_partial(a, sg, (int)nl, q, w, val_out, idx_out, fin, st);
    if (rc) return dispatch_err(rc, a);
    if (!fin) launch_finish_lists(w.c, U, bpu, q, val_out, idx_out, st);
    return check_launch(fn);
}

extern "C" int ce_select_batched(const void* p, ce_dtype dt, int64_t total_items, int32_t M, int32_t C, int64_t sN,
                                 int64_t sM, int64_t sC, const int64_t* offsets, int32_t U, int32_t q, void* ws,
                                 size_t ws_bytes, double* val_out, int64_t* idx_out, ce_stream_t stream) {
    return select_batched("ce_select_batched", p, dt, total_items, M, C, sN, sM, sC, offsets, U, nullptr, q, ws,
                          ws_bytes, val_out, idx_out, stream);
}

extern "C" int ce_select_batched_excl(const void* p, ce_dtype dt, int64_t total_items, int32_t M, int32_t C,
                                      int64_t sN, int64_t sM, int64_t sC, const int64_t* offsets, int32_t U,
                                      const uint32_t* excl, int32_t q, void* ws, size_t ws_bytes, double* val_out,
                                      int64_t* idx_out, ce_stream_t stream) {
    return select_batched("ce_select_batched_excl", p, dt, total_items, M, C, sN, sM, sC, offsets, U, excl, q, ws,
                          ws_bytes, val_out, idx_out, stream);
}

// ---- batched mix (ws_batched_mix, ce_ws.hpp) -----------------------------------
extern "C" size_t ce_select_batched_mix_workspace_bytes(int64_t total_items, int64_t total_h, int32_t U, int32_t q) {
    return ws_batched_mix(total_items, total_h, U, q).bytes;
}

extern "C" int ce_select_batched_mix(const void* p, ce_dtype dt, int64_t total_items, int32_t M, int32_t C, int64_t sN,
                                     int64_t sM, int64_t sC, const int64_t* offsets, const double* hc, int64_t total_h,
                                     int64_t ld_hc, const int64_t* offsets_h, int32_t U, const uint32_t* excl,
                                     const uint32_t* excl_h, int32_t q, void* ws, size_t ws_bytes, double* val_out,
                                     int64_t* idx_out, ce_stream_t stream) {
    const hipStream_t st = enter(stream);
    CommArgs a{p, (int)dt, total_items, M, C, sN, sM, sC};
    int rc = check_comm(a);
    if (rc) return rc;
    rc = check_q(q);
    if (rc) return rc;
    if (U < 1 || !offsets || !offsets_h) return fail(CE_EINVAL, "bad batched arguments (U=%d, offsets, offsets_h)", U);
    if (total_h < 0 || (total_h > 0 && (!hc || ld_hc < C)))
        return fail(CE_EINVAL, "bad hc table (total_h=%lld, ld_hc=%lld < C=%d?)", (long long)total_h, (long long)ld_hc, C);
    if (q > 0 && (!val_out || !idx_out)) return fail(CE_EINVAL, "null outputs");
    if (q == 0) return CE_OK;
    if (C != 4 || q > kStreamMaxQ)
        return fail(CE_EUNSUPPORTED, "the batched mix runs C = 4 and q <= %d (got C=%d, q=%d): compose it from "
                    "ce_select_batched_excl over either part and ce_topq_merge", kStreamMaxQ, C, q);
    rc = check_ws(ws_batched_mix(total_items, total_h, U, q), ws, ws_bytes);
    if (rc) return rc;
    const CommArgs t{hc, kF64, total_h, 1, C, ld_hc, C, 1};  // the stacked tables: a one-member f64 committee
    if (!launch_small_mix_users(a, t, offsets, offsets_h, U, q, val_out, idx_out, excl, excl_h, st))
        return dispatch_err(CE_EUNSUPPORTED, a);
    return check_launch("ce_select_batched_mix");
}
