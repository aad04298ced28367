// ce_xgb_users.hip -- C-ABI entries of the users form of the XGBoost member
// (ce_xgb_users.hpp): the only TU that instantiates its kernels.
// ce_xgb_predict_proba_users: one launch; ce_xgb_score_users: one
// stream-ordered memset of cm (under capture: one memset node) and one launch.
// No workspace, nothing read back or synchronised: capturable.
#include <algorithm>

#include "ce_abi.hpp"
#include "ce_xgb_users.hpp"

using namespace ce;

// What the two entry points check alike.
static int xgb_users_check(const void* X, ce_dtype x_dt, int64_t F, int32_t D, int64_t ld, const uint32_t* table,
                           int32_t TT, const int32_t* tree_ids, int64_t L, const int32_t* group_offsets, int32_t G,
                           int32_t depth, int32_t C, int32_t U, const int64_t* item_offsets,
                           const int64_t* frame_offsets) {
    if (F < 0 || D < 1 || D > kXgbMaxFeat || ld < D || G < 1 || G > kXgbMaxGroups || !(G == C || (G == 1 && C == 2)) ||
        TT < 0 || L < 0 || depth < 0)
        return fail(CE_EINVAL, "bad XGB shapes F=%lld D=%d G=%d C=%d TT=%d L=%lld depth=%d", (long long)F, D, G, C, TT,
                    (long long)L, depth);
    if (x_dt != CE_F32 && x_dt != CE_F64) return fail(CE_EINVAL, "XGB dtypes must be F32 or F64");
    if (U < 1) return fail(CE_EINVAL, "U=%d users: at least one", U);
    if (!item_offsets || !frame_offsets || !group_offsets) return fail(CE_EINVAL, "null offsets");
    if (L > 0 && (!table || !tree_ids || TT < 1)) return fail(CE_EINVAL, "null table or tree_ids (L=%lld, TT=%d)", (long long)L, TT);
    if (F > 0 && !X) return fail(CE_EINVAL, "null pointer");
    if (depth > kXgbLaneDepth)
        return fail(CE_EUNSUPPORTED, "the users form holds lane tables of depth <= %d, got %d", kXgbLaneDepth, depth);
    return CE_OK;
}

extern "C" int ce_xgb_predict_proba_users(const void* X, ce_dtype x_dt, int64_t F, int32_t D, int64_t ld,
                                          const uint32_t* table, int32_t TT, const int32_t* tree_ids, int64_t L,
                                          const int32_t* group_offsets, int32_t G, int32_t depth, float base_margin,
                                          int32_t C, int32_t U, const int64_t* item_offsets,
                                          const int64_t* frame_offsets, const int64_t* frame_perm,
                                          const uint32_t* excl, void* out, ce_dtype out_dt, int64_t ld_out,
                                          ce_stream_t stream) {
    note_kernel("%s", "");
    if (int rc = xgb_users_check(X, x_dt, F, D, ld, table, TT, tree_ids, L, group_offsets, G, depth, C, U,
                                 item_offsets, frame_offsets))
        return rc;
    if (out_dt != CE_F32 && out_dt != CE_F64) return fail(CE_EINVAL, "XGB dtypes must be F32 or F64");
    if (ld_out < C) return fail(CE_EINVAL, "ld_out=%lld below the %d classes", (long long)ld_out, C);
    if (F > 0 && !out) return fail(CE_EINVAL, "null pointer");
    if (F == 0) return CE_OK;
    const int S = xgb_users_splits(G);
    const XgbArgs a{X, F, D, ld, G, C, S, base_margin, out, ld_out};
    const uint2* tb = reinterpret_cast<const uint2*>(table);
    const UsersGeom ug{item_offsets, frame_offsets, frame_perm, excl, U};
    with_kf(D, [&](auto kf) {
        constexpr int KF = decltype(kf)::value;
        auto go = [&](auto kern, int xd, int od) {
            note_kernel("ce::k_xgb_users<%d, %d, %d>", xd, od, KF);
            xgb_users_launch(kern, F, D, G, S, stream, a, ug, tb, tree_ids, group_offsets, TT, depth, L);
        };
        if (x_dt == CE_F64)
            out_dt == CE_F64 ? go(k_xgb_users<CE_F64, CE_F64, KF>, CE_F64, CE_F64)
                             : go(k_xgb_users<CE_F64, CE_F32, KF>, CE_F64, CE_F32);
        else
            out_dt == CE_F64 ? go(k_xgb_users<CE_F32, CE_F64, KF>, CE_F32, CE_F64)
                             : go(k_xgb_users<CE_F32, CE_F32, KF>, CE_F32, CE_F32);
    });
    return check_launch("ce_xgb_predict_proba_users");
}

extern "C" int ce_xgb_score_users(const void* X, ce_dtype x_dt, int64_t F, int32_t D, int64_t ld,
                                  const uint32_t* table, int32_t TT, const int32_t* tree_ids, int64_t L,
                                  const int32_t* group_offsets, int32_t G, int32_t depth, float base_margin,
                                  int32_t C, int32_t U, const int64_t* item_offsets, const int64_t* frame_offsets,
                                  const int64_t* frame_perm, const uint32_t* excl, const int32_t* y, int64_t* cm,
                                  int32_t* pred, float* proba, int64_t ld_proba, ce_stream_t stream) {
    note_kernel("%s", "");
    if (int rc = xgb_users_check(X, x_dt, F, D, ld, table, TT, tree_ids, L, group_offsets, G, depth, C, U,
                                 item_offsets, frame_offsets))
        return rc;
    if (!cm || (F > 0 && !y)) return fail(CE_EINVAL, "null y or cm");
    if (proba && ld_proba < C) return fail(CE_EINVAL, "ld_proba=%lld below the %d classes", (long long)ld_proba, C);
    const hipError_t e = hipMemsetAsync(cm, 0, (size_t)U * C * C * sizeof(int64_t), (hipStream_t)stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(CE_ELAUNCH, "ce_xgb_score_users: %s", hipGetErrorString(e));
    }
    if (F == 0) return CE_OK;
    const int S = xgb_users_splits(G);
    const XgbArgs a{X, F, D, ld, G, C, S, base_margin, nullptr, 0};
    const uint2* tb = reinterpret_cast<const uint2*>(table);
    const UsersGeom ug{item_offsets, frame_offsets, frame_perm, excl, U};
    const XgbScoreOut o{y, reinterpret_cast<unsigned long long*>(cm), pred, proba, ld_proba};
    with_kf(D, [&](auto kf) {
        constexpr int KF = decltype(kf)::value;
        note_kernel("ce::k_xgb_score_users<%d, %d>", (int)x_dt, KF);
        if (x_dt == CE_F64)
            xgb_users_launch(k_xgb_score_users<CE_F64, KF>, F, D, G, S, stream, a, ug, o, tb, tree_ids, group_offsets, TT,
                             depth, L);
        else
            xgb_users_launch(k_xgb_score_users<CE_F32, KF>, F, D, G, S, stream, a, ug, o, tb, tree_ids, group_offsets, TT,
                             depth, L);
    });
    return check_launch("ce_xgb_score_users");
}
