// ce_xgb_fit.hip -- C-ABI entries of the on-device XGBoost refit
// (ce_xgb_fit.hpp): the only TU that instantiates its kernels.  Three
// stream-ordered launches (the geometry's identity offsets, the start margins
// through the users walk, the fit); nothing allocated, read back or synchronised.
#include <algorithm>

#include "ce_abi.hpp"
#include "ce_xgb_fit.hpp"

using namespace ce;

extern "C" size_t ce_xgb_fit_workspace_bytes(int64_t R, int64_t n_max, int32_t D, int32_t G, int32_t rounds) {
    if (R <= 0 || n_max <= 0 || D < 1 || G < 1 || rounds < 1) return 0;
    return xgb_fit_ws(R, D, G).total;
}

template <class K>
static bool fit_lds(K kern, size_t lds) {
    if (lds <= 65536) return true;
    return hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}

extern "C" int ce_xgb_fit_users(const void* X, ce_dtype x_dt, int64_t F, int32_t D, int64_t ld, const int64_t* rows,
                                const int32_t* labels, const int64_t* row_offsets, int32_t U, int64_t R, int64_t n_max,
                                const uint32_t* table, int32_t TT, const int32_t* tree_ids, int64_t L,
                                const int32_t* group_offsets, int32_t G, int32_t depth, float base_margin,
                                int32_t rounds, int32_t max_depth, float eta, float lambda, float min_child_weight,
                                uint32_t* nodes_out, float* leaves_out, int32_t* left_out, int32_t* right_out,
                                int32_t* split_out, float* cond_out, uint8_t* default_left_out, int32_t* num_nodes_out,
                                float* margins_out, int32_t* status, void* workspace, size_t workspace_bytes,
                                ce_stream_t stream) {
    note_kernel("%s", "");
    if (F < 0 || D < 1 || ld < D || U < 1 || R < 0 || n_max < 0 || G < 1 || TT < 0 || L < 0 || depth < 0 || rounds < 1 ||
        max_depth < 1)
        return fail(CE_EINVAL, "bad XGB fit shapes F=%lld D=%d U=%d R=%lld n_max=%lld G=%d TT=%d L=%lld depth=%d rounds=%d "
                    "max_depth=%d", (long long)F, D, U, (long long)R, (long long)n_max, G, TT, (long long)L, depth, rounds,
                    max_depth);
    if (x_dt != CE_F32 && x_dt != CE_F64) return fail(CE_EINVAL, "XGB dtypes must be F32 or F64");
    if (!(eta > 0.0f) || !(eta < __builtin_inff()) || !(lambda >= 0.0f) || !(lambda < __builtin_inff()) ||
        !(min_child_weight >= 0.0f) || !(min_child_weight < __builtin_inff()))
        return fail(CE_EINVAL, "eta must be positive, lambda and min_child_weight non-negative, all finite (got %g, %g, %g)",
                    (double)eta, (double)lambda, (double)min_child_weight);
    if (G == 1) return fail(CE_EUNSUPPORTED, "the XGB fit grows multi:softprob forests only (binary:logistic has G = 1)");
    if (D > kXgbMaxFeat || G > kXgbMaxGroups || max_depth > kXgbFitMaxDepth || depth > kXgbLaneDepth)
        return fail(CE_EUNSUPPORTED, "the XGB fit takes D <= %d, G <= %d, max_depth <= %d (got D=%d G=%d max_depth=%d "
                    "depth=%d)", kXgbMaxFeat, kXgbMaxGroups, kXgbFitMaxDepth, D, G, max_depth, depth);
    if (n_max > kXgbFitMaxRows)
        return fail(CE_EUNSUPPORTED, "the XGB fit takes at most %d rows per user (n_max=%lld)", kXgbFitMaxRows,
                    (long long)n_max);
    if (depth < max_depth)
        return fail(CE_EINVAL, "the stack's depth %d is below max_depth %d: pack it at max_depth first", depth, max_depth);
    if (n_max > R) return fail(CE_EINVAL, "n_max=%lld above the %lld rows in all", (long long)n_max, (long long)R);
    if (!row_offsets || !group_offsets || !status) return fail(CE_EINVAL, "null offsets or status");
    if (R == 0) return CE_OK;  // every batch is empty: no new tree
    if (n_max < 1) return fail(CE_EINVAL, "n_max=0 with %lld rows", (long long)R);
    if (F == 0 || !X || !rows || !labels) return fail(CE_EINVAL, "rows without frames, or a null pointer");
    if (L > 0 && (!table || !tree_ids || TT < 1)) return fail(CE_EINVAL, "null table or tree_ids (L=%lld, TT=%d)", (long long)L, TT);
    if (!nodes_out || !leaves_out || !left_out || !right_out || !split_out || !cond_out || !default_left_out ||
        !num_nodes_out)
        return fail(CE_EINVAL, "null output");
    const XgbFitWs ws = xgb_fit_ws(R, D, G);
    if (!workspace || ((uintptr_t)workspace & 15)) return fail(CE_EINVAL, "workspace must be 16-byte aligned");
    if (workspace_bytes < ws.total)
        return fail(CE_EWORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes, ws.total);
    const int NT = xgb_fit_threads(D), nr = xgb_fit_rows_pad(n_max);
    const size_t lds = xgb_fit_lds_bytes(NT, nr);
    if (lds > 160 * 1024) return fail(CE_EUNSUPPORTED, "the XGB fit needs %zu bytes of LDS", lds);
    char* wb = static_cast<char*>(workspace);
    int64_t* ident = reinterpret_cast<int64_t*>(wb + ws.ident);
    float* m0 = reinterpret_cast<float*>(wb + ws.m0);

    // the start margins: the users walk over the batch (user u's songs: its rows, one frame each)
    hipLaunchKernelGGL(k_xgb_fit_ident, dim3((unsigned)((R + 256) / 256)), dim3(256), 0, (hipStream_t)stream, ident, R);
    const int S = xgb_users_splits(G);
    const XgbArgs xa{X, F, D, ld, G, G, S, base_margin, nullptr, 0};
    const UsersGeom ug{row_offsets, ident, rows, nullptr, U};
    const uint2* tb = reinterpret_cast<const uint2*>(table);
    with_kf(D, [&](auto kf) {
        constexpr int KF = decltype(kf)::value;
        if (x_dt == CE_F64)
            xgb_users_launch(k_xgb_fit_margins<CE_F64, KF>, R, D, G, S, stream, xa, ug, m0, tb, tree_ids, group_offsets, TT,
                             depth, L);
        else
            xgb_users_launch(k_xgb_fit_margins<CE_F32, KF>, R, D, G, S, stream, xa, ug, m0, tb, tree_ids, group_offsets, TT,
                             depth, L);
    });
    if (int rc = check_launch("ce_xgb_fit_users (start margins)")) return rc;

    const XgbFitArgs a{X, F, D, ld, rows, labels, row_offsets, G, rounds, max_depth, depth, nr, eta, lambda,
                       min_child_weight, nodes_out, leaves_out, left_out, right_out, split_out, cond_out,
                       default_left_out, num_nodes_out, margins_out, status, m0, reinterpret_cast<float*>(wb + ws.m1),
                       reinterpret_cast<float*>(wb + ws.sval), reinterpret_cast<uint16_t*>(wb + ws.sidx), ws.Dp};
    bool ok = true;
    auto fit = [&](auto kern, int xd) {
        note_kernel("ce::k_xgb_fit<%d>", xd);
        ok = fit_lds(kern, lds);
        if (ok) hipLaunchKernelGGL(kern, dim3(U), dim3(NT), lds, (hipStream_t)stream, a);
    };
    x_dt == CE_F64 ? fit(k_xgb_fit<CE_F64>, CE_F64) : fit(k_xgb_fit<CE_F32>, CE_F32);
    if (!ok) return fail(CE_ELAUNCH, "ce_xgb_fit_users: no %zu bytes of LDS for the fit", lds);
    return check_launch("ce_xgb_fit_users");
}
