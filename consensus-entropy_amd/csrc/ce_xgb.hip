// ce_xgb.hip -- C-ABI entries of the XGBoost member (ce_xgb_walk.hpp over
// ce_xgb.hpp): host checks, dispatch and launches; the only TU that
// instantiates its kernels.
#include <algorithm>

#include "ce_abi.hpp"
#include "ce_xgb_table.hpp"
#include "ce_xgb_walk.hpp"

using namespace ce;

extern "C" size_t ce_xgb_lds_bytes(int32_t D, int32_t G) {
    return (size_t)D * kXgbCol * sizeof(float) + (size_t)std::max(G, 1) * 64 * sizeof(float) + 16 * sizeof(uint32_t);
}

// waves per group: fill a 16-wave block
static int xgb_splits(int G) { return std::max(1, 16 / G); }

template <class LaunchFn>
static void xgb_dispatch(ce_dtype x_dt, ce_dtype out_dt, LaunchFn&& fn) {
    if (x_dt == CE_F64)
        out_dt == CE_F64 ? fn(std::integral_constant<int, CE_F64>(), std::integral_constant<int, CE_F64>())
                         : fn(std::integral_constant<int, CE_F64>(), std::integral_constant<int, CE_F32>());
    else
        out_dt == CE_F64 ? fn(std::integral_constant<int, CE_F32>(), std::integral_constant<int, CE_F64>())
                         : fn(std::integral_constant<int, CE_F32>(), std::integral_constant<int, CE_F32>());
}

static int xgb_check(const void* X, ce_dtype x_dt, int64_t F, int32_t D, int64_t ld, int32_t G, int32_t C,
                     const void* out, ce_dtype out_dt, int64_t ld_out) {
    if (F < 0 || D < 1 || D > kXgbMaxFeat || ld < D || G < 1 || G > kXgbMaxGroups || ld_out < C ||
        !(G == C || (G == 1 && C == 2)))
        return fail(CE_EINVAL, "bad XGB shapes F=%lld D=%d G=%d C=%d", (long long)F, D, G, C);
    if ((x_dt != CE_F32 && x_dt != CE_F64) || (out_dt != CE_F32 && out_dt != CE_F64))
        return fail(CE_EINVAL, "XGB dtypes must be F32 or F64");
    if (F > 0 && (!X || !out)) return fail(CE_EINVAL, "null pointer");
    return CE_OK;
}

template <class K, class... Args>
static void xgb_launch(K kern, int64_t F, size_t lds, int threads, ce_stream_t stream, Args... args) {
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)((F + kXgbTile - 1) / kXgbTile)), dim3(threads), lds,
                       (hipStream_t)stream, args...);
}

extern "C" int ce_xgb_predict_proba(const void* X, ce_dtype x_dt, int64_t F, int32_t D, int64_t ld,
                                    const uint32_t* nodes, const float* leaves, const int32_t* group_offsets,
                                    int32_t G, int32_t depth, float base_margin, int32_t C, void* out,
                                    ce_dtype out_dt, int64_t ld_out, ce_stream_t stream) {
    if (int rc = xgb_check(X, x_dt, F, D, ld, G, C, out, out_dt, ld_out)) return rc;
    if (depth < 0 || depth > kXgbMaxDepth) return fail(CE_EINVAL, "XGB depth %d outside [0, %d]", depth, kXgbMaxDepth);
    if (!nodes || !leaves || !group_offsets) return fail(CE_EINVAL, "null pointer");
    if (F == 0) return CE_OK;
    const int S = xgb_splits(G);
    const XgbArgs a{X, F, D, ld, G, C, S, base_margin, out, ld_out};
    xgb_dispatch(x_dt, out_dt, [&](auto xd, auto od) {
        constexpr int XD = decltype(xd)::value, OD = decltype(od)::value;
        const auto kern = depth <= kXgbLaneDepth ? k_xgb_walk<XD, OD, true> : k_xgb_walk<XD, OD, false>;
        xgb_launch(kern, F, ce_xgb_lds_bytes(D, G), 64 * G * S, stream, a, reinterpret_cast<const uint2*>(nodes),
                   leaves, group_offsets, depth);
    });
    return check_launch("ce_xgb_predict_proba");
}

extern "C" int ce_xgb_lane_table(const uint32_t* nodes, const float* leaves, int32_t T, int32_t depth, int32_t D,
                                 uint32_t* table, ce_stream_t stream) {
    if (T < 0 || depth < 0 || depth > kXgbLaneDepth || D < 1 || D > kXgbMaxFeat)
        return fail(CE_EINVAL, "lane tables: T=%d depth=%d (<= %d) D=%d", T, depth, kXgbLaneDepth, D);
    if (T == 0) return CE_OK;
    if (!nodes || !leaves || !table) return fail(CE_EINVAL, "null pointer");
    hipLaunchKernelGGL(k_xgb_lane_table, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint2*>(nodes), leaves, T, depth, D, reinterpret_cast<uint2*>(table));
    return check_launch("ce_xgb_lane_table");
}

extern "C" int ce_xgb_predict_proba_lanes(const void* X, ce_dtype x_dt, int64_t F, int32_t D, int64_t ld,
                                          const uint32_t* table, int32_t T, const int32_t* group_offsets, int32_t G,
                                          int32_t depth, float base_margin, int32_t C, void* out, ce_dtype out_dt,
                                          int64_t ld_out, ce_stream_t stream) {
    if (int rc = xgb_check(X, x_dt, F, D, ld, G, C, out, out_dt, ld_out)) return rc;
    if (depth < 0 || depth > kXgbLaneDepth)
        return fail(CE_EINVAL, "XGB lane tables hold depth <= %d, got %d", kXgbLaneDepth, depth);
    if (!table || !group_offsets || T < 1) return fail(CE_EINVAL, "null pointer or no trees (T=%d)", T);
    if (F == 0) return CE_OK;
    const int S = xgb_splits(G);
    const uint2* tb = reinterpret_cast<const uint2*>(table);
    const XgbArgs a{X, F, D, ld, G, C, S, base_margin, out, ld_out};
    xgb_dispatch(x_dt, out_dt, [&](auto xd, auto od) {
        constexpr int XD = decltype(xd)::value, OD = decltype(od)::value;
        const auto kern = D <= 128 ? k_xgb_lanes<XD, OD, 2>
                        : D <= 256 ? k_xgb_lanes<XD, OD, 4>
                        : D <= 320 ? k_xgb_lanes<XD, OD, 5> : k_xgb_lanes<XD, OD, 8>;
        xgb_launch(kern, F, ce_xgb_lds_bytes(D, G), 64 * G * S, stream, a, tb, tb + (int64_t)T * 64, group_offsets,
                   depth);
    });
    return check_launch("ce_xgb_predict_proba_lanes");
}

extern "C" int ce_xgb_expf(const float* x, int64_t n, float* y, ce_stream_t stream) {
    if (n < 0 || (n > 0 && (!x || !y))) return fail(CE_EINVAL, "bad expf arguments");
    if (n == 0) return CE_OK;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(k_expf, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, y);
    return check_launch("ce_xgb_expf");
}
