// ce_members_users.hip -- C-ABI entries of the users form of the linear
// members' predict_proba (ce_members_users.hpp): the only TU that instantiates
// its kernels.  One launch, no workspace, nothing synchronised: capturable.
#include "ce_dispatch.hpp"
#include "ce_members_users.hpp"

using namespace ce;

extern "C" int ce_gnb_predict_proba_users(const double* X, int64_t F, int32_t D, int64_t ld, const double* theta,
                                          const double* var, const double* log_prior, int32_t C, int32_t U,
                                          const int64_t* item_offsets, const int64_t* frame_offsets,
                                          const int64_t* frame_perm, const uint32_t* excl, double* out,
                                          int64_t ld_out, ce_stream_t stream) {
    if (F < 0 || D < 1 || D > kMaxFeat || ld < D || C < 1 || C > kMaxMemberC || ld_out < C)
        return fail(CE_EINVAL, "bad GaussianNB shapes F=%lld D=%d C=%d", (long long)F, D, C);
    int rc = check_users_geom(U, item_offsets, frame_offsets);
    if (rc) return rc;
    if ((F > 0 && (!X || !out)) || !theta || !var || !log_prior) return fail(CE_EINVAL, "null pointer");
    if (D < 8) return fail(CE_EUNSUPPORTED, "GaussianNB needs D >= 8 features (got %d)", D);  // as ce_gnb_predict_proba
    if (F == 0) return CE_OK;
    GnbArgs a{X, F, D, ld, theta, var, log_prior, C, out, ld_out};
    UsersGeom ug{item_offsets, frame_offsets, frame_perm, excl, U};
    const PwPlan pl = pw_plan(D);
    const size_t lds = (size_t)3 * C * D * sizeof(double);  // up to 96 KB at C = 8, D = 512
    if (D == 260 && ld == 260 && C == 4) {  // the reference's contiguous rows: feature-streamed, as ce_gnb_predict_proba
        auto kern = k_gnb_users260<4, 3>;
        hipLaunchKernelGGL(kern, dim3(users_grid(kern, 0, F)), dim3(256), 0, (hipStream_t)stream, a, ug);
        return check_launch("ce_gnb_predict_proba_users");
    }
    if (D == 260) {  // the reference's feature count: constant pairwise plan
        auto kern = k_gnb_proba_users<36, 260>;
        hipLaunchKernelGGL(kern, dim3(users_grid(kern, lds, F)), dim3(256), lds, (hipStream_t)stream, a, ug, pl);
        return check_launch("ce_gnb_predict_proba_users");
    }
    with_nx(D, [&](auto nx) {
        auto kern = k_gnb_proba_users<decltype(nx)::value, 0>;
        if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(users_grid(kern, lds, F)), dim3(256), lds, (hipStream_t)stream, a, ug, pl);
    });
    return check_launch("ce_gnb_predict_proba_users");
}

extern "C" int ce_sgd_predict_proba_users(const double* X, int64_t F, int32_t D, int64_t ld, const double* coef,
                                          const double* intercept, int32_t K, int32_t C, int32_t U,
                                          const int64_t* item_offsets, const int64_t* frame_offsets,
                                          const int64_t* frame_perm, const uint32_t* excl, double* out,
                                          int64_t ld_out, ce_stream_t stream) {
    if (F < 0 || D < 1 || D > kMaxFeat || ld < D || C < 2 || C > kMaxMemberC || ld_out < C ||
        !(K == C || (K == 1 && C == 2)))
        return fail(CE_EINVAL, "bad SGD shapes F=%lld D=%d K=%d C=%d", (long long)F, D, K, C);
    int rc = check_users_geom(U, item_offsets, frame_offsets);
    if (rc) return rc;
    if ((F > 0 && (!X || !out)) || !coef || !intercept) return fail(CE_EINVAL, "null pointer");
    if (F == 0) return CE_OK;
    SgdArgs a{X, F, D, ld, coef, intercept, K, C, out, ld_out};
    UsersGeom ug{item_offsets, frame_offsets, frame_perm, excl, U};
    const size_t lds = ((size_t)K * D + K) * sizeof(double);  // coef and the intercept: 32 KB at K = 8, D = 512
    with_nx(D, [&](auto nx) {
        auto kern = k_sgd_proba_users<decltype(nx)::value>;
        hipLaunchKernelGGL(kern, dim3(users_grid(kern, lds, F)), dim3(256), lds, (hipStream_t)stream, a, ug);
    });
    return check_launch("ce_sgd_predict_proba_users");
}
