// ce_members_score.hip -- C-ABI entries of the evaluate step of the linear
// members (ce_members_score.hpp): the only TU that instantiates its kernels.
// ce_*_score_users: one stream-ordered memset of cm (under capture: one memset
// node) and one launch; ce_f1_weighted_users: one launch.  No workspace,
// nothing synchronised: capturable.
#include "ce_dispatch.hpp"
#include "ce_members_score.hpp"

using namespace ce;

// What the two score entry points check alike, after their own shapes; cm is zero-filled here.
static int score_common(const char* what, int64_t F, int32_t C, int32_t U, const int64_t* item_offsets,
                        const int64_t* frame_offsets, const int32_t* y, int64_t* cm, const double* scores,
                        int64_t ld_scores, int32_t score_cols, hipStream_t st) {
    const int rc = check_users_geom(U, item_offsets, frame_offsets);
    if (rc) return rc;
    if (!cm || (F > 0 && !y)) return fail(CE_EINVAL, "null y or cm");
    if (scores && ld_scores < score_cols)
        return fail(CE_EINVAL, "ld_scores=%lld below the %d score column(s)", (long long)ld_scores, score_cols);
    const hipError_t e = hipMemsetAsync(cm, 0, (size_t)U * C * C * sizeof(int64_t), st);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(CE_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    }
    return CE_OK;
}

extern "C" int ce_gnb_score_users(const double* X, int64_t F, int32_t D, int64_t ld, const double* theta,
                                  const double* var, const double* log_prior, int32_t C, int32_t U,
                                  const int64_t* item_offsets, const int64_t* frame_offsets,
                                  const int64_t* frame_perm, const uint32_t* excl, const int32_t* y, int64_t* cm,
                                  int32_t* pred, double* scores, int64_t ld_scores, ce_stream_t stream) {
    note_kernel("%s", "");
    if (F < 0 || D < 1 || D > kMaxFeat || ld < D || C < 2 || C > kMaxMemberC)
        return fail(CE_EINVAL, "bad GaussianNB shapes F=%lld D=%d C=%d", (long long)F, D, C);
    if ((F > 0 && !X) || !theta || !var || !log_prior) return fail(CE_EINVAL, "null pointer");
    if (D < 8) return fail(CE_EUNSUPPORTED, "GaussianNB needs D >= 8 features (got %d)", D);  // as ce_gnb_predict_proba
    int rc = score_common("ce_gnb_score_users", F, C, U, item_offsets, frame_offsets, y, cm, scores, ld_scores, C,
                          (hipStream_t)stream);
    if (rc || F == 0) return rc;
    GnbArgs a{X, F, D, ld, theta, var, log_prior, C, nullptr, 0};
    UsersGeom ug{item_offsets, frame_offsets, frame_perm, excl, U};
    ScoreOut o{y, reinterpret_cast<unsigned long long*>(cm), pred, scores, ld_scores};
    const PwPlan pl = pw_plan(D);
    const size_t lds = (size_t)3 * C * D * sizeof(double);  // up to 96 KB at C = 8, D = 512
    if (D == 260 && ld == 260 && C == 4) {  // the reference's contiguous rows: feature-streamed
        auto kern = k_gnb_score_users260<4, 3>;
        note_kernel("%s", "ce::k_gnb_score_users260<4, 3>");
        hipLaunchKernelGGL(kern, dim3(users_grid(kern, 0, F)), dim3(256), 0, (hipStream_t)stream, a, ug, o);
        return check_launch("ce_gnb_score_users");
    }
    if (D == 260) {  // the reference's feature count: constant pairwise plan
        auto kern = k_gnb_score_users<36, 260>;
        note_kernel("%s", "ce::k_gnb_score_users<36, 260>");
        hipLaunchKernelGGL(kern, dim3(users_grid(kern, lds, F)), dim3(256), lds, (hipStream_t)stream, a, ug, pl, o);
        return check_launch("ce_gnb_score_users");
    }
    with_nx(D, [&](auto nx) {
        auto kern = k_gnb_score_users<decltype(nx)::value, 0>;
        note_kernel("ce::k_gnb_score_users<%d, 0>", (int)decltype(nx)::value);
        if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(users_grid(kern, lds, F)), dim3(256), lds, (hipStream_t)stream, a, ug, pl, o);
    });
    return check_launch("ce_gnb_score_users");
}

extern "C" int ce_sgd_score_users(const double* X, int64_t F, int32_t D, int64_t ld, const double* coef,
                                  const double* intercept, int32_t K, int32_t C, int32_t U,
                                  const int64_t* item_offsets, const int64_t* frame_offsets,
                                  const int64_t* frame_perm, const uint32_t* excl, const int32_t* y, int64_t* cm,
                                  int32_t* pred, double* scores, int64_t ld_scores, ce_stream_t stream) {
    note_kernel("%s", "");
    if (F < 0 || D < 1 || D > kMaxFeat || ld < D || C < 2 || C > kMaxMemberC || !(K == C || (K == 1 && C == 2)))
        return fail(CE_EINVAL, "bad SGD shapes F=%lld D=%d K=%d C=%d", (long long)F, D, K, C);
    if ((F > 0 && !X) || !coef || !intercept) return fail(CE_EINVAL, "null pointer");
    int rc = score_common("ce_sgd_score_users", F, C, U, item_offsets, frame_offsets, y, cm, scores, ld_scores, K,
                          (hipStream_t)stream);
    if (rc || F == 0) return rc;
    SgdArgs a{X, F, D, ld, coef, intercept, K, C, nullptr, 0};
    UsersGeom ug{item_offsets, frame_offsets, frame_perm, excl, U};
    ScoreOut o{y, reinterpret_cast<unsigned long long*>(cm), pred, scores, ld_scores};
    const size_t lds = ((size_t)K * D + K) * sizeof(double);  // coef and the intercept: 32 KB at K = 8, D = 512
    with_nx(D, [&](auto nx) {
        auto kern = k_sgd_score_users<decltype(nx)::value>;
        note_kernel("ce::k_sgd_score_users<%d>", (int)decltype(nx)::value);
        hipLaunchKernelGGL(kern, dim3(users_grid(kern, lds, F)), dim3(256), lds, (hipStream_t)stream, a, ug, o);
    });
    return check_launch("ce_sgd_score_users");
}

extern "C" int ce_f1_weighted_users(const int64_t* cm, int32_t U, int32_t C, double* f1, double* prf,
                                    ce_stream_t stream) {
    if (U < 1 || C < 2 || C > kMaxMemberC) return fail(CE_EINVAL, "bad F1 shapes U=%d C=%d", U, C);
    if (!cm || !f1) return fail(CE_EINVAL, "null cm or f1");
    hipLaunchKernelGGL(k_f1_weighted_users, dim3((U + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(cm), U, C, f1, prf);
    return check_launch("ce_f1_weighted_users");
}
