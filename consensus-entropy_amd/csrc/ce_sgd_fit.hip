// ce_sgd_fit.hip -- C-ABI entry of the SGDClassifier partial_fit (ce_sgd_fit.hpp):
// the only TU that instantiates its kernel.
#include "ce_host.hpp"
#include "ce_sgd_fit.hpp"

using namespace ce;

static inline int sgd_problems(int C) { return C == 2 ? 1 : C; }

extern "C" size_t ce_sgd_partial_fit_workspace_bytes(int64_t R, int32_t C) {
    if (R <= 0 || C < 2 || C > kSgdMaxK) return 0;
    const int64_t slots = (int64_t)sgd_problems(C) * R;
    // K * R indices in all: up to kSgdPermLds of them every model's permutations fit in LDS
    return slots <= kSgdPermLds ? 0 : (size_t)slots * sizeof(int32_t);
}

extern "C" int ce_sgd_partial_fit(const double* X, int64_t F, int32_t D, int64_t ld, const int64_t* rows,
                                  const int32_t* labels, const int64_t* row_offsets, int32_t U, int32_t C,
                                  double alpha, double optimal_init, const uint32_t* shuffle_seeds, int32_t grad,
                                  double* coef, double* intercept, double* t, int32_t* status, void* workspace,
                                  size_t workspace_bytes, ce_stream_t stream) {
    if (F < 0 || D < 1 || ld < D || C < 2 || U < 1)
        return fail(CE_EINVAL, "bad SGD partial_fit shapes F=%lld D=%d ld=%lld C=%d U=%d", (long long)F, D, (long long)ld,
                    C, U);
    if (D > kSgdMaxD || C > kSgdMaxK)
        return fail(CE_EUNSUPPORTED, "SGD partial_fit takes D <= %d features and C <= %d classes (got D=%d C=%d)",
                    kSgdMaxD, kSgdMaxK, D, C);
    if (!(alpha > 0.0) || !(alpha < __builtin_inf()) || !(optimal_init > 0.0) || !(optimal_init < __builtin_inf()))
        return fail(CE_EINVAL, "alpha and optimal_init must be positive and finite (got %g, %g)", alpha, optimal_init);
    if (grad != kSgdGradHalfBinomial && grad != kSgdGradLogDloss) return fail(CE_EINVAL, "unknown gradient %d", grad);
    if (!X || !rows || !labels || !row_offsets || !shuffle_seeds || !coef || !intercept || !t || !status)
        return fail(CE_EINVAL, "null pointer");
    if (workspace && ((uintptr_t)workspace & 3)) return fail(CE_EINVAL, "workspace must be 4-byte aligned");
    if (F == 0) return CE_OK;  // no frame, so no row: every batch is empty
    const int K = sgd_problems(C);
    SgdFitArgs a{X, F, D, ld, rows, labels, row_offsets, K, alpha, optimal_init, shuffle_seeds, coef, intercept, t, status,
                 (int32_t*)workspace, workspace ? (int64_t)(workspace_bytes / sizeof(int32_t)) : 0};
    if (grad == kSgdGradHalfBinomial)
        hipLaunchKernelGGL((k_sgd_partial_fit<kSgdGradHalfBinomial>), dim3(U), dim3(64 * K), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((k_sgd_partial_fit<kSgdGradLogDloss>), dim3(U), dim3(64 * K), 0, (hipStream_t)stream, a);
    return check_launch("ce_sgd_partial_fit");
}
