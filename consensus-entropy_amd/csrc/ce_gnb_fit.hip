// ce_gnb_fit.hip -- C-ABI entry of the GaussianNB partial_fit (ce_gnb_fit.hpp):
// the only TU that instantiates its kernel.
#include "ce_host.hpp"
#include "ce_gnb_fit.hpp"

using namespace ce;

// accumulators for 2, 4 or 8 classes (the reference: 4 quadrants)
template <bool VEC2>
static void launch_fit(const GnbFitArgs& a, int U, hipStream_t st) {
    if (a.C <= 2) hipLaunchKernelGGL((k_gnb_partial_fit<VEC2, 2>), dim3(U), dim3(kFitBS), 0, st, a);
    else if (a.C <= 4) hipLaunchKernelGGL((k_gnb_partial_fit<VEC2, 4>), dim3(U), dim3(kFitBS), 0, st, a);
    else hipLaunchKernelGGL((k_gnb_partial_fit<VEC2, kFitMaxC>), dim3(U), dim3(kFitBS), 0, st, a);
}

extern "C" int ce_gnb_partial_fit(const double* X, int64_t F, int32_t D, int64_t ld, const int64_t* rows,
                                  const int32_t* labels, const int64_t* row_offsets, int32_t U, int32_t C,
                                  double var_smoothing, double* theta, double* var, double* class_count,
                                  double* class_prior, double* epsilon, ce_stream_t stream) {
    if (F < 0 || D < 1 || D > 2 * kFitBS || ld < D || C < 2 || C > kFitMaxC || U < 1)
        return fail(CE_EINVAL, "bad GaussianNB partial_fit shapes F=%lld D=%d ld=%lld C=%d U=%d", (long long)F, D,
                    (long long)ld, C, U);
    if (!X || !rows || !labels || !row_offsets || !theta || !var || !class_count || !class_prior || !epsilon)
        return fail(CE_EINVAL, "null pointer");
    // numpy sums one feature's column as a contiguous pairwise sum, not row after row
    if (D < 2) return fail(CE_EUNSUPPORTED, "GaussianNB partial_fit needs D >= 2 features (got %d)", D);
    if (F == 0) return CE_OK;  // no frame, so no row: every batch is empty
    GnbFitArgs a{X, F, D, ld, rows, labels, row_offsets, C, var_smoothing, theta, var, class_count, class_prior, epsilon};
    const bool vec2 = D % 2 == 0 && ld % 2 == 0 && ((uintptr_t)X & 15) == 0;
    if (vec2) launch_fit<true>(a, U, (hipStream_t)stream);
    else launch_fit<false>(a, U, (hipStream_t)stream);
    return check_launch("ce_gnb_partial_fit");
}
