// ce_dispatch.hpp -- what only the objects that launch kernels need: the
// runtime (dtype, C, alignment) -> compile-time choice of an item source
// (with_committee) or of the wide kernels' parameters (with_wide_v), the wide
// kernels' arguments, and the resident grid of a kernel.  Included by the
// ce_launch_*.hip files and by the launcher parts of ce_abi_core.hip and
// ce_abi_frames.hip; the entry points see ce_host.hpp alone.
#pragma once
#include "ce_host.hpp"
#include "ce_src.hpp"
#include "ce_wide.hpp"  // WideArgs, kWideMaxC, wide_lds_doubles

// ---- committee dispatch ----------------------------------------------------
static inline bool vec_ok(const CommArgs& a, int C) {
    if (a.sC != 1) return false;
    const int eb = elem_bytes(a.dt);
    const int vb = a.dt == kBF16 ? 8 : 16;  // bytes per vector load
    if (a.dt == kF64 ? (C % 2) : (C % 4)) return false;
    if ((uintptr_t)a.p % vb) return false;
    if ((a.sN * eb) % vb || (a.sM * eb) % vb) return false;
    return true;
}

template <int DT, int C, bool VEC>
static inline CommitteeSrc<DT, C, VEC> make_src(const CommArgs& a) {
    CommitteeSrc<DT, C, VEC> s;
    s.p = a.p;
    s.sN = a.sN;
    s.sM = a.sM;
    s.sC = a.sC;
    s.M = a.M;
    s.dM = (double)a.M;
    s.invM = 1.0 / (double)a.M;
    s.pow2 = (a.M & (a.M - 1)) == 0;
    return s;
}

// Calls f(src) with the CommitteeSrc instantiation matching (dtype, C, vec).
template <class F>
static inline int with_committee(const CommArgs& a, F&& f) {
#define CE_CASE(DT_, C_)                                       \
    if (a.dt == DT_ && a.C == C_) {                            \
        if (vec_ok(a, C_)) f(make_src<DT_, C_, true>(a));      \
        else f(make_src<DT_, C_, false>(a));                   \
        return CE_OK;                                          \
    }
    CE_CASE(kF32, 4) CE_CASE(kF64, 4) CE_CASE(kBF16, 4)
    CE_CASE(kF32, 8) CE_CASE(kF64, 8) CE_CASE(kBF16, 8)
    CE_CASE(kF64, 2)
#undef CE_CASE
#define CE_CASE_S(DT_, C_)                                     \
    if (a.dt == DT_ && a.C == C_) {                            \
        f(make_src<DT_, C_, false>(a));                        \
        return CE_OK;                                          \
    }
    CE_CASE_S(kF32, 2) CE_CASE_S(kBF16, 2)
    CE_CASE_S(kF32, 3) CE_CASE_S(kF64, 3) CE_CASE_S(kBF16, 3)
#undef CE_CASE_S
    return CE_EUNSUPPORTED;
}

// ---- wide-class dispatch (C not in the register-path set) -------------------
static inline WideArgs wide_args(const CommArgs& a) {
    WideArgs w{a.p, a.N, a.M, a.C, a.sN, a.sM, a.sC, (double)a.M, 1.0 / (double)a.M, (a.M & (a.M - 1)) == 0};
    return w;
}
static inline size_t wide_lds_bytes(int C) { return (size_t)4 * wide_lds_doubles(C) * sizeof(double); }

static inline bool wide_vec_ok(const CommArgs& a) {
    const int eb = elem_bytes(a.dt);
    return a.sC == 1 && (a.C * eb) % 16 == 0 && (a.sM * eb) % 16 == 0 && (a.sN * eb) % 16 == 0 &&
           (uintptr_t)a.p % 16 == 0;
}

// f(dt, npl, vec) with compile-time values
template <class F>
static inline int with_wide_v(const CommArgs& a, F&& f) {
    if (a.C > kWideMaxC) return CE_EUNSUPPORTED;
    const bool vec = wide_vec_ok(a);
#define CE_WV(DT_, NPL_)                                                                              \
    if (vec) f(std::integral_constant<int, DT_>(), std::integral_constant<int, NPL_>(), std::true_type()); \
    else f(std::integral_constant<int, DT_>(), std::integral_constant<int, NPL_>(), std::false_type());
#define CE_WD(DT_)                                   \
    if (a.dt == DT_) {                               \
        if (a.C <= 512) { CE_WV(DT_, 8) }            \
        else if (a.C <= 1024) { CE_WV(DT_, 16) }     \
        else { CE_WV(DT_, 32) }                      \
        return CE_OK;                                \
    }
    CE_WD(kF32) CE_WD(kF64) CE_WD(kBF16)
#undef CE_WD
#undef CE_WV
    return CE_EUNSUPPORTED;
}

// ---- member inference dispatch (ce_members.hpp, ce_members_users.hpp, ce_members_score.hpp) ----
// features per lane of the 8-lanes-per-frame kernels: ceil(D / 8), rounded up to a multiple of 8
template <class F>
static inline int with_nx(int D, F&& f) {
    const int nx = (D + 7) / 8;
#define CE_NX(N_) if (nx <= N_) { f(std::integral_constant<int, N_>()); return CE_OK; }
    CE_NX(8) CE_NX(16) CE_NX(24) CE_NX(32) CE_NX(36) CE_NX(40) CE_NX(48) CE_NX(56) CE_NX(64)
#undef CE_NX
    return CE_EUNSUPPORTED;
}

// Blocks of `kernel` resident on the whole device (occupancy API x CUs), cached.
static inline int device_cus() {
    static int cus[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) return 256;
    if (!cus[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

template <class K>
static inline int resident_grid(K kernel, size_t dyn_lds, int cap) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, dyn_lds) != hipSuccess || per_cu < 1)
        per_cu = 1;
    (void)hipGetLastError();
    const int g = per_cu * device_cus();
    return g < cap ? g : cap;
}

// The users forms (ce_members_users.hip, ce_members_score.hip): every block
// resident at once, each with an equal share of the positions: at least 128 of
// them (4 passes of the block), so a restage is amortised.  F bounds the
// positions a well-formed geometry names; the kernel divides the real count,
// which only the device knows, among the blocks launched.
template <class K>
static inline int users_grid(K kern, size_t lds, int64_t F) {
    return resident_grid(kern, lds, (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(F, 128), 1 << 20)));
}

// What every users entry point checks of its geometry.
static inline int check_users_geom(int32_t U, const int64_t* item_offsets, const int64_t* frame_offsets) {
    if (U < 1) return fail(CE_EINVAL, "U=%d users: at least one", U);
    if (!item_offsets || !frame_offsets) return fail(CE_EINVAL, "null offsets");
    return CE_OK;
}
