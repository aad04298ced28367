// ce_glibc_expf.hpp -- glibc's f32 expf, restated bit for bit for the device.
//
// Why: xgboost 1.3.3's softmax and logistic transforms (ce_xgb.hpp) call expf
// from the C library; with this routine the XGB member's probabilities are the
// reference's bit for bit.
//
// Algorithm: glibc >= 2.27 sysdeps/ieee754/flt-32/e_expf.c (EXP2F_TABLE_BITS =
// 5), as its x86-64 FMA ifunc variant (__expf_fma) evaluates it: the
// __builtin_fma calls below are the multiplies GCC's contraction fuses there;
// tab[i] = bits(2^(i/32)) - (i << 52) / 32.  Verified bit-identical to the
// host's libm on all 2^32 floats: tests/test_xgb.py on a dense stride (the host
// restatement), tests/test_gpu_xgb.py exhaustively on the device (ce_xgb_expf).
//
// Included by ce_xgb.hip alone: the table is a __constant__ of that code object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ce {

__constant__ uint64_t kExp2fTab[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
    0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
    0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
    0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
    0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
    0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
    0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};

__device__ __forceinline__ float glibc_expf(float x) {
    const uint32_t ux = __float_as_uint(x);
    const uint32_t abstop = (ux >> 20) & 0x7ff;
    if (abstop >= 0x42bu) {  // |x| >= 88 or NaN
        if (ux == 0xff800000u) return 0.0f;
        if (abstop >= 0x7f8u) return x + x;
        if (x > 0x1.62e42ep6f) return __uint_as_float(0x7f800000u);
        if (x < -0x1.9fe368p6f) return 0.0f;
    }
    constexpr double kN = 32.0;
    const double inv_ln2_n = 0x1.71547652b82fep+0 * kN;
    const double c0 = 0x1.c6af84b912394p-5 / kN / kN / kN, c1 = 0x1.ebfce50fac4f3p-3 / kN / kN,
                 c2 = 0x1.62e42ff0c52d6p-1 / kN;
    const double shift = 0x1.8p+52;
    const double xd = (double)x;
    const double z = inv_ln2_n * xd;
    double kd = z + shift;
    const uint64_t ki = (uint64_t)__double_as_longlong(kd);
    kd -= shift;
    const double r = __builtin_fma(inv_ln2_n, xd, -kd);  // the FMA build contracts z - kd
    uint64_t t = kExp2fTab[ki % 32];
    t += ki << (52 - 5);
    const double s = __longlong_as_double((long long)t);
    const double zz = __builtin_fma(c0, r, c1);
    const double r2 = r * r;
    double y = __builtin_fma(c2, r, 1.0);
    y = __builtin_fma(zz, r2, y);
    y = y * s;
    return (float)y;
}

}  // namespace ce
