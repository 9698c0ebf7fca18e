// lk_range_bound.h — the matcher's range gate (voxel_map.cc:380-383) without its square root.
//
// The gate is  (double)sqrtf(x) <= 3.0 * (double)radius  with x the float  dis_to_center - dis_to_plane^2.  sqrtf is correctly rounded and
// monotone, so for a given radius the floats x that pass are an interval [0, X*] (-0 included), and X* is a constant of the plane:
//     T  = 3.0 * (double)radius                    exact: a 24-bit significand times 3
//     f  = the largest float <= T                  sqrtf(x) is a float, so  sqrtf(x) <= T  <=>  sqrtf(x) <= f
//     B  = (f + ulp_above(f) / 2)^2                the midpoint between f and the next float, squared: 25 bits squared, exact in a double.
//                                                  sqrt(x) <  midpoint rounds to f or below, sqrt(x) > midpoint to the next float or above,
//                                                  and sqrt(x) == midpoint cannot happen: the midpoint's 25-bit significand is odd, and such
//                                                  a number squared needs more than the 24 bits of a float x
//     X* = the largest float < B
// so that for EVERY float x (NaN, +-0, negatives, denormals, +inf):
//     (x >= 0 && x <= X*)  ==  ((double)sqrtf(x) <= 3.0 * (double)radius)
// T < 0 gives a negative bound (nothing passes), NaN gives NaN (nothing passes), T = +inf gives +inf (every x >= 0 passes), and a finite T above
// FLT_MAX gives FLT_MAX (sqrtf never gets there; +inf still fails).
// Plain C++ when not compiled by hipcc: tests/test_range_bound.py builds a host harness around this file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LK_RANGE_FN __host__ __device__ __forceinline__
#else
#define LK_RANGE_FN static inline
#endif

LK_RANGE_FN uint32_t lk_range_f2u(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, sizeof(u));
    return u;
}
LK_RANGE_FN float lk_range_u2f(uint32_t u) {
    float v;
    __builtin_memcpy(&v, &u, sizeof(v));
    return v;
}

LK_RANGE_FN float lk_range_bound(float radius) {
    const double flt_max = 3.4028234663852886e38;   // FLT_MAX, exactly
    const double T = 3.0 * (double)radius;
    if (T != T) return radius;                       // NaN
    if (T < 0.0) return -1.0f;
    if (T == 0.0) return 0.0f;                       // only x = +-0 passes (radius = +-0)
    if (T > flt_max) return T > 1.7976931348623157e308 ? radius : 3.4028234663852886e38f;   // radius = +inf: +inf
    float f = (float)T;                              // nearest; step down if that went above T (f > T > 0: the bit pattern below is the float below)
    if ((double)f > T) f = lk_range_u2f(lk_range_f2u(f) - 1u);
    const uint32_t fu = lk_range_f2u(f);
    const double up = fu == 0x7f7fffffu ? 3.4028236692093846e38 /* 2^128 */ : (double)lk_range_u2f(fu + 1u);
    const double m = 0.5 * ((double)f + up);         // exact: two neighbouring floats
    const double B = m * m;                          // exact: 50 bits
    if (B > flt_max) return 3.4028234663852886e38f;
    float c = (float)B;
    if ((double)c >= B) c = lk_range_u2f(lk_range_f2u(c) - 1u);   // c >= B > 0
    return c;
}
