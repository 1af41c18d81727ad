// spec_math.h -- EXP and LOG of include/snac_hip.h ("Acting from a policy"): fixed sequences of float64 operations, every one rounded on
// its own, so that numpy restates their results byte for byte.  For softmax_rule.h and the rules built on it (soft_rule.h, ppo_rule.h), on
// the device and on the host: the functions are __host__ __device__ under hipcc and plain inline functions under a host compiler (which then needs -ffp-contract=off; clang reads the
// pragmas below, gcc does not).  Not part of snac_dev.h: nothing of the env kernels needs them.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SNAC_SPEC_FN __host__ __device__ __forceinline__
#else
#define SNAC_SPEC_FN inline
#endif

namespace snac_spec {

constexpr double LOG2E = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42feep-1, LN2_LO = 0x1.a39ef35793c76p-33, SQRT_HALF = 0x1.6a09e667f3bcdp-1;

// EXP of the header: x <= 0 (or -inf), never a NaN
SNAC_SPEC_FN double spec_exp(double x) {
#pragma clang fp contract(off)                                      // every operation rounded on its own, in the header's order
    constexpr double c[14] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0, 1.0 / 362880.0,
                              1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0};
    const double xc = x < -45.0 ? -45.0 : x;                         // the series runs on a finite argument; the result is dropped below
    const double k = rint(xc * LOG2E);
    const double r = (xc - k * LN2_HI) - k * LN2_LO;
    double p = c[13];
#pragma unroll
    for (int n = 12; n >= 0; --n) p = p * r + c[n];
    const double e = ldexp(p, (int)k);
    return x < -45.0 ? 0.0 : e;
}

// LOG of the header, and its LOGP ("Exploration noise"): the same sequence for every positive normal s -- frexp takes the exponent and the
// series sees f in [sqrt 1/2, sqrt 2) alone.  Not for 0, a subnormal, a negative, an infinity or a NaN: a caller keeps those away
SNAC_SPEC_FN double spec_log(double s) {
#pragma clang fp contract(off)
    constexpr double d[11] = {1.0, 1.0 / 3.0, 1.0 / 5.0, 1.0 / 7.0, 1.0 / 9.0, 1.0 / 11.0, 1.0 / 13.0, 1.0 / 15.0, 1.0 / 17.0, 1.0 / 19.0, 1.0 / 21.0};
    int e;
    double f = frexp(s, &e);
    if (f < SQRT_HALF) { f = f * 2.0; e = e - 1; }
    const double z = (f - 1.0) / (f + 1.0);
    const double z2 = z * z;
    double q = d[10];
#pragma unroll
    for (int n = 9; n >= 0; --n) q = q * z2 + d[n];
    return (double)e * LN2_HI + ((2.0 * z) * q + (double)e * LN2_LO);
}

}  // namespace snac_spec
