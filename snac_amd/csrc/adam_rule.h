// adam_rule.h -- the rule of include/snac_hip.h, "Optimiser step of the device network", in the pieces that k_adam.hip runs per lane and
// that a host compiler can compile as they stand (tests/native/adam_host.cpp, with -ffp-contract=off): the clip coefficient from the sum
// of squares, the constants of a step, one parameter's Adam update and one parameter's move of the target.  Every float64 operation below
// is one operation of the rule, rounded on its own.  adam_sumsq_host is the sum of squares as plain loops in the stated order (what the
// host runs; the kernels spread the same additions over lanes with batch_sum.h's butterfly).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "spec_math.h"

namespace snac_spec {

// norm = sqrt(ss); max_norm == 0: no clip; else torch's clip_grad_norm_: min(max_norm / (norm + 1e-6), 1)
SNAC_SPEC_FN double adam_norm(double ss) { return std::sqrt(ss); }
SNAC_SPEC_FN double adam_coef(double ss, double max_norm) {
#pragma clang fp contract(off)
    if (max_norm == 0.0) return 1.0;
    const double c = max_norm / (adam_norm(ss) + 1e-6);
    return c < 1.0 ? c : 1.0;
}

// a bad step: some gradient is a NaN or an infinity (the square of a finite float32 cannot overflow float64)
SNAC_SPEC_FN bool adam_bad(double ss) { return !std::isfinite(ss); }

// the constants of a step, one operation each: 1 - beta1, 1 - beta2, sqrt(bias2), lr / bias1
struct AdamStep {
    double beta1, beta2, one_minus_beta1, one_minus_beta2, eps, sqrt_bias2, step;
};
SNAC_SPEC_FN AdamStep adam_step_of(double lr, double beta1, double beta2, double eps, double bias1, double bias2) {
#pragma clang fp contract(off)
    AdamStep s;
    s.beta1 = beta1, s.beta2 = beta2, s.eps = eps;
    s.one_minus_beta1 = 1.0 - beta1;
    s.one_minus_beta2 = 1.0 - beta2;
    s.sqrt_bias2 = std::sqrt(bias2);
    s.step = lr / bias1;
    return s;
}

struct AdamParam {
    float m, v, theta;
};
// one parameter: the stored, rounded m' and v' are what the update reads
SNAC_SPEC_FN AdamParam adam_param(float theta, float g, float m, float v, double coef, const AdamStep& s) {
#pragma clang fp contract(off)
    AdamParam o;
    const double gd = coef * (double)g;
    const double m1 = s.beta1 * (double)m;
    const double m2 = s.one_minus_beta1 * gd;
    o.m = (float)(m1 + m2);
    const double v1 = s.beta2 * (double)v;
    const double g2 = gd * gd;
    const double v2 = s.one_minus_beta2 * g2;
    o.v = (float)(v1 + v2);
    const double root = std::sqrt((double)o.v);
    const double scaled = root / s.sqrt_bias2;
    const double denom = scaled + s.eps;
    const double ratio = (double)o.m / denom;
    const double move = s.step * ratio;
    o.theta = (float)((double)theta - move);
    return o;
}

// one parameter of the target: tau == 1.0 copies the bits
SNAC_SPEC_FN float lerp_param(float tgt, float theta, double tau) {
#pragma clang fp contract(off)
    if (tau == 1.0) return theta;
    const double diff = (double)theta - (double)tgt;
    const double move = tau * diff;
    return (float)((double)tgt + move);
}

// the xor butterfly over 64 values in place: u_j = u_j + u_{j ^ off}, off = 32 .. 1; every place holds the sum afterwards
SNAC_SPEC_FN void adam_butterfly(double (&u)[64]) {
#pragma clang fp contract(off)
    for (int off = 32; off >= 1; off >>= 1) {
        double t[64];
        for (int j = 0; j < 64; ++j) t[j] = u[j] + u[j ^ off];
        for (int j = 0; j < 64; ++j) u[j] = t[j];
    }
}

// ss of g[0 .. P) in the stated order; partials: W = ceil(P / 64) values, written
SNAC_SPEC_FN double adam_sumsq_host(const float* g, int64_t P, double* partials) {
#pragma clang fp contract(off)
    const int64_t W = (P + 63) / 64;
    double u[64];
    for (int64_t w = 0; w < W; ++w) {
        for (int j = 0; j < 64; ++j) {
            const int64_t p = 64 * w + j;
            u[j] = p < P ? (double)g[p] * (double)g[p] : 0.0;
        }
        adam_butterfly(u);
        partials[w] = u[0];
    }
    for (int j = 0; j < 64; ++j) {
        u[j] = 0.0;
        for (int64_t w = j; w < W; w += 64) u[j] = u[j] + partials[w];
    }
    adam_butterfly(u);
    return u[0];
}

}  // namespace snac_spec
