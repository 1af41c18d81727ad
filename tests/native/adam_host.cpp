// adam_host.cpp -- the rule k_adam runs (snac_amd/csrc/adam_rule.h), compiled for the host as it stands: tests/test_adam_host.py builds
// this file into a shared object with the system compiler and -ffp-contract=off and compares every output's bytes with the numpy statement
// of the rule.  The loops below are the launch sequence's with the flat index a loop index: the sum of squares in the stated order
// (adam_sumsq_host), the clip, then adam_param and lerp_param per parameter; theta and tgt are flat here, where the kernels walk the
// layers' arrays.  With -DADAM_HOST_MAIN the file is a program: every size class of the GPU tests in exactly sized heap arrays, for a run
// under the host sanitizers.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "adam_rule.h"

// -> 0: a step; 1: a bad step (nothing but norm_out and partials written); -1: refused (P < 1).  tgt may be NULL, norm_out may be NULL.
extern "C" int adam_host(int64_t P, float* theta, const float* g, float* m, float* v, double lr, double beta1, double beta2, double eps,
                         double bias1, double bias2, double max_norm, float* tgt, double tau, double* norm_out, double* partials) {
    using namespace snac_spec;
    if (P < 1) return -1;
    const double ss = adam_sumsq_host(g, P, partials);
    const bool bad = adam_bad(ss);
    const double coef = bad ? 0.0 : adam_coef(ss, max_norm);
    if (norm_out) norm_out[0] = adam_norm(ss), norm_out[1] = coef;
    if (bad) return 1;
    const AdamStep s = adam_step_of(lr, beta1, beta2, eps, bias1, bias2);
    for (int64_t p = 0; p < P; ++p) {
        const AdamParam o = adam_param(theta[p], g[p], m[p], v[p], coef, s);
        m[p] = o.m, v[p] = o.v, theta[p] = o.theta;
        if (tgt) tgt[p] = lerp_param(tgt[p], o.theta, tau);
    }
    return 0;
}

extern "C" int lerp_host(int64_t P, float* tgt, const float* theta, double tau) {
    if (P < 1) return -1;
    for (int64_t p = 0; p < P; ++p) tgt[p] = snac_spec::lerp_param(tgt[p], theta[p], tau);
    return 0;
}

#ifdef ADAM_HOST_MAIN
#include <cstdio>
#include <cstring>

// The sizes of the GPU tests (under one wave, a partly filled last wave, more than 64 waves, a large grid) and the edges of a wave, with
// and without a target, clipped and not, and a bad step: anything indexed past P or past the W partials shows under
// -fsanitize=address,undefined.  Prints the counts; exit status 1 if one is off: three steps move the parameters, a bad step
// leaves every array's bytes as they were.
int main() {
    const int64_t sizes[] = {1, 2, 32, 63, 64, 65, 3718, 4096, 4097, 7878, 196102};
    int status = 0;
    for (int64_t P : sizes) {
        for (int target = 0; target < 2; ++target) {
            const int64_t W = (P + 63) / 64;
            std::vector<float> theta((size_t)P), g((size_t)P), m((size_t)P), v((size_t)P), tgt((size_t)P);
            std::vector<double> partials((size_t)W);
            for (int64_t p = 0; p < P; ++p) {
                theta[p] = 0.03125f * (float)((p * 7) % 31 - 15);
                g[p] = 0.25f * (float)((p * 5) % 13 - 6) + 0.125f;
                m[p] = 0.0625f * (float)((p * 3) % 11 - 5);
                v[p] = 0.015625f * (float)((p * 11) % 17);
                tgt[p] = -theta[p];
            }
            int bad = 0;
            double norm_out[2] = {-1.0, -1.0};
            const std::vector<float> before = theta;
            for (double max_norm : {0.0, 0.5, 1.0e9}) {
                const int rc = adam_host(P, theta.data(), g.data(), m.data(), v.data(), 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, max_norm,
                                         target ? tgt.data() : nullptr, target ? 0.005 : 0.0, norm_out, partials.data());
                bad += rc != 0;
                bad += !(norm_out[0] > 0.0) || !(norm_out[1] > 0.0 && norm_out[1] <= 1.0);
                bad += max_norm == 0.5 && P >= 32 && !(norm_out[1] < 1.0);
                bad += max_norm != 0.5 && norm_out[1] != 1.0;
            }
            int64_t still = 0;                                       // (a moment that cancels to nearly nothing may leave a parameter where it was)
            for (int64_t p = 0; p < P; ++p) still += theta[p] == before[p];
            bad += still > P / 8;
            if (target) bad += lerp_host(P, tgt.data(), theta.data(), 1.0) != 0 || std::memcmp(tgt.data(), theta.data(), (size_t)P * 4) != 0;
            // a bad step: a NaN at the last flat index and an infinity at index 0
            g[(size_t)P - 1] = NAN;
            g[0] = P > 1 ? INFINITY : NAN;
            const std::vector<float> t0 = theta, m0 = m, v0 = v, g0 = tgt;
            bad += adam_host(P, theta.data(), g.data(), m.data(), v.data(), 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, 0.5, target ? tgt.data() : nullptr,
                             1.0, norm_out, partials.data()) != 1;
            bad += norm_out[1] != 0.0 || std::isfinite(norm_out[0]);
            bad += std::memcmp(t0.data(), theta.data(), (size_t)P * 4) != 0 || std::memcmp(m0.data(), m.data(), (size_t)P * 4) != 0;
            bad += std::memcmp(v0.data(), v.data(), (size_t)P * 4) != 0 || std::memcmp(g0.data(), tgt.data(), (size_t)P * 4) != 0;
            std::printf("P %lld target %d: W %lld, off %d\n", (long long)P, target, (long long)W, bad);
            if (bad) status = 1;
        }
    }
    if (adam_host(0, nullptr, nullptr, nullptr, nullptr, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, 0.0, nullptr, 1.0, nullptr, nullptr) != -1) status = 1;
    return status;
}
#endif
