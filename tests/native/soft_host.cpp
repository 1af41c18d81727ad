// soft_host.cpp -- the per-sample function k_soft_value runs (snac_amd/csrc/soft_rule.h), compiled for the host as it stands:
// tests/test_sac_host.py builds this file into a shared object with the system compiler and -ffp-contract=off and compares every
// output's bytes with the numpy statement of the rule.  The loop below is k_soft_value's body with `i` a loop index; snac_soft_value's
// conventions for NULL pointers hold.
#include <cstddef>
#include <cstdint>

#include "soft_rule.h"

namespace {

template <int A>
int run(int32_t B, const float* logits, const float* q1p, const float* q2p, const float* alphap, const float* retp, const float* discountp, double scale,
        float* v, float* y, float* entropy, float* grad) {
    using namespace snac_spec;
    const bool use_q = v || y || grad, want_y = y != nullptr, two_q = use_q && q2p;
    int bad_rows = 0;
    for (int32_t i = 0; i < B; ++i) {
        const size_t at = (size_t)i * A;
        float l[A], q1[A], q2[A];
        for (int a = 0; a < A; ++a) {
            l[a] = logits[at + a];
            q1[a] = use_q ? q1p[at + a] : 0.0f;
            q2[a] = two_q ? q2p[at + a] : 0.0f;
        }
        const float ret = want_y ? retp[i] : 0.0f, discount = want_y ? discountp[i] : 0.0f, alpha = use_q ? alphap[0] : 0.0f;
        const SoftSample<A> o = two_q ? soft_sample<A, true>(l, q1, q2, alpha, ret, discount, use_q, want_y, scale)
                                      : soft_sample<A, false>(l, q1, q2, alpha, ret, discount, use_q, want_y, scale);
        bad_rows += o.bad;
        if (v) v[i] = o.v;
        if (y) y[i] = o.y;
        if (entropy) entropy[i] = o.entropy;
        if (grad)
            for (int a = 0; a < A; ++a) grad[at + a] = o.grad[a];
    }
    return bad_rows;
}

}  // namespace

// -> the number of bad samples, or -1 for an unsupported num_actions
extern "C" int soft_host(int32_t B, int32_t num_actions, const float* logits, const float* q1, const float* q2, const float* alpha, const float* ret,
                         const float* discount, double scale, float* v, float* y, float* entropy, float* grad) {
    switch (num_actions) {
        case 3: return run<3>(B, logits, q1, q2, alpha, ret, discount, scale, v, y, entropy, grad);
        case 5: return run<5>(B, logits, q1, q2, alpha, ret, discount, scale, v, y, entropy, grad);
        case 8: return run<8>(B, logits, q1, q2, alpha, ret, discount, scale, v, y, entropy, grad);
        default: return -1;
    }
}
