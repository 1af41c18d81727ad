// policy_dev.h -- the draw of include/snac_hip.h, "Acting from a policy", for one row of A scores, once, for the kernels that make it:
// k_policy_act (k_policy.hip: the scores from memory) and k_policy_rollout (k_policy_roll.hip: the scores are the network's outputs, in
// LDS).  softmax_rule.h states the softmax.  Device code only; all arrays are indexed by unrolled constants: no scratch.
#pragma once
#include <cmath>

#include "snac_hip.h"
#include "softmax_rule.h"

namespace snac_policy_dev {

using namespace snac_spec;

struct PolicyDraw {
    int action;
    bool bad;                                                        // the row was drawn as if every score were 0: one more in bad_rows[0]
    float logp, entropy;                                             // categorical mode, where asked for; else 0
};

// s: the row's scores (zeroed here when the row is bad); w: the env's word of stream 5; eps: the epsilon of the epsilon-greedy mode
// (the per-env value widened, or the scalar); want_logp / want_entropy: uniform
template <int A, int MODE>
__device__ __forceinline__ PolicyDraw policy_draw(float (&s)[A], uint32_t w, double eps, bool want_logp, bool want_entropy) {
    PolicyDraw o{0, false, 0.0f, 0.0f};
    float m;
    if (softmax_scan(s, m)) {                                        // a bad row: drawn as if every score were 0
        m = 0.0f;
#pragma unroll
        for (int a = 0; a < A; ++a) s[a] = 0.0f;
        o.bad = true;
    }
    int greedy = A - 1;
#pragma unroll
    for (int a = A - 2; a >= 0; --a) greedy = s[a] == m ? a : greedy;    // the lowest index of the largest score

    int action = greedy;
    if (MODE == SNAC_POLICY_EPS_GREEDY) {
        const double v = floor(eps * 65536.0);
        const uint32_t eps_fx = v >= 65536.0 ? 65536u : v > 0.0 ? (uint32_t)v : 0u;
        if ((w >> 16) < eps_fx) action = (int)(((w & 0xffffu) * (uint32_t)A) >> 16);
    }
    if (MODE == SNAC_POLICY_CATEGORICAL) {
        double x[A], e[A];
        softmax_terms(s, m, x, e);
        uint32_t wt[A], total = 0;                                   // total <= 8 * 2^28 = 2^31
#pragma unroll
        for (int a = 0; a < A; ++a) {
            wt[a] = (uint32_t)(uint64_t)floor(e[a] * 268435456.0);   // a power of two: the product is exact
            total += wt[a];
        }
        const uint32_t u = __umulhi(w, total);                       // ((uint64)w * total) >> 32, below total
        uint32_t cum = 0;
        bool found = false;
        double xa = x[A - 1];
        action = A - 1;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            cum += wt[a];
            const bool hit = !found && cum > u;
            action = hit ? a : action;
            xa = hit ? x[a] : xa;
            found |= hit;
        }
        if (want_logp || want_entropy) {
            const SoftmaxSums sm = softmax_sums(x, e);
            if (want_logp) {
#pragma clang fp contract(off)
                o.logp = (float)(xa - sm.L);
            }
            if (want_entropy) o.entropy = (float)softmax_entropy(sm);
        }
    }
    o.action = action;
    return o;
}

}  // namespace snac_policy_dev
