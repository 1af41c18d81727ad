// soft_rule.h -- the per-sample rule of include/snac_hip.h, "Soft values (discrete SAC)", as one function that k_soft.hip runs per lane
// and that a host compiler can compile as it stands (tests/native/soft_host.cpp, with -ffp-contract=off): the soft state value, the TD
// target, the entropy and the gradient of the actor loss with respect to the logits, all from one softmax (softmax_rule.h states it).  Every float64
// operation below is one operation of the rule, rounded on its own; sums run in index order from 0.0.
#pragma once
#include <cmath>

#include "softmax_rule.h"

namespace snac_spec {

template <int A>
struct SoftSample {                                                  // what one sample gives; bad: it counts in bad_rows and the rest is zero
    float v, y, entropy;
    float grad[A];
    bool bad;
};

// One sample.  use_q: v, y or grad is asked for, so q1, (TWO_Q) q2 and alpha are read -- else they are never touched, and only the entropy
// is defined.  want_y: ret and discount are read and checked.  All arrays are indexed by unrolled constants.
template <int A, bool TWO_Q>
SNAC_SPEC_FN SoftSample<A> soft_sample(const float (&l)[A], const float (&q1)[A], const float (&q2)[A], float alpha, float ret, float discount,
                                       bool use_q, bool want_y, double scale) {
#pragma clang fp contract(off)
    SoftSample<A> o;
    float m;
    bool bad = softmax_scan(l, m);
    if (use_q) bad |= !(fabsf(alpha) < INFINITY) || alpha < 0.0f;
    if (want_y) bad |= !(fabsf(ret) < INFINITY) || !(fabsf(discount) < INFINITY) || discount < 0.0f;
    o.bad = bad;
    if (bad) {
        o.v = o.y = o.entropy = 0.0f;
#pragma unroll
        for (int a = 0; a < A; ++a) o.grad[a] = 0.0f;
        return o;
    }
    double x[A], e[A];
    softmax_terms(l, m, x, e);
    const SoftmaxSums sm = softmax_sums(x, e);
    const double S = sm.S, L = sm.L;
    o.entropy = (float)softmax_entropy(sm);
    o.v = o.y = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) o.grad[a] = 0.0f;
    if (!use_q) return o;
    const double al = (double)alpha;
    double pi[A], d[A];
    double V = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const bool live = e[a] != 0.0;
        pi[a] = e[a] / S;
        const double lp = x[a] - L;
        const double qm = (double)(TWO_Q && q2[a] < q1[a] ? q2[a] : q1[a]);      // a float compare: a NaN in q2 never wins
        d[a] = live ? qm - al * lp : 0.0;                            // a masked action's q is never read into a sum
        V = V + (live ? pi[a] * d[a] : 0.0);
    }
    o.v = (float)V;
    if (want_y) o.y = (float)((double)ret + (double)discount * V);
#pragma unroll
    for (int a = 0; a < A; ++a) o.grad[a] = e[a] != 0.0 ? (float)(scale * (pi[a] * (V - d[a]))) : 0.0f;
    return o;
}

}  // namespace snac_spec
