// softmax_rule.h -- the float64 softmax of a row of A float32 scores as include/snac_hip.h states it ("Acting from a policy"), once, for
// every unit that takes one: k_policy.hip, soft_rule.h and ppo_rule.h.  Three steps that a caller runs in turn -- the scan, the terms,
// the sums -- each operation rounded on its own and in the header's order, so the entropy of a row is the same bytes whichever unit
// computes it.  The steps stay apart because their callers differ between them: snac_policy_act draws from a bad row as if every score
// were 0 where the other two return zeros, and it takes the sums and LOG only when logp or entropy is asked for.  Host and device, as
// spec_math.h: a host compiler needs -ffp-contract=off.  All arrays are indexed by unrolled constants.
#pragma once
#include <cmath>

#include "spec_math.h"

namespace snac_spec {

// The scan: m = the row's largest score; returns whether the row is bad (a NaN or +inf score, or every score -inf).
template <int A>
SNAC_SPEC_FN bool softmax_scan(const float (&l)[A], float& m) {
#pragma clang fp contract(off)
    m = l[0];
    bool bad = false;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        if (a && l[a] > m) m = l[a];
        bad |= (l[a] != l[a]) || l[a] == INFINITY;
    }
    bad |= m == -INFINITY;
    return bad;
}

// The terms: x_a = l_a - m and e_a = EXP(x_a).
template <int A>
SNAC_SPEC_FN void softmax_terms(const float (&l)[A], float m, double (&x)[A], double (&e)[A]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int a = 0; a < A; ++a) {
        x[a] = (double)l[a] - (double)m;
        e[a] = spec_exp(x[a]);
    }
}

// The sums, in index order from 0.0: S = sum e_a, T = sum e_a x_a, and L = LOG(S).
struct SoftmaxSums {
    double S, T, L;
};

template <int A>
SNAC_SPEC_FN SoftmaxSums softmax_sums(const double (&x)[A], const double (&e)[A]) {
#pragma clang fp contract(off)
    double S = 0.0, T = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        S = S + e[a];
        T = T + (e[a] == 0.0 ? 0.0 : e[a] * x[a]);                   // x may be -inf where e is 0: that term is 0.0
    }
    return {S, T, spec_log(S)};
}

// The entropy of the row.
SNAC_SPEC_FN double softmax_entropy(const SoftmaxSums& s) {
#pragma clang fp contract(off)
    return s.L - s.T / s.S;
}

}  // namespace snac_spec
