// search_rule.h -- the per-sample rule of include/snac_hip.h, "Search loss (AlphaZero / Gumbel self-play)", as one function that
// k_search.hip runs per lane and that a host compiler can compile as it stands (tests/native/search_host.cpp, with -ffp-contract=off):
// the cross-entropy of the network's policy to the search's distribution pi, the squared or Huber error of its value to the return z,
// the gradient with respect to the row of logits and to the value, the new priority |value - z| and the sample's eight contributions to
// the batch statistics.  The softmax is softmax_rule.h's.  Every float64 operation below is one operation of the rule, rounded on its own.
#pragma once
#include <cmath>
#include <cstdint>

#include "softmax_rule.h"

namespace snac_spec {

// the places of a sample's contributions u[0..8), which are the places of stats[0..8) of snac_search_loss
enum { SEARCH_TOTAL = 0, SEARCH_POLICY = 1, SEARCH_VALUE = 2, SEARCH_ENTROPY = 3, SEARCH_ABS = 4, SEARCH_AGREE = 5, SEARCH_GOOD = 6, SEARCH_WEIGHT = 7,
       SEARCH_STATS = 8 };

struct SearchParams {
    double vf_coef, delta, scale;                                    // delta == 0: the squared value error; > 0: Huber's
};

template <int A>
struct SearchSample {                                                // what one sample gives; bad: it counts in bad_rows and the rest is zero
    float loss, priority, grad_value;
    float grad[A];
    double u[SEARCH_STATS];
    bool bad;
};

// One sample.  weighted: weight is read and checked.  All arrays are indexed by unrolled constants; the places of the largest logit and
// of the largest pi are carried along with the compares.
template <int A>
SNAC_SPEC_FN SearchSample<A> search_sample(const float (&l)[A], float value, const float (&pi)[A], float z, float weight, bool weighted,
                                           const SearchParams& p) {
#pragma clang fp contract(off)
    SearchSample<A> o;
    o.loss = o.priority = o.grad_value = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) o.grad[a] = 0.0f;
#pragma unroll
    for (int k = 0; k < SEARCH_STATS; ++k) o.u[k] = 0.0;
    float m;
    bool bad = softmax_scan(l, m);
#pragma unroll
    for (int a = 0; a < A; ++a) {
        bad |= !(fabsf(pi[a]) < INFINITY) || pi[a] < 0.0f;           // -0.0 is a zero, not negative
        bad |= pi[a] > 0.0f && l[a] == -INFINITY;                    // a target on a masked action
    }
    bad |= !(fabsf(value) < INFINITY) || !(fabsf(z) < INFINITY);
    if (weighted) bad |= !(fabsf(weight) < INFINITY) || weight < 0.0f;
    o.bad = bad;
    if (bad) return o;
    double x[A], e[A];
    softmax_terms(l, m, x, e);
    const SoftmaxSums s = softmax_sums(x, e);
    const double H = softmax_entropy(s);
    double M = 0.0, ce = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const double pa = (double)pi[a];
        const double lp = x[a] - s.L;                                // finite for every finite logit, also where EXP gave e == 0
        M = M + pa;
        ce = ce + (pa == 0.0 ? 0.0 : pa * lp);                       // lp is -inf at a masked action, where pi is 0: that term is 0.0
    }
    const double Lpi = -ce;
    int al = 0, ap = 0;                                              // the first largest logit and the first largest pi
    float bl = l[0], bp = pi[0];
#pragma unroll
    for (int a = 1; a < A; ++a) {
        const bool wl = l[a] > bl, wp = pi[a] > bp;                  // ties keep the lower index
        bl = wl ? l[a] : bl;
        al = wl ? a : al;
        bp = wp ? pi[a] : bp;
        ap = wp ? a : ap;
    }
    const double dv = (double)value - (double)z;
    const double ab = fabs(dv);
    double Lv, g;
    if (p.delta == 0.0) {
        Lv = dv * dv;
        g = 2.0 * dv;
    } else {
        const bool lin = ab > p.delta;
        Lv = lin ? p.delta * (ab - 0.5 * p.delta) : 0.5 * (dv * dv);
        g = lin ? (dv < 0.0 ? -p.delta : p.delta) : dv;
    }
    const double per = Lpi + p.vf_coef * Lv;
    const double w = weighted ? (double)weight : 1.0;
    const double total = w * per;
    o.loss = (float)per;
    o.priority = (float)ab;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const double pa = e[a] / s.S;
        o.grad[a] = l[a] == -INFINITY ? 0.0f : (float)(p.scale * (w * (M * pa - (double)pi[a])));
    }
    o.grad_value = (float)(p.scale * (w * (p.vf_coef * g)));
    o.u[SEARCH_TOTAL] = total;
    o.u[SEARCH_POLICY] = Lpi;
    o.u[SEARCH_VALUE] = Lv;
    o.u[SEARCH_ENTROPY] = H;
    o.u[SEARCH_ABS] = ab;
    o.u[SEARCH_AGREE] = al == ap ? 1.0 : 0.0;
    o.u[SEARCH_GOOD] = 1.0;
    o.u[SEARCH_WEIGHT] = w;
    return o;
}

// The second stage of the reduction for one of the eight sums, as the second kernel's lane j runs its first half: partials[j],
// partials[j + 64], ... of column k added in increasing order from 0.0 (W rows of SEARCH_STATS doubles).
SNAC_SPEC_FN double search_lane_sum(const double* partials, long long W, int j, int k) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (long long w = j; w < W; w += 64) s = s + partials[w * SEARCH_STATS + k];
    return s;
}

}  // namespace snac_spec
