// td_rule.h -- the per-sample rule of include/snac_hip.h, "Q-learning losses", as one function that k_qloss.hip runs per lane and that a
// host compiler can compile as it stands (tests/native/td_host.cpp, with -ffp-contract=off): the greedy or double-DQN target of one
// sample, its squared or Huber error, the gradient with respect to the row of Q-values, the new priority and the sample's eight
// contributions to the batch statistics.  Every float64 operation below is one operation of the rule, rounded on its own.
#pragma once
#include <cmath>
#include <cstdint>

#include "spec_math.h"

namespace snac_spec {

// the places of a sample's contributions u[0..8), which are the places of stats[0..8) of snac_td_loss
enum { TD_TOTAL = 0, TD_LOSS = 1, TD_ABS = 2, TD_Q = 3, TD_Y = 4, TD_LINEAR = 5, TD_GOOD = 6, TD_WEIGHT = 7, TD_STATS = 8 };

struct TdParams {
    double delta, scale;                                             // delta == 0: the squared error; > 0: Huber's
};

template <int A>
struct TdSample {                                                    // what one sample gives; bad: it counts in bad_rows and the rest is zero
    float loss, priority, y;
    float grad[A];
    double u[TD_STATS];
    bool bad;
};

// One sample.  NEXT: the target is ret + discount * nxt[a_star], a_star the largest of sel (the caller passes nxt as sel without a
// q_select), and y is never looked at; else the target is y, and sel, nxt, ret and discount are never looked at.  weighted: weight is
// read and checked.  All arrays are indexed by unrolled constants; the taken and the chosen action's values are picked by compares.
template <int A, bool NEXT>
SNAC_SPEC_FN TdSample<A> td_sample(const float (&q)[A], int64_t action, const float (&sel)[A], const float (&nxt)[A], float ret, float discount,
                                   float y, float weight, bool weighted, const TdParams& p) {
#pragma clang fp contract(off)
    TdSample<A> o;
    o.loss = o.priority = o.y = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) o.grad[a] = 0.0f;
#pragma unroll
    for (int k = 0; k < TD_STATS; ++k) o.u[k] = 0.0;
    bool bad = action < 0 || action >= A;
    float qa = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) qa = action == a ? q[a] : qa;       // a compare per unrolled a: no register array is indexed by a variable
    bad |= !(fabsf(qa) < INFINITY);
    double yv;
    if (NEXT) {
        float best = sel[0], qn = nxt[0];                            // qn: nxt[a_star], carried along with the choice
#pragma unroll
        for (int a = 1; a < A; ++a) {
            const float s = sel[a], n = nxt[a];                      // read before the choice: values are chosen below, never addresses
            const bool wins = s > best;                              // a NaN never wins; ties keep the lower index
            best = wins ? s : best;
            qn = wins ? n : qn;
        }
        bad |= !(fabsf(ret) < INFINITY) || !(fabsf(discount) < INFINITY) || discount < 0.0f || !(fabsf(qn) < INFINITY);
        yv = (double)ret + (double)discount * (double)qn;
    } else {
        bad |= !(fabsf(y) < INFINITY);
        yv = (double)y;
    }
    if (weighted) bad |= !(fabsf(weight) < INFINITY) || weight < 0.0f;
    o.bad = bad;
    if (bad) return o;
    const double td = (double)qa - yv;
    const double ab = fabs(td);
    double L, g;
    bool lin = false;
    if (p.delta == 0.0) {
        L = td * td;
        g = 2.0 * td;
    } else {
        lin = ab > p.delta;
        L = lin ? p.delta * (ab - 0.5 * p.delta) : 0.5 * (td * td);
        g = lin ? (td < 0.0 ? -p.delta : p.delta) : td;
    }
    const double w = weighted ? (double)weight : 1.0;
    const double total = w * L;
    o.loss = (float)L;
    o.priority = (float)ab;
    o.y = (float)yv;
    const float ga = (float)(p.scale * (w * g));
#pragma unroll
    for (int a = 0; a < A; ++a) o.grad[a] = action == a ? ga : 0.0f;
    o.u[TD_TOTAL] = total;
    o.u[TD_LOSS] = L;
    o.u[TD_ABS] = ab;
    o.u[TD_Q] = (double)qa;
    o.u[TD_Y] = yv;
    o.u[TD_LINEAR] = lin ? 1.0 : 0.0;
    o.u[TD_GOOD] = 1.0;
    o.u[TD_WEIGHT] = w;
    return o;
}

// The second stage of the reduction for one of the eight sums, as the second kernel's lane j runs its first half: partials[j],
// partials[j + 64], ... of column k added in increasing order from 0.0 (W rows of TD_STATS doubles).
SNAC_SPEC_FN double td_lane_sum(const double* partials, long long W, int j, int k) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (long long w = j; w < W; w += 64) s = s + partials[w * TD_STATS + k];
    return s;
}

}  // namespace snac_spec
