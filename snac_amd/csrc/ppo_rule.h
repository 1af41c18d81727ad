// ppo_rule.h -- the per-sample rule of include/snac_hip.h, "PPO loss (the reference's script/PPO)", as one function that k_ppo.hip runs
// per lane and that a host compiler can compile as it stands (tests/native/ppo_host.cpp, with -ffp-contract=off): PPO2's clipped
// surrogate, its clipped value loss and the entropy bonus of one sample, the closed-form gradient with respect to the logits and to the
// value, and the sample's eight contributions to the batch statistics.  Every float64 operation below is one operation of the rule,
// rounded on its own; sums run in index order from 0.0.  The softmax part is softmax_rule.h's.
#pragma once
#include <cmath>
#include <cstdint>

#include "softmax_rule.h"

#define SNAC_PPO_LOGRATIO_MAX 20.0                                    // |lp - logp_old| beyond it: the ratio is taken at the bound, no gradient

namespace snac_spec {

// the places of a sample's contributions u[0..8), which are the places of stats[0..8) of snac_ppo_loss
enum { PPO_TOTAL = 0, PPO_LPI = 1, PPO_LV = 2, PPO_H = 3, PPO_KL = 4, PPO_CLIPPED = 5, PPO_GOOD = 6, PPO_CLAMPED = 7, PPO_STATS = 8 };

struct PpoParams {                                                   // lo = 1.0 - clip and hi = 1.0 + clip, computed once by the caller
    double clip, lo, hi, clip_vf, vf_coef, ent_coef, scale;
};

template <int A>
struct PpoSample {                                                   // what one sample gives; bad: it counts in bad_rows and the rest is zero
    float loss, grad_value;
    float grad[A];
    double u[PPO_STATS];
    bool bad;
};

// One sample.  CLIP_VF: the value function is clipped (clip_vf >= 0) and value_old is read and checked -- else it is never looked at.
// All arrays are indexed by unrolled constants; the taken action's terms are picked by compares.
template <int A, bool CLIP_VF>
SNAC_SPEC_FN PpoSample<A> ppo_sample(const float (&l)[A], int64_t action, float logp_old, float adv, float value, float value_old, float ret,
                                     const PpoParams& p) {
#pragma clang fp contract(off)
    PpoSample<A> o;
    o.loss = o.grad_value = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) o.grad[a] = 0.0f;
#pragma unroll
    for (int k = 0; k < PPO_STATS; ++k) o.u[k] = 0.0;
    float m;
    bool bad = softmax_scan(l, m);
    bad |= action < 0 || action >= A;
    bad |= !(fabsf(logp_old) < INFINITY) || !(fabsf(adv) < INFINITY) || !(fabsf(value) < INFINITY) || !(fabsf(ret) < INFINITY);
    if (CLIP_VF) bad |= !(fabsf(value_old) < INFINITY);
    o.bad = bad;
    if (bad) return o;
    double x[A], e[A];
    softmax_terms(l, m, x, e);
    const SoftmaxSums sm = softmax_sums(x, e);
    const double S = sm.S, L = sm.L, H = softmax_entropy(sm);
    double pi[A], lpa[A];
    double lp = 0.0, e_act = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        pi[a] = e[a] / S;
        lpa[a] = x[a] - L;
        const bool taken = action == a;                              // a compare per unrolled a: no register array is indexed by a variable
        lp = taken ? lpa[a] : lp;
        e_act = taken ? e[a] : e_act;
    }
    if (e_act == 0.0) {                                              // the taken action has no weight: its log-probability is -inf
        o.bad = true;
        return o;
    }
    const double d = lp - (double)logp_old;
    const bool clamped = fabs(d) > SNAC_PPO_LOGRATIO_MAX;
    const double dc = d < -SNAC_PPO_LOGRATIO_MAX ? -SNAC_PPO_LOGRATIO_MAX : d > SNAC_PPO_LOGRATIO_MAX ? SNAC_PPO_LOGRATIO_MAX : d;
    const double r = dc <= 0.0 ? spec_exp(dc) : 1.0 / spec_exp(-dc); // EXP keeps its stated domain x <= 0
    const double rc = r < p.lo ? p.lo : r > p.hi ? p.hi : r;
    const double ad = (double)adv;
    const double s1 = r * ad, s2 = rc * ad;
    const bool second = s2 < s1;
    const double Lpi = -(second ? s2 : s1);
    const double g = (!second && !clamped) ? -(ad * r) : 0.0;       // dLpi / dlp
    const double dv = (double)value - (double)ret;
    double Lv, gv;
    if (CLIP_VF) {
        const double u = (double)value - (double)value_old;
        const double uc = u < -p.clip_vf ? -p.clip_vf : u > p.clip_vf ? p.clip_vf : u;
        const double dc2 = ((double)value_old + uc) - (double)ret;
        const double q1 = dv * dv, q2 = dc2 * dc2;
        if (q2 > q1) {
            Lv = 0.5 * q2;
            gv = u == uc ? dc2 : 0.0;
        } else {
            Lv = 0.5 * q1;
            gv = dv;
        }
    } else {
        Lv = 0.5 * (dv * dv);
        gv = dv;
    }
    const double kl = 0.5 * (dc * dc);
    const bool clipped = fabs(r - 1.0) > p.clip;
    const double total = (Lpi + p.vf_coef * Lv) - p.ent_coef * H;
    o.loss = (float)total;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const double onehot = action == a ? 1.0 : 0.0;
        o.grad[a] = e[a] != 0.0 ? (float)(p.scale * (g * (onehot - pi[a]) + p.ent_coef * (pi[a] * (lpa[a] + H)))) : 0.0f;
    }
    o.grad_value = (float)(p.scale * (p.vf_coef * gv));
    o.u[PPO_TOTAL] = total;
    o.u[PPO_LPI] = Lpi;
    o.u[PPO_LV] = Lv;
    o.u[PPO_H] = H;
    o.u[PPO_KL] = kl;
    o.u[PPO_CLIPPED] = clipped ? 1.0 : 0.0;
    o.u[PPO_GOOD] = 1.0;
    o.u[PPO_CLAMPED] = clamped ? 1.0 : 0.0;
    return o;
}

// The second stage of the reduction for one of the eight sums, as k_ppo_reduce's lane j runs its first half: partials[j], partials[j + 64],
// ... of column k added in increasing order from 0.0 (W rows of PPO_STATS doubles).
SNAC_SPEC_FN double ppo_lane_sum(const double* partials, long long W, int j, int k) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (long long w = j; w < W; w += 64) s = s + partials[w * PPO_STATS + k];
    return s;
}

}  // namespace snac_spec
