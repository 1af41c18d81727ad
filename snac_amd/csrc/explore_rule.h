// explore_rule.h -- the rules of include/snac_hip.h, "Exploration noise", once, for k_explore.hip, for k_uct_pick (k_uct_play.hip) and for a
// host compiler as it stands (tests/native/explore_host.cpp, with -ffp-contract=off): the log of a Gamma(alpha, 1) draw by a counted
// rejection loop, the pieces of the Dirichlet root noise and of the Gumbel scores per slot (b, a), and the move drawn from a root's visit
// counts -- greedy, in proportion to the counts, or to their power 1 / T.  The counter RNG is not here: a caller hands the words in, as a
// callable (j, k) -> word for the Gamma draw and as plain words elsewhere.  Every float64 operation below is one operation of the rule,
// rounded on its own; LOGP is spec_math.h's spec_log on its whole domain, the softmax softmax_rule.h's.
#pragma once
#include <cmath>
#include <cstdint>

#include "softmax_rule.h"

namespace snac_spec {

constexpr uint32_t DIRICHLET_STREAM = 6, GUMBEL_STREAM = 7;          // the counter RNG's streams of the two noises
constexpr int EXPLORE_GROUP = 8;                                     // slots per tree in the keys: (env_id_base + b) * 8 + a for every A
constexpr int EXPLORE_MAX_ATTEMPTS = 32;

// U of the header: the word's cell of (0, 1), at its middle; exact
SNAC_SPEC_FN double unit_of(uint32_t w) {
#pragma clang fp contract(off)
    return ((double)w + 0.5) * 0x1p-32;
}

// the counter of attempt j's word k at move t: 32-bit wrap-around
SNAC_SPEC_FN uint32_t dirichlet_counter(uint32_t t, int j, int k) { return t * 128u + 4u * (uint32_t)j + (uint32_t)k; }

// What a call fixes for every slot; the host computes d, c and logd once (gamma_params below) and the device takes no square root.
struct GammaParams {
    double alpha, d, c, logd;
    int32_t attempts;
    bool boost;
};

SNAC_SPEC_FN GammaParams gamma_params(double alpha, int32_t attempts) {
#pragma clang fp contract(off)
    GammaParams g;
    g.alpha = alpha;
    g.boost = alpha < 1.0;
    const double a1 = g.boost ? alpha + 1.0 : alpha;
    g.d = a1 - 1.0 / 3.0;
    g.c = 1.0 / sqrt(9.0 * g.d);
    g.logd = spec_log(g.d);
    g.attempts = attempts;
    return g;
}

// log of a Gamma(alpha, 1) draw: Marsaglia and Tsang's squeeze-free test on a ratio-of-uniforms normal, at most g.attempts attempts;
// word(j, k): word k of attempt j.  accepted: whether an attempt was (else the draw is d, the mode's neighbour).
template <class W>
SNAC_SPEC_FN double gamma_log(const GammaParams& g, W word, bool& accepted) {
#pragma clang fp contract(off)
    double lv = 0.0;
    bool got = false;
    for (int j = 0; j < g.attempts && !got; ++j) {                   // a counted loop: a lane leaves it at its first accepted attempt
        const double u1 = unit_of(word(j, 0)), u2 = unit_of(word(j, 1)), u3 = unit_of(word(j, 2));
        const double x = (1.7156 * (u2 - 0.5)) / u1;
        const double x2 = x * x;
        const bool normal = x2 <= -4.0 * spec_log(u1);
        const double s = 1.0 + g.c * x;
        const double v = (s * s) * s;
        const bool positive = v > 0.0;
        const double lt = spec_log(positive ? v : 1.0);
        const double rhs = ((0.5 * x2 + g.d) - g.d * v) + g.d * lt;
        if (normal && positive && spec_log(u3) < rhs) {
            lv = lt;
            got = true;
        }
    }
    accepted = got;
    double lg = got ? g.logd + lv : g.logd;
    if (g.boost) lg = lg + spec_log(unit_of(word(0, 3))) / g.alpha;
    return lg;
}

// ---- Dirichlet root noise, per slot and per row
// a row of root priors is bad: some p_a a NaN, infinite or negative, or no p_a > 0 (-0.0 is a zero)
template <int A>
SNAC_SPEC_FN bool priors_bad(const float (&p)[A]) {
    bool bad = false, any = false;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        bad |= !(fabsf(p[a]) < INFINITY) || p[a] < 0.0f;
        any |= p[a] > 0.0f;
    }
    return bad || !any;
}

// l_a: the float32 log of the slot's Gamma draw on the support, -inf off it
template <class W>
SNAC_SPEC_FN float dirichlet_logit(float p, const GammaParams& g, W word, bool& accepted) {
    accepted = true;
    if (!(p > 0.0f)) return -INFINITY;
    return (float)gamma_log(g, word, accepted);
}

// S of softmax_rule.h's sums alone: e_0 + ... + e_{A-1} in index order from 0.0
template <int A>
SNAC_SPEC_FN double terms_sum(const double (&e)[A]) {
#pragma clang fp contract(off)
    double S = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) S = S + e[a];
    return S;
}

// p'_a on the support: om = 1 - eps, computed once per call
SNAC_SPEC_FN float dirichlet_mix(float p, double e, double S, double om, double eps) {
#pragma clang fp contract(off)
    const double eta = e / S;
    const double keep = om * (double)p;
    const double add = eps * eta;
    return (float)(keep + add);
}

// ---- Gumbel scores, per slot: log prior plus (noisy) a Gumbel(0, 1) draw from the slot's word
SNAC_SPEC_FN float gumbel_score(float p, bool noisy, uint32_t w) {
#pragma clang fp contract(off)
    if (p == 0.0f) return -INFINITY;
    if (!(p > 0.0f) || !(p < INFINITY)) return NAN;                  // a NaN, a negative or an infinite prior
    double n = 0.0;
    if (noisy) n = -spec_log(-spec_log(unit_of(w)));
    return (float)(spec_log((double)p) + n);
}

// ---- The move from a root's counts
// the lowest a with the largest count
template <int A>
SNAC_SPEC_FN int pick_greedy(const uint32_t (&n)[A]) {
    int act = 0;
    uint32_t best = n[0];
#pragma unroll
    for (int a = 1; a < A; ++a)
        if (n[a] > best) { best = n[a]; act = a; }
    return act;
}

// in proportion to integer weights: u = (w * total) >> 32 without leaving 64 bits (total < 2^35), the lowest a whose running sum passes u
// (u < total: there is one)
template <int A, typename T>
SNAC_SPEC_FN int pick_weighted(const T (&wt)[A], uint64_t total, uint32_t w) {
    const uint64_t u = (uint64_t)w * (total >> 32) + (((uint64_t)w * (total & 0xFFFFFFFFull)) >> 32);
    uint64_t cum = 0;
    bool found = false;
    int act = A - 1;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        cum += wt[a];
        if (!found && cum > u) { act = a; found = true; }
    }
    return act;
}

// the weights of a temperature T that is neither 0 nor 1: N_a^(1 / T) relative to the largest count, in units of 2^-28; their sum
template <int A>
SNAC_SPEC_FN uint64_t temp_weights(const uint32_t (&n)[A], double T, uint64_t (&wt)[A]) {
#pragma clang fp contract(off)
    const double r = 1.0 / T;
    uint32_t nmax = n[0];
#pragma unroll
    for (int a = 1; a < A; ++a) nmax = n[a] > nmax ? n[a] : nmax;
    const double lmax = spec_log((double)(nmax ? nmax : 1u));
    uint64_t total = 0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        uint64_t w = 0;
        if (n[a] == nmax) w = n[a] ? 1ull << 28 : 0;                 // exactly 2^28, also where r is infinite
        else if (n[a] > 0) w = (uint64_t)floor(spec_exp((spec_log((double)n[a]) - lmax) * r) * 0x1p28);
        wt[a] = w;
        total += w;
    }
    return total;
}

// The move of snac_explore_pick_moves_temp for a root with counts n (their sum `total`): greedy where asked, or at a NaN or T <= 0; the
// integer rule at T == 1; else by temp_weights.  w: the tree's stream-3 word.
template <int A>
SNAC_SPEC_FN int temp_move(const uint32_t (&n)[A], uint64_t total, bool greedy, double T, uint32_t w) {
    if (total == 0) return 0;
    if (greedy || !(T > 0.0)) return pick_greedy<A>(n);
    if (T == 1.0) return pick_weighted<A>(n, total, w);
    uint64_t wt[A];
    const uint64_t sum = temp_weights<A>(n, T, wt);
    return pick_weighted<A>(wt, sum, w);
}

}  // namespace snac_spec
