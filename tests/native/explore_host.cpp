// explore_host.cpp -- the rules k_root_dirichlet, k_gumbel_scores and k_uct_pick<A, true> run (snac_amd/csrc/explore_rule.h), compiled for
// the host as they stand: tests/test_explore_host.py builds this file into a shared object with the system compiler and -ffp-contract=off
// and compares every output's bytes with the numpy statement of the rules.  The loops below are the kernels' bodies with the slot
// (b, a) a pair of loop indices and a lane read an array read; the counter RNG of include/snac_hip.h is restated here, since the
// kernels' own is device code.  With -DEXPLORE_HOST_MAIN the file is a program: cases with zeros, bad rows of each sort and masks in
// exactly sized heap arrays, for a run under the host sanitizers.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "explore_rule.h"

namespace {

using namespace snac_spec;

uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
uint32_t stream_key(uint64_t seed, uint32_t stream) { return mix32((uint32_t)seed ^ mix32((uint32_t)(seed >> 32) + 0x9E3779B9u * (stream + 1u))); }
struct Keys { uint32_t e0, e1; };
Keys env_keys(uint32_t key, uint64_t env) {
    const uint32_t elo = (uint32_t)env, ehi = (uint32_t)(env >> 32);
    return {mix32(key ^ mix32(elo + 0x85EBCA6Bu * ehi + 0x1B873593u)), mix32((key + 0x27D4EB2Fu) ^ mix32((elo ^ 0x165667B1u) + 0xC2B2AE35u * ehi))};
}
uint32_t rng_word(Keys k, uint32_t t) { return mix32(mix32(k.e0 ^ (0x9E3779B9u * t)) + k.e1); }
uint64_t slot_env(int64_t base, int32_t b, int a) { return (uint64_t)(base + b) * (uint64_t)EXPLORE_GROUP + (uint64_t)a; }

template <int A>
int dirichlet(uint64_t seed, int64_t base, int32_t B, uint32_t t, float* priors, const uint8_t* mask, double alpha, double eps, int32_t attempts,
              uint8_t* accepted) {
#pragma clang fp contract(off)
    const GammaParams g = gamma_params(alpha, attempts);
    const double om = 1.0 - eps;
    const uint32_t key = stream_key(seed, DIRICHLET_STREAM);
    int bad_rows = 0;
    for (int32_t b = 0; b < B; ++b) {
        if (mask && mask[b] == 0) continue;
        float p[A], l[A];
        for (int a = 0; a < A; ++a) p[a] = priors[(size_t)b * A + a];
        if (priors_bad<A>(p)) { bad_rows += 1; continue; }
        for (int a = 0; a < A; ++a) {
            const Keys k = env_keys(key, slot_env(base, b, a));
            bool acc = true;
            l[a] = dirichlet_logit(p[a], g, [k, t](int j, int i) { return rng_word(k, dirichlet_counter(t, j, i)); }, acc);
            if (accepted) accepted[(size_t)b * A + a] = acc ? 1 : 0;
        }
        float m;
        softmax_scan<A>(l, m);
        double e[A];
        for (int a = 0; a < A; ++a) {                                // a lane's own term
            const float own[1] = {l[a]};
            double x1[1], e1[1];
            softmax_terms<1>(own, m, x1, e1);
            e[a] = e1[0];
        }
        const double S = terms_sum<A>(e);
        for (int a = 0; a < A; ++a)
            if (p[a] > 0.0f) priors[(size_t)b * A + a] = dirichlet_mix(p[a], e[a], S, om, eps);
    }
    return bad_rows;
}

template <int A>
void temp(uint64_t seed, int64_t base, int32_t B, uint32_t t, const int32_t* counts, const uint8_t* greedy, const float* temperature, double T1,
          int8_t* action) {
    const uint32_t key = stream_key(seed, 3);
    for (int32_t b = 0; b < B; ++b) {
        uint32_t n[A];
        uint64_t total = 0;
        for (int a = 0; a < A; ++a) {
            const int32_t c = counts[(size_t)b * A + a];
            n[a] = (uint32_t)(c > 0 ? c : 0);
            total += n[a];
        }
        const bool gr = !greedy || greedy[b] != 0;
        const uint32_t w = gr ? 0u : rng_word(env_keys(key, (uint64_t)(base + b)), t);
        action[b] = (int8_t)temp_move<A>(n, total, gr, temperature ? (double)temperature[b] : T1, w);
    }
}

}  // namespace

// -> the number of bad rows, or -1 for an unsupported num_actions.  priors: [B][A], changed in place; accepted (may be NULL): [B][A], 1
// where the slot's Gamma draw was accepted within its attempts (or the slot drew nothing), written for the rows that drew
extern "C" int explore_dirichlet_host(uint64_t seed, int64_t base, int32_t B, int32_t A, uint32_t t, float* priors, const uint8_t* mask, double alpha,
                                      double eps, int32_t attempts, uint8_t* accepted) {
    switch (A) {
        case 3: return dirichlet<3>(seed, base, B, t, priors, mask, alpha, eps, attempts, accepted);
        case 5: return dirichlet<5>(seed, base, B, t, priors, mask, alpha, eps, attempts, accepted);
        case 8: return dirichlet<8>(seed, base, B, t, priors, mask, alpha, eps, attempts, accepted);
        default: return -1;
    }
}

extern "C" int explore_gumbel_host(uint64_t seed, int64_t base, int32_t B, int32_t A, uint32_t t, const float* priors, const uint8_t* noisy,
                                   float* scores) {
    if (A != 3 && A != 5 && A != 8) return -1;
    const uint32_t key = stream_key(seed, GUMBEL_STREAM);
    for (int32_t b = 0; b < B; ++b)
        for (int a = 0; a < A; ++a) {
            const bool on = !noisy || noisy[b] != 0;
            const uint32_t w = on ? rng_word(env_keys(key, slot_env(base, b, a)), t) : 0u;
            scores[(size_t)b * A + a] = gumbel_score(priors[(size_t)b * A + a], on, w);
        }
    return 0;
}

extern "C" int explore_temp_host(uint64_t seed, int64_t base, int32_t B, int32_t A, uint32_t t, const int32_t* counts, const uint8_t* greedy,
                                 const float* temperature, double T1, int8_t* action) {
    switch (A) {
        case 3: temp<3>(seed, base, B, t, counts, greedy, temperature, T1, action); return 0;
        case 5: temp<5>(seed, base, B, t, counts, greedy, temperature, T1, action); return 0;
        case 8: temp<8>(seed, base, B, t, counts, greedy, temperature, T1, action); return 0;
        default: return -1;
    }
}

extern "C" void explore_logp_host(int64_t n, const double* s, double* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = spec_log(s[i]);
}

#ifdef EXPLORE_HOST_MAIN
#include <cstdio>

// Per action count and batch: priors with zeros, a bad row of each sort, a mask; every alpha's branch (boosted or not), one attempt and
// sixteen; the scores of the same priors; moves at every sort of temperature from counts with zeros and a count of 2^31 - 1.  Prints
// the counts; exit status 1 if one is off.
int main() {
    int status = 0;
    for (int A : {3, 5, 8}) {
        for (int32_t B : {1, 9, 257}) {
            std::vector<float> p((size_t)B * A), q, scores((size_t)B * A);
            std::vector<uint8_t> mask(B), acc((size_t)B * A);
            std::vector<int32_t> counts((size_t)B * A);
            std::vector<float> temps(B);
            std::vector<int8_t> action(B);
            int want_bad = 0;
            for (int32_t b = 0; b < B; ++b) {
                for (int a = 0; a < A; ++a) p[(size_t)b * A + a] = (float)(1 + (b * 5 + a * 7) % 13) / 64.0f;
                mask[b] = b % 4 != 3;
                float* r = &p[(size_t)b * A];
                bool bad = false;
                switch (b % 9) {
                    case 1: r[b % A] = 0.0f; break;
                    case 2: r[0] = NAN; bad = true; break;
                    case 3: r[A - 1] = INFINITY; bad = true; break;
                    case 4: r[b % A] = -0.25f; bad = true; break;
                    case 5: for (int a = 0; a < A; ++a) r[a] = 0.0f; bad = true; break;
                    case 6: r[b % A] = -0.0f; break;
                    default: break;
                }
                want_bad += bad && mask[b];
                for (int a = 0; a < A; ++a) counts[(size_t)b * A + a] = (b + a) % 3 == 0 ? 0 : (a == 1 && b % 5 == 0 ? 0x7FFFFFFF : 1 + (b * 3 + a) % 40);
                const float ts[] = {0.0f, 1.0f, 0.5f, 2.0f, INFINITY, NAN, -1.0f, 1e-30f};
                temps[b] = ts[b % 8];
            }
            for (double alpha : {0.03, 1.0, 2.5}) {
                for (int32_t attempts : {1, 16}) {
                    q = p;
                    const int bad = explore_dirichlet_host(7, 1000, B, A, (1u << 25) + 3u, q.data(), mask.data(), alpha, 0.25, attempts, acc.data());
                    std::printf("A %d B %d alpha %g attempts %d: bad %d (want %d)\n", A, (int)B, alpha, (int)attempts, bad, want_bad);
                    if (bad != want_bad) status = 1;
                }
            }
            explore_gumbel_host(7, 1000, B, A, 5, p.data(), mask.data(), scores.data());
            explore_temp_host(7, 1000, B, A, 5, counts.data(), nullptr, temps.data(), 1.0, action.data());
            explore_temp_host(7, 1000, B, A, 5, counts.data(), mask.data(), temps.data(), 1.0, action.data());
            explore_temp_host(7, 1000, B, A, 5, counts.data(), mask.data(), nullptr, 0.25, action.data());
            for (int32_t b = 0; b < B; ++b)
                if (action[b] < 0 || action[b] >= A) status = 1;
        }
    }
    return status;
}
#endif
