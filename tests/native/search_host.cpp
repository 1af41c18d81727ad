// search_host.cpp -- the per-sample function k_search_loss runs (snac_amd/csrc/search_rule.h), compiled for the host as it stands, with a
// C++ restatement of both stages of the batch reduction: tests/test_search_loss_host.py builds this file into a shared object with the
// system compiler and -ffp-contract=off and compares every output's bytes with the numpy statement of the rule.  The loops below are
// k_search_loss's and k_search_reduce's bodies with the lane a loop index; snac_search_loss's conventions for NULL pointers hold.
// With -DSEARCH_HOST_MAIN the file is a program: cases with masked, far and bad rows, for a run under the host sanitizers.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "search_rule.h"

namespace {

using namespace snac_spec;

// the xor butterfly over 64 values: every j of a step together
double butterfly(const double* v) {
    double u[64], t[64];
    for (int j = 0; j < 64; ++j) u[j] = v[j];
    for (int off = 32; off >= 1; off >>= 1) {
        for (int j = 0; j < 64; ++j) t[j] = u[j] + u[j ^ off];
        for (int j = 0; j < 64; ++j) u[j] = t[j];
    }
    return u[0];
}

template <int A>
int run(int32_t B, const float* logits, const float* value, const float* pi, const float* z, const float* weight, const SearchParams& p, float* loss,
        float* priority, float* grad_logits, float* grad_value, double* stats, float* mean_loss, double* partials) {
    int bad_rows = 0;
    const long long W = ((long long)B + 63) / 64;
    for (long long w = 0; w < W; ++w) {
        double u[SEARCH_STATS][64];
        for (int j = 0; j < 64; ++j) {
            const long long i = w * 64 + j;
            for (int k = 0; k < SEARCH_STATS; ++k) u[k][j] = 0.0;
            if (i >= B) continue;
            const size_t at = (size_t)i * A;
            float l[A], t[A];
            for (int a = 0; a < A; ++a) {
                l[a] = logits[at + a];
                t[a] = pi[at + a];
            }
            const SearchSample<A> o = search_sample<A>(l, value[i], t, z[i], weight ? weight[i] : 1.0f, weight != nullptr, p);
            bad_rows += o.bad;
            if (loss) loss[i] = o.loss;
            if (priority) priority[i] = o.priority;
            if (grad_value) grad_value[i] = o.grad_value;
            if (grad_logits)
                for (int a = 0; a < A; ++a) grad_logits[at + a] = o.grad[a];
            for (int k = 0; k < SEARCH_STATS; ++k) u[k][j] = o.u[k];
        }
        if (stats)
            for (int k = 0; k < SEARCH_STATS; ++k) partials[w * SEARCH_STATS + k] = butterfly(u[k]);
    }
    if (stats) {
        for (int k = 0; k < SEARCH_STATS; ++k) {
            double t[64];
            for (int j = 0; j < 64; ++j) t[j] = search_lane_sum(partials, W, j, k);
            const double s = butterfly(t);
            stats[k] = k == SEARCH_GOOD ? s : s / (double)B;
        }
        if (mean_loss) mean_loss[0] = (float)stats[SEARCH_TOTAL];
    }
    return bad_rows;
}

}  // namespace

// -> the number of bad samples, or -1 for an unsupported num_actions
extern "C" int search_host(int32_t B, int32_t num_actions, const float* logits, const float* value, const float* pi, const float* z,
                           const float* weight, double vf_coef, double delta, double scale, float* loss, float* priority, float* grad_logits,
                           float* grad_value, double* stats, float* mean_loss, double* partials) {
    const SearchParams p{vf_coef, delta, scale};
    switch (num_actions) {
        case 3: return run<3>(B, logits, value, pi, z, weight, p, loss, priority, grad_logits, grad_value, stats, mean_loss, partials);
        case 5: return run<5>(B, logits, value, pi, z, weight, p, loss, priority, grad_logits, grad_value, stats, mean_loss, partials);
        case 8: return run<8>(B, logits, value, pi, z, weight, p, loss, priority, grad_logits, grad_value, stats, mean_loss, partials);
        default: return -1;
    }
}

#ifdef SEARCH_HOST_MAIN
#include <cstdio>

// One case per action count with masked actions, logits far below the largest, targets on masked actions, NaNs and infinities in every
// input, through ragged waves and a second stage of more than 64 partials, in exactly sized heap arrays: a lane past B that wrote, or
// anything indexed past a row, shows under -fsanitize=address,undefined.  Prints the counts; exit status 1 if a count is off.
int main() {
    int status = 0;
    for (int A : {3, 5, 8}) {
        for (int32_t B : {1, 65, 4097}) {
            const long long W = ((long long)B + 63) / 64;
            std::vector<float> l((size_t)B * A), pi((size_t)B * A), value(B), z(B), weight(B), loss(B), prio(B), gl((size_t)B * A), gv(B);
            std::vector<double> stats(SEARCH_STATS), partials((size_t)W * SEARCH_STATS);
            int want_bad = 0, want_bad_w = 0;
            for (int32_t i = 0; i < B; ++i) {
                for (int a = 0; a < A; ++a) {
                    l[(size_t)i * A + a] = 0.25f * (float)((i * 7 + a * 3) % 11) - 1.0f;
                    pi[(size_t)i * A + a] = (float)(1 + (i * 5 + a * 7) % 13) / 64.0f;
                }
                value[i] = 0.3f * (float)(i % 7) - 1.0f;
                z[i] = 0.1f * (float)(i % 17) - 0.5f;
                weight[i] = 0.1f * (float)(1 + i % 10);
                const int last = A - 1, mid = i % A;
                bool bad = false, bad_w = false;
                switch (i % 13) {
                    case 1: l[(size_t)i * A + mid] = -INFINITY; pi[(size_t)i * A + mid] = 0.0f; break;      // masked, fine
                    case 2: l[(size_t)i * A + mid] = -INFINITY; bad = true; break;                          // a target on a masked action
                    case 3: l[(size_t)i * A + last] = -300.0f; break;                                       // far below the largest: e == 0, fine
                    case 4: l[(size_t)i * A] = NAN; bad = true; break;
                    case 5: l[(size_t)i * A + last] = INFINITY; bad = true; break;
                    case 6: pi[(size_t)i * A + mid] = -0.5f; bad = true; break;
                    case 7: pi[(size_t)i * A + mid] = -0.0f; break;
                    case 8: pi[(size_t)i * A + last] = NAN; bad = true; break;
                    case 9: value[i] = INFINITY; bad = true; break;
                    case 10: z[i] = NAN; bad = true; break;
                    case 11: weight[i] = i % 2 ? -0.5f : NAN; bad_w = true; break;
                    case 12: for (int a = 0; a < A; ++a) l[(size_t)i * A + a] = -INFINITY; bad = true; break;
                    default: break;
                }
                want_bad += bad;
                want_bad_w += bad || bad_w;
            }
            for (int weighted = 0; weighted < 2; ++weighted) {
                for (double delta : {0.0, 1.0}) {
                    float mean = 0.0f;
                    const int bad = search_host(B, A, l.data(), value.data(), pi.data(), z.data(), weighted ? weight.data() : nullptr, 0.5, delta, 1.0 / B,
                                                loss.data(), prio.data(), gl.data(), gv.data(), stats.data(), &mean, partials.data());
                    const int want = weighted ? want_bad_w : want_bad;
                    std::printf("A %d B %d weighted %d delta %g: bad %d (want %d), good %.0f, mean loss %.9g\n", A, (int)B, weighted, delta, bad, want,
                                stats[SEARCH_GOOD], (double)mean);
                    if (bad != want || stats[SEARCH_GOOD] != (double)(B - want) || !(std::fabs(mean) < INFINITY)) status = 1;
                }
            }
        }
    }
    return status;
}
#endif
