// ppo_host.cpp -- the per-sample function k_ppo_loss runs (snac_amd/csrc/ppo_rule.h), compiled for the host as it stands, with a C++
// restatement of both stages of the batch reduction: tests/test_ppo_loss_host.py builds this file into a shared object with the system
// compiler and -ffp-contract=off and compares every output's bytes with the numpy statement of the rule.  The loops below are
// k_ppo_loss's and k_ppo_reduce's bodies with the lane a loop index; snac_ppo_loss's conventions for NULL pointers hold.
// With -DPPO_HOST_MAIN the file is a program: one case with actions out of range, for a run under the host sanitizers.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ppo_rule.h"

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

template <int A, bool CLIP_VF>
int run(int32_t B, const float* logits, const int64_t* action, const float* logp_old, const float* adv, const float* value, const float* value_old,
        const float* ret, const PpoParams& p, float* loss, float* grad_logits, float* grad_value, double* stats, float* mean_loss, double* partials) {
    int bad_rows = 0;
    const long long W = ((long long)B + 63) / 64;
    for (long long w = 0; w < W; ++w) {
        double u[PPO_STATS][64];
        for (int j = 0; j < 64; ++j) {
            const long long i = w * 64 + j;
            for (int k = 0; k < PPO_STATS; ++k) u[k][j] = 0.0;
            if (i >= B) continue;
            const size_t at = (size_t)i * A;
            float l[A];
            for (int a = 0; a < A; ++a) l[a] = logits[at + a];
            const PpoSample<A> o = ppo_sample<A, CLIP_VF>(l, action[i], logp_old[i], adv[i], value[i], CLIP_VF ? value_old[i] : 0.0f, ret[i], p);
            bad_rows += o.bad;
            if (loss) loss[i] = o.loss;
            if (grad_value) grad_value[i] = o.grad_value;
            if (grad_logits)
                for (int a = 0; a < A; ++a) grad_logits[at + a] = o.grad[a];
            for (int k = 0; k < PPO_STATS; ++k) u[k][j] = o.u[k];
        }
        if (stats)
            for (int k = 0; k < PPO_STATS; ++k) partials[w * PPO_STATS + k] = butterfly(u[k]);
    }
    if (stats) {
        for (int k = 0; k < PPO_STATS; ++k) {
            double t[64];
            for (int j = 0; j < 64; ++j) t[j] = ppo_lane_sum(partials, W, j, k);
            const double s = butterfly(t);
            stats[k] = (k == PPO_GOOD || k == PPO_CLAMPED) ? s : s / (double)B;
        }
        if (mean_loss) mean_loss[0] = (float)stats[PPO_TOTAL];
    }
    return bad_rows;
}

}  // namespace

// -> the number of bad samples, or -1 for an unsupported num_actions
extern "C" int ppo_host(int32_t B, int32_t num_actions, const float* logits, const int64_t* action, const float* logp_old, const float* adv,
                        const float* value, const float* value_old, const float* ret, double clip, double clip_vf, double vf_coef, double ent_coef,
                        double scale, float* loss, float* grad_logits, float* grad_value, double* stats, float* mean_loss, double* partials) {
    const PpoParams p{clip, 1.0 - clip, 1.0 + clip, clip_vf, vf_coef, ent_coef, scale};
#define PPO_HOST_RUN(A)                                                                                                                     \
    return clip_vf >= 0.0 ? run<A, true>(B, logits, action, logp_old, adv, value, value_old, ret, p, loss, grad_logits, grad_value, stats, \
                                         mean_loss, partials)                                                                              \
                          : run<A, false>(B, logits, action, logp_old, adv, value, value_old, ret, p, loss, grad_logits, grad_value, stats, \
                                          mean_loss, partials)
    switch (num_actions) {
        case 3: PPO_HOST_RUN(3);
        case 5: PPO_HOST_RUN(5);
        case 8: PPO_HOST_RUN(8);
        default: return -1;
    }
#undef PPO_HOST_RUN
}

#ifdef PPO_HOST_MAIN
#include <cstdio>

// One case per action count whose actions run from -2 to A + 1 and beyond (and the int64 extremes), through ragged waves and a second
// stage of more than 64 partials, in exactly sized heap arrays: an action that indexed anything, or a lane past B that wrote, shows
// under -fsanitize=address,undefined.  Prints the counts; exit status 1 if a count is off.
int main() {
    int status = 0;
    for (int A : {3, 5, 8}) {
        for (int32_t B : {1, 65, 4097}) {
            const long long W = ((long long)B + 63) / 64;
            std::vector<float> logits((size_t)B * A), logp(B), adv(B), value(B), value_old(B), ret(B), loss(B), gl((size_t)B * A), gv(B);
            std::vector<int64_t> action(B);
            std::vector<double> stats(PPO_STATS), partials((size_t)W * PPO_STATS);
            int want_bad = 0;
            for (int32_t i = 0; i < B; ++i) {
                for (int a = 0; a < A; ++a) logits[(size_t)i * A + a] = 0.25f * (float)((i * 7 + a * 3) % 11) - 1.0f;
                const int64_t special[4] = {INT64_MIN, INT64_MAX, (int64_t)1 << 32, -((int64_t)1 << 32)};
                action[i] = i % 13 == 12 ? special[(i / 13) % 4] : (int64_t)(i % (A + 4)) - 2;      // -2 .. A + 1
                want_bad += action[i] < 0 || action[i] >= A;
                logp[i] = -1.0f - 0.01f * (float)(i % 50);
                adv[i] = (i % 2 ? 1.0f : -1.0f) * (1.0f + (float)(i % 5));
                value[i] = 0.1f * (float)(i % 17);
                value_old[i] = value[i] + 0.05f * (float)(i % 9 - 4);
                ret[i] = 0.3f * (float)(i % 7);
            }
            for (double clip_vf : {-1.0, 0.2}) {
                float mean = 0.0f;
                const int bad = ppo_host(B, A, logits.data(), action.data(), logp.data(), adv.data(), value.data(), clip_vf >= 0 ? value_old.data() : nullptr,
                                         ret.data(), 0.2, clip_vf, 0.5, 0.01, 1.0 / B, loss.data(), gl.data(), gv.data(), stats.data(), &mean, partials.data());
                std::printf("A %d B %d clip_vf %g: bad %d (want %d), good %.0f, mean loss %.9g\n", A, (int)B, clip_vf, bad, want_bad, stats[PPO_GOOD], (double)mean);
                if (bad != want_bad || stats[PPO_GOOD] != (double)(B - want_bad)) status = 1;
            }
        }
    }
    return status;
}
#endif
