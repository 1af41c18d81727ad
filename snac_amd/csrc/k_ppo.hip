// k_ppo.hip -- snac_ppo_loss: PPO2's clipped loss of a minibatch, its gradient with respect to the logits and the value, and its
// statistics (the mean loss and its parts, the approximate KL, the clip fraction), in two launches on the caller's stream and in a fixed
// order of float64 additions.  include/snac_hip.h, "PPO loss (the reference's script/PPO)", has the rule; ppo_rule.h states it per
// sample, for the first kernel and for the host.
#include <cmath>
#include <cstddef>

#include "snac_units.h"
#include "batch_sum.h"
#include "ppo_rule.h"

static_assert(SNAC_PPO_STATS == snac_spec::PPO_STATS && snac_spec::PPO_STATS == snac_detail::BATCH_STATS, "the header's count of statistics is the rule's");

// k_ppo_loss: lane = sample, blocks of one wave, as k_soft_value: a lane reads its row of logits as A strided dword loads and its six
// scalars, all issued before the first use; a wave's rows are one contiguous span per input.  All arrays are indexed by unrolled
// constants (the taken action is picked by compares): registers only, no scratch, no LDS.  What is new is the end: the lanes past B and
// the bad lanes carry +0.0 in all eight contributions and stay in the wave, the wave adds each contribution over its 64 lanes by the xor
// butterfly of the header (u_j = u_j + u_{j ^ off}, off = 32 .. 1: every lane holds the same sum afterwards, since a + b == b + a bit for
// bit), and lane 0 writes the wave's row of partials.
// k_ppo_reduce: one wave.  Lane j adds rows j, j + 64, ... of the partials in increasing order from 0.0, then the same butterfly, the
// divisions by B, and lane 0 writes stats and mean_loss.  No atomics on floats, nothing waits for the host.  (batch_sum.h has wave_sum
// and the second kernel's body, for this unit and k_qloss.hip.)
namespace {

using namespace snac_detail;
using namespace snac_spec;

struct PpoArgs {
    int32_t B;
    const float* logits;
    const int64_t* action;
    const float* logp_old;
    const float* adv;
    const float* value;
    const float* value_old;
    const float* ret;
    PpoParams p;
    float* loss;
    float* grad_logits;
    float* grad_value;
    double* partials;
    int32_t* bad_rows;
};

template <int A, bool CLIP_VF>
__global__ __launch_bounds__(64) void k_ppo_loss(const PpoArgs g) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    const bool in = i < g.B;
    const size_t at = (size_t)(in ? i : 0) * A, is = (size_t)(in ? i : 0);      // a lane past B reads sample 0 and drops it
    float l[A];
#pragma unroll
    for (int a = 0; a < A; ++a) l[a] = g.logits[at + a];             // every load of the lane on its way before the first use
    const int64_t action = g.action[is];
    const float logp_old = g.logp_old[is], adv = g.adv[is], value = g.value[is], ret = g.ret[is];
    const float value_old = CLIP_VF ? g.value_old[is] : 0.0f;

    PpoSample<A> o = ppo_sample<A, CLIP_VF>(l, action, logp_old, adv, value, value_old, ret, g.p);
    if (in) {
        if (o.bad && g.bad_rows) atomicAdd(g.bad_rows, 1);
        if (g.loss) g.loss[i] = o.loss;
        if (g.grad_value) g.grad_value[i] = o.grad_value;
        if (g.grad_logits) {
#pragma unroll
            for (int a = 0; a < A; ++a) g.grad_logits[at + a] = o.grad[a];
        }
    }
    if (!g.partials) return;                                         // uniform: no statistics asked for
#pragma unroll
    for (int k = 0; k < PPO_STATS; ++k) {
        const double s = wave_sum(in ? o.u[k] : 0.0);                // every lane of the wave is here: none has returned
        if (threadIdx.x == 0) g.partials[(size_t)blockIdx.x * PPO_STATS + k] = s;
    }
}

__global__ __launch_bounds__(64) void k_ppo_reduce(const double* partials, long long W, int32_t B, double* stats, float* mean_loss) {
    reduce_partials<(1u << PPO_GOOD | 1u << PPO_CLAMPED)>(partials, W, B, stats, mean_loss);      // the two counts are not divided by B
}

}  // namespace

extern "C" int snac_ppo_loss(int32_t B, int32_t num_actions, const float* logits, const int64_t* action, const float* logp_old, const float* adv,
                             const float* value, const float* value_old, const float* ret, double clip, double clip_vf, double vf_coef, double ent_coef,
                             double scale, float* loss, float* grad_logits, float* grad_value, double* stats, float* mean_loss, double* partials,
                             int32_t* bad_rows, void* stream) {
    using namespace snac_detail;
    if (!logits) return fail(SNAC_ERR_ARG, "null logits");
    if (!action) return fail(SNAC_ERR_ARG, "null action");
    if (!logp_old || !adv || !value || !ret) return fail(SNAC_ERR_ARG, "logp_old, adv, value and ret are needed");
    if (B < 1) return fail(SNAC_ERR_ARG, "B must be >= 1");
    if (!std::isfinite(clip) || !(clip > 0.0)) return fail(SNAC_ERR_ARG, "clip must be finite and > 0");
    if (!std::isfinite(clip_vf)) return fail(SNAC_ERR_ARG, "clip_vf must be finite (negative: the value function is not clipped)");
    if (!std::isfinite(vf_coef)) return fail(SNAC_ERR_ARG, "vf_coef must be finite");
    if (!std::isfinite(ent_coef)) return fail(SNAC_ERR_ARG, "ent_coef must be finite");
    if (!std::isfinite(scale)) return fail(SNAC_ERR_ARG, "scale must be finite");
    const bool clip_v = clip_vf >= 0.0;
    if (clip_v && !value_old) return fail(SNAC_ERR_ARG, "value_old is needed when clip_vf >= 0");
    if (!clip_v && value_old) return fail(SNAC_ERR_ARG, "value_old belongs to clip_vf >= 0");
    if (stats && !partials) return fail(SNAC_ERR_ARG, "partials are needed for stats");
    if (!stats && mean_loss) return fail(SNAC_ERR_ARG, "mean_loss is stats[0]: stats is needed for it");
    if ((uintptr_t)action % 8) return fail(SNAC_ERR_ARG, "action must be 8-byte aligned");
    if (stats && ((uintptr_t)stats % 8 || (uintptr_t)partials % 8)) return fail(SNAC_ERR_ARG, "stats and partials must be 8-byte aligned");
    return by_actions(num_actions, [&](auto actions) -> int {
        constexpr int A = decltype(actions)::value;
        if (!loss && !grad_logits && !grad_value && !stats && !bad_rows) return SNAC_OK;      // nothing asked for
        const snac_spec::PpoParams p{clip, 1.0 - clip, 1.0 + clip, clip_vf, vf_coef, ent_coef, scale};
        const PpoArgs g{B, logits, action, logp_old, adv, value, value_old, ret, p, loss, grad_logits, grad_value, stats ? partials : nullptr, bad_rows};
        g_kernel = "k_ppo_loss";
        const long long W = ((long long)B + 63) / 64;                // waves, and rows of partials
        const hipStream_t s = (hipStream_t)stream;
        if (clip_v) hipLaunchKernelGGL((k_ppo_loss<A, true>), dim3((unsigned)W), dim3(64), 0, s, g);
        else hipLaunchKernelGGL((k_ppo_loss<A, false>), dim3((unsigned)W), dim3(64), 0, s, g);
        if (stats) hipLaunchKernelGGL(k_ppo_reduce, dim3(1), dim3(64), 0, s, (const double*)partials, W, B, stats, mean_loss);
        return launched("snac_ppo_loss");
    });
}
