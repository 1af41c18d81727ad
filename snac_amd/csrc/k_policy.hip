// k_policy.hip -- snac_policy_act: one action per env from a row of A float32 scores (categorical, greedy, epsilon-greedy), with the
// categorical draw's log-probability and entropy.  include/snac_hip.h, "Acting from a policy", has the rule; softmax_rule.h states its softmax, for this kernel and for
// the rules of k_soft.hip and k_ppo.hip; policy_dev.h the draw of a row, for this kernel and k_policy_roll.hip.
#include <cmath>
#include <cstddef>

#include "snac_units.h"
#include "softmax_rule.h"
#include "policy_dev.h"

// lane = env: the outputs of a wave are coalesced spans of action / logp / entropy, and nothing crosses lanes.  The scores are read as A
// strided dword loads per lane, all issued before the first use.  A wave's rows are one contiguous span of 64 * A floats (768 / 1280 /
// 2048 bytes), so every line a load fetches is used whole and the A - 1 loads after the first hit the lines the first brought in; the rows
// of 12 and 20 bytes are no multiple of 16 and `scores` is only aligned as a float, so a wide-load form would need an aligned body with
// ragged ends and an LDS or cross-lane transpose -- for an input of 2 MB at 65 536 envs x 8 actions, which the float64 series below
// outweighs.  All arrays are indexed by unrolled constants: they live in registers, there is no scratch.
namespace {

using namespace snac_detail;
using namespace snac_spec;
using namespace snac_policy_dev;

struct PolicyArgs {
    int32_t n;
    uint32_t t, key;                                                 // key = stream_key(seed, 5)
    int64_t env_id_base;
    const float* scores;
    double epsilon;
    const float* eps_env;
    int8_t* action;
    float* logp;
    float* entropy;
    int32_t* bad_rows;
};

template <int A, int MODE>
__global__ __launch_bounds__(64) void k_policy_act(const PolicyArgs g) {
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= g.n) return;
    const float* row = g.scores + (size_t)i * A;
    float s[A];
#pragma unroll
    for (int a = 0; a < A; ++a) s[a] = row[a];                       // A loads on their way together
    float eps = 0.0f;
    if (MODE == SNAC_POLICY_EPS_GREEDY && g.eps_env) eps = g.eps_env[i];
    const uint32_t w = rng_word(env_keys(g.key, (uint64_t)(g.env_id_base + i)), g.t);

    const PolicyDraw d = policy_draw<A, MODE>(s, w, g.eps_env ? (double)eps : g.epsilon, g.logp != nullptr, g.entropy != nullptr);   // policy_dev.h
    if (d.bad && g.bad_rows) atomicAdd(g.bad_rows, 1);
    if (g.logp) g.logp[i] = d.logp;                                  // uniform: kernel arguments; NULL outside the categorical mode
    if (g.entropy) g.entropy[i] = d.entropy;
    const int action = d.action;
    if (g.action) g.action[i] = (int8_t)action;
}

}  // namespace

extern "C" int snac_policy_act(const snac_env_desc* desc, int32_t N, uint32_t t, int32_t mode, const float* scores, double epsilon,
                               const float* epsilon_per_env, int8_t* action, float* logp, float* entropy, int32_t* bad_rows, void* stream) {
    using namespace snac_detail;
    if (!desc || !scores) return fail(SNAC_ERR_ARG, "null desc/scores");
    snac_sizes sz;
    if (snac_env_sizes(desc->kind, desc->dynamic != 0, &sz) != SNAC_OK) return fail(SNAC_ERR_ARG, "unknown env kind");
    if (N < 1) return fail(SNAC_ERR_ARG, "N must be >= 1");
    if (mode != SNAC_POLICY_CATEGORICAL && mode != SNAC_POLICY_GREEDY && mode != SNAC_POLICY_EPS_GREEDY)
        return fail(SNAC_ERR_ARG, "mode must be SNAC_POLICY_CATEGORICAL, _GREEDY or _EPS_GREEDY");
    if (!std::isfinite(epsilon) || epsilon < 0.0 || epsilon > 1.0) return fail(SNAC_ERR_ARG, "epsilon must be finite and in [0, 1]");
    if (epsilon_per_env && mode != SNAC_POLICY_EPS_GREEDY) return fail(SNAC_ERR_ARG, "epsilon_per_env belongs to the epsilon-greedy mode");
    if ((logp || entropy) && mode != SNAC_POLICY_CATEGORICAL) return fail(SNAC_ERR_ARG, "logp / entropy are defined by the categorical mode only");
    if (!action && !logp && !entropy) return SNAC_OK;                // nothing asked for
    const PolicyArgs g{N, t, stream_key(desc->seed, 5), desc->env_id_base, scores, epsilon, epsilon_per_env, action, logp, entropy, bad_rows};
    return by_actions(sz.num_actions, [&](auto actions) {
        constexpr int A = decltype(actions)::value;
        g_kernel = "k_policy_act";
        const dim3 grid((unsigned)(((long long)N + 63) / 64)), block(64);
        const hipStream_t s = (hipStream_t)stream;
        if (mode == SNAC_POLICY_CATEGORICAL) hipLaunchKernelGGL((k_policy_act<A, SNAC_POLICY_CATEGORICAL>), grid, block, 0, s, g);
        else if (mode == SNAC_POLICY_GREEDY) hipLaunchKernelGGL((k_policy_act<A, SNAC_POLICY_GREEDY>), grid, block, 0, s, g);
        else hipLaunchKernelGGL((k_policy_act<A, SNAC_POLICY_EPS_GREEDY>), grid, block, 0, s, g);
        return launched("snac_policy_act");
    });
}
