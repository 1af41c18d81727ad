// k_search.hip -- snac_search_loss: the loss of a minibatch of self-play positions (AlphaZero, MuZero, Gumbel): the cross-entropy of the
// network's policy to the search's distribution, the squared or Huber error of its value to the return, the importance weights of
// prioritised replay, the mean, the gradient with respect to the logits and the value, the new priorities |value - z| and the
// statistics, in two launches on the caller's stream and in a fixed order of float64 additions.  include/snac_hip.h, "Search loss
// (AlphaZero / Gumbel self-play)", has the rule; search_rule.h states it per sample, for the first kernel and for the host.
#include <cmath>
#include <cstddef>

#include "snac_units.h"
#include "batch_sum.h"
#include "search_rule.h"

static_assert(SNAC_SEARCH_STATS == snac_spec::SEARCH_STATS && snac_spec::SEARCH_STATS == snac_detail::BATCH_STATS,
              "the header's count of statistics is the rule's");

// k_search_loss: lane = sample, blocks of one wave, as k_td_loss: a lane reads its rows of logits and pi as A strided dword loads each
// and its two or three scalars, all issued before the first use; a wave's rows are one contiguous span per input.  All arrays are
// indexed by unrolled constants: registers only, no scratch, no LDS.  The lanes past B and the bad lanes carry +0.0 in all eight
// contributions and stay in the wave for batch_sum.h's butterfly; lane 0 writes the wave's row of partials.
// k_search_reduce: one wave over the partials.  No atomics on floats, nothing waits for the host.
namespace {

using namespace snac_detail;
using namespace snac_spec;

struct SearchArgs {
    int32_t B;
    const float* logits;
    const float* value;
    const float* pi;
    const float* z;
    const float* weight;
    SearchParams p;
    float* loss;
    float* priority;
    float* grad_logits;
    float* grad_value;
    double* partials;
    int32_t* bad_rows;
};

template <int A>
__global__ __launch_bounds__(64) void k_search_loss(const SearchArgs g) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    const bool in = i < g.B;
    const size_t at = (size_t)(in ? i : 0) * A, is = (size_t)(in ? i : 0);      // a lane past B reads sample 0 and drops it
    const bool weighted = g.weight != nullptr;                       // uniform: a kernel argument
    float l[A], pi[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {                                    // every load of the lane on its way before the first use
        l[a] = g.logits[at + a];
        pi[a] = g.pi[at + a];
    }
    const float value = g.value[is], z = g.z[is];
    const float weight = weighted ? g.weight[is] : 1.0f;

    const SearchSample<A> o = search_sample<A>(l, value, pi, z, weight, weighted, g.p);
    if (in) {
        if (o.bad && g.bad_rows) atomicAdd(g.bad_rows, 1);
        if (g.loss) g.loss[i] = o.loss;
        if (g.priority) g.priority[i] = o.priority;
        if (g.grad_value) g.grad_value[i] = o.grad_value;
        if (g.grad_logits) {
#pragma unroll
            for (int a = 0; a < A; ++a) g.grad_logits[at + a] = o.grad[a];
        }
    }
    if (!g.partials) return;                                         // uniform: no statistics asked for
#pragma unroll
    for (int k = 0; k < SEARCH_STATS; ++k) {
        const double s = wave_sum(in ? o.u[k] : 0.0);                // every lane of the wave is here: none has returned
        if (threadIdx.x == 0) g.partials[(size_t)blockIdx.x * SEARCH_STATS + k] = s;
    }
}

__global__ __launch_bounds__(64) void k_search_reduce(const double* partials, long long W, int32_t B, double* stats, float* mean_loss) {
    reduce_partials<(1u << SEARCH_GOOD)>(partials, W, B, stats, mean_loss);      // the number of good samples is not divided by B
}

}  // namespace

extern "C" int snac_search_loss(int32_t B, int32_t num_actions, const float* logits, const float* value, const float* pi, const float* z,
                                const float* weight, double vf_coef, double delta, double scale, float* loss, float* priority,
                                float* grad_logits, float* grad_value, double* stats, float* mean_loss, double* partials, int32_t* bad_rows,
                                void* stream) {
    using namespace snac_detail;
    if (!logits) return fail(SNAC_ERR_ARG, "null logits");
    if (!value) return fail(SNAC_ERR_ARG, "null value");
    if (!pi) return fail(SNAC_ERR_ARG, "null pi");
    if (!z) return fail(SNAC_ERR_ARG, "null z");
    if (B < 1) return fail(SNAC_ERR_ARG, "B must be >= 1");
    if (!std::isfinite(vf_coef) || vf_coef < 0.0) return fail(SNAC_ERR_ARG, "vf_coef must be finite and >= 0");
    if (!std::isfinite(delta) || delta < 0.0) return fail(SNAC_ERR_ARG, "delta must be finite and >= 0 (0: the squared error)");
    if (!std::isfinite(scale)) return fail(SNAC_ERR_ARG, "scale must be finite");
    if (stats && !partials) return fail(SNAC_ERR_ARG, "partials are needed for stats");
    if (!stats && mean_loss) return fail(SNAC_ERR_ARG, "mean_loss is stats[0]: stats is needed for it");
    if (stats && ((uintptr_t)stats % 8 || (uintptr_t)partials % 8)) return fail(SNAC_ERR_ARG, "stats and partials must be 8-byte aligned");
    return by_actions(num_actions, [&](auto actions) -> int {
        constexpr int A = decltype(actions)::value;
        if (!loss && !priority && !grad_logits && !grad_value && !stats && !bad_rows) return SNAC_OK;      // nothing asked for
        const SearchArgs g{B, logits, value, pi, z, weight, snac_spec::SearchParams{vf_coef, delta, scale}, loss, priority, grad_logits, grad_value,
                           stats ? partials : nullptr, bad_rows};
        g_kernel = "k_search_loss";
        const long long W = ((long long)B + 63) / 64;                // waves, and rows of partials
        const hipStream_t s = (hipStream_t)stream;
        hipLaunchKernelGGL(k_search_loss<A>, dim3((unsigned)W), dim3(64), 0, s, g);
        if (stats) hipLaunchKernelGGL(k_search_reduce, dim3(1), dim3(64), 0, s, (const double*)partials, W, B, stats, mean_loss);
        return launched("snac_search_loss");
    });
}
