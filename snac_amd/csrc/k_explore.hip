// k_explore.hip -- self-play's exploration noise on the UCT trees of k_uct.hip, drawn from the counter RNG: snac_explore_root_dirichlet
// (AlphaZero's Dirichlet noise mixed into the roots' priors, in place) and snac_explore_gumbel_scores (log priors plus Gumbel noise, the
// scores of the Gumbel root search).  include/snac_hip.h, "Exploration noise", has the rules; explore_rule.h states them per slot, for
// these kernels and for the host.  The third entry point of that section, snac_explore_pick_moves_temp, is beside k_uct_pick in k_uct_play.hip.
#include <cmath>
#include <cstddef>

#include "snac_units.h"
#include "explore_rule.h"

// Both kernels are lane = slot (b, a): eight lanes per tree whatever A is (lanes a >= A idle), eight trees per wave64, blocks of one wave.
// The rejection loop of a Gamma draw then diverges per draw and not per tree, and a tree's A draws run side by side.  A row's scan for
// bad priors, its largest logit and the sum of its terms are taken from the group's values through lane reads in index order: every lane
// of a group computes the same row values from the same operands in the same order.  A lane computes EXP of its own term only.  No LDS,
// no atomics on floats; every lane of the wave stays to the last lane read (a lane past B reads tree B - 1 and writes nothing).
namespace {

using namespace snac_detail;
using namespace snac_spec;

static_assert(EXPLORE_GROUP == 8 && sizeof(snac_uct_node) == 256, "eight lanes per tree; a statistics row is 64 words");

struct ExploreArgs {
    uint32_t* stats;                                                 // the rows as words
    int32_t B, cap;
    uint32_t key, t;
    int64_t env_id_base;
    const uint8_t* mask;                                             // Dirichlet: the trees to change; Gumbel: the trees that get noise
    GammaParams g;
    double om, eps;
    int32_t* bad_rows;
    float* scores;
};

struct Slot {
    int b, a;
    bool tree, slot;
    size_t word;                                                     // the slot's prior word in stats
    uint64_t env;                                                    // its key in the counter RNG
};

__device__ __forceinline__ Slot slot_of(const ExploreArgs& v) {
    Slot s;
    const int lane = (int)threadIdx.x;
    const long long b = (long long)blockIdx.x * (64 / EXPLORE_GROUP) + lane / EXPLORE_GROUP;
    s.a = lane % EXPLORE_GROUP;
    s.tree = b < v.B;
    s.b = s.tree ? (int)b : v.B - 1;
    s.word = (size_t)s.b * (size_t)v.cap * 64 + SNAC_UCT_PRIOR_WORD;
    s.env = (uint64_t)(v.env_id_base + s.b) * (uint64_t)EXPLORE_GROUP + (uint64_t)s.a;
    return s;
}

template <int A>
__global__ __launch_bounds__(64) void k_root_dirichlet(const ExploreArgs v) {
    Slot s = slot_of(v);
    s.slot = s.a < A;
    float* const mine = reinterpret_cast<float*>(v.stats) + s.word + (s.slot ? s.a : 0);      // an idle lane reads prior 0 and drops it
    const float p = *mine;
    const bool on = s.tree && (!v.mask || v.mask[s.b] != 0);
    float row[A];
#pragma unroll
    for (int a = 0; a < A; ++a) row[a] = __shfl(p, a, EXPLORE_GROUP);
    const bool bad = priors_bad<A>(row);
    const bool draw = on && !bad && s.slot && p > 0.0f;
    float l = -INFINITY;
    if (draw) {
        const EnvKeys k = env_keys(v.key, s.env);
        const uint32_t t = v.t;
        bool accepted;
        l = dirichlet_logit(p, v.g, [k, t](int j, int i) { return rng_word(k, dirichlet_counter(t, j, i)); }, accepted);
    }
    float lr[A];
#pragma unroll
    for (int a = 0; a < A; ++a) lr[a] = __shfl(l, a, EXPLORE_GROUP);
    float m;
    const bool none = softmax_scan<A>(lr, m);                        // no draw in this row: a bad or masked tree, a group past B
    const float own[1] = {l};
    double x[1], e1[1];
    softmax_terms<1>(own, none ? 0.0f : m, x, e1);
    double e[A];
#pragma unroll
    for (int a = 0; a < A; ++a) e[a] = __shfl(e1[0], a, EXPLORE_GROUP);
    const double S = terms_sum<A>(e);
    if (draw) *mine = dirichlet_mix(p, e1[0], S, v.om, v.eps);
    if (on && bad && s.a == 0 && v.bad_rows) atomicAdd(v.bad_rows, 1);
}

template <int A>
__global__ __launch_bounds__(64) void k_gumbel_scores(const ExploreArgs v) {
    Slot s = slot_of(v);
    if (!s.tree || s.a >= A) return;
    const float p = reinterpret_cast<const float*>(v.stats)[s.word + s.a];
    const bool noisy = !v.mask || v.mask[s.b] != 0;
    const uint32_t w = noisy ? rng_word(env_keys(v.key, s.env), v.t) : 0u;
    v.scores[(size_t)s.b * A + s.a] = gumbel_score(p, noisy, w);
}

template <int A>
void launch_explore(bool dirichlet, const ExploreArgs& v, hipStream_t s) {
    const dim3 grid((unsigned)(((long long)v.B + 7) / 8)), block(64);
    if (dirichlet) hipLaunchKernelGGL(k_root_dirichlet<A>, grid, block, 0, s, v);
    else hipLaunchKernelGGL(k_gumbel_scores<A>, grid, block, 0, s, v);
}

}  // namespace

extern "C" {

int snac_explore_root_dirichlet(const snac_env_desc* desc, int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap,
                                const uint8_t* mask, uint32_t t, double alpha, double eps, int32_t attempts, int32_t* bad_rows, void* stream) {
    using namespace snac_detail;
    if (!desc) return fail(SNAC_ERR_ARG, "null desc");
    if (int rc = play_check(num_actions, stats, stats_rows, B, cap)) return rc;
    if (!(alpha >= 0x1p-10 && alpha <= 0x1p10)) return fail(SNAC_ERR_ARG, "alpha must be in [2^-10, 2^10]");
    if (!(eps >= 0.0 && eps <= 1.0)) return fail(SNAC_ERR_ARG, "eps must be in [0, 1]");
    if (attempts < 1 || attempts > snac_spec::EXPLORE_MAX_ATTEMPTS) return fail(SNAC_ERR_ARG, "attempts must be in [1, 32]");
    if (eps == 0.0 && !bad_rows) return SNAC_OK;                     // every prior keeps its bits and nothing is counted
    double om;
    {
#pragma clang fp contract(off)
        om = 1.0 - eps;
    }
    const ExploreArgs v{(uint32_t*)stats, B, cap, stream_key(desc->seed, snac_spec::DIRICHLET_STREAM), t, desc->env_id_base, mask,
                        snac_spec::gamma_params(alpha, attempts), om, eps, bad_rows, nullptr};
    g_kernel = "k_root_dirichlet";
    if (num_actions == 3) launch_explore<3>(true, v, (hipStream_t)stream);
    else if (num_actions == 5) launch_explore<5>(true, v, (hipStream_t)stream);
    else launch_explore<8>(true, v, (hipStream_t)stream);
    return launched("snac_explore_root_dirichlet");
}

int snac_explore_gumbel_scores(const snac_env_desc* desc, int32_t num_actions, const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap,
                               const uint8_t* noisy, uint32_t t, float* scores, void* stream) {
    using namespace snac_detail;
    if (!desc) return fail(SNAC_ERR_ARG, "null desc");
    if (int rc = play_check(num_actions, stats, stats_rows, B, cap)) return rc;
    if (!scores) return fail(SNAC_ERR_ARG, "null scores");
    const ExploreArgs v{(uint32_t*)stats, B, cap, stream_key(desc->seed, snac_spec::GUMBEL_STREAM), t, desc->env_id_base, noisy,
                        snac_spec::GammaParams{}, 0.0, 0.0, nullptr, scores};
    g_kernel = "k_gumbel_scores";
    if (num_actions == 3) launch_explore<3>(false, v, (hipStream_t)stream);
    else if (num_actions == 5) launch_explore<5>(false, v, (hipStream_t)stream);
    else launch_explore<8>(false, v, (hipStream_t)stream);
    return launched("snac_explore_gumbel_scores");
}

}  // extern "C"
