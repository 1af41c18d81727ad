// k_qloss.hip -- snac_td_loss: the temporal-difference loss of a minibatch of Q-values (DQN, double DQN, n-step, SAC's critics), its
// gradient with respect to q, the new priorities and its statistics; snac_c51_loss: the cross-entropy of a projected categorical target
// and the online distribution of the action taken (Rainbow), its gradient with respect to the logits and its statistics.  Each in two
// launches on the caller's stream and in a fixed order of float64 additions.  include/snac_hip.h, "Q-learning losses", has the rules;
// td_rule.h states the first per sample, for the kernel and for the host.
#include <cmath>
#include <cstddef>

#include "snac_units.h"
#include "batch_sum.h"
#include "lane_dev.h"
#include "td_rule.h"

static_assert(SNAC_Q_STATS == snac_spec::TD_STATS && snac_spec::TD_STATS == snac_detail::BATCH_STATS, "the header's count of statistics is the rule's");

// k_td_loss: lane = sample, blocks of one wave, as k_ppo_loss: a lane reads its rows of q, q_next and q_select as A strided dword loads
// each and its scalars, all issued before the first use; a wave's rows are one contiguous span per input.  All arrays are indexed by
// unrolled constants (the taken and the chosen action are picked by compares): registers only, no scratch, no LDS.  The lanes past B and
// the bad lanes carry +0.0 in all eight contributions and stay in the wave for batch_sum.h's butterfly; lane 0 writes the wave's row of
// partials.  MODE: the target is y (TD_MODE_Y), or comes from q_next with the choice made on q_next (TD_MODE_NEXT) or on q_select (TD_MODE_DOUBLE).
// k_q_reduce: one wave over the partials, for both losses.  No atomics on floats, nothing waits for the host.
//
// k_c51_loss: lane = atom, as k_dist.hip: a row of K <= 64 logits and the row of m are one coalesced dword load each.  A block owns 64
// consecutive samples, so that stage 1 of the sums keeps its order: wave v of the block takes samples v * SPW .. v * SPW + SPW - 1 of them
// in turn.  The row's address needs the sample's action, so a wave loads the actions and weights of all its samples in one coalesced
// load up front (lane t: sample t of the wave) and reads them back with wave-uniform lane reads; the next sample's two rows are on their
// way while the current one is computed.  The four sums over the atoms are the header's TREE (lane_dev.h).  Lane 0 puts the sample's
// eight contributions in LDS slot `sample % 64`; after a barrier wave 0 runs the butterfly with lane j holding sample j, and writes the
// block's row of partials.  Everything a sample decides on (bad, the action) is wave-uniform.  C51L_WAVES = 8 (8 samples a wave) by
// measurement (profiles/r28_qloss.txt): of 1, 2, 4, 8 and 16 it is the fastest at B = 65 536 and within 0.003 ms of 16 below that.
namespace {

using namespace snac_detail;
using namespace snac_spec;

enum { TD_MODE_Y = 0, TD_MODE_NEXT = 1, TD_MODE_DOUBLE = 2 };

struct TdArgs {
    int32_t B;
    const float* q;
    const int64_t* action;
    const float* y;
    const float* q_next;
    const float* q_select;
    const float* ret;
    const float* discount;
    const float* weight;
    TdParams p;
    float* loss;
    float* priority;
    float* y_out;
    float* grad_q;
    double* partials;
    int32_t* bad_rows;
};

template <int A, int MODE>
__global__ __launch_bounds__(64) void k_td_loss(const TdArgs g) {
    constexpr bool NEXT = MODE != TD_MODE_Y;
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    const bool in = i < g.B;
    const size_t at = (size_t)(in ? i : 0) * A, is = (size_t)(in ? i : 0);      // a lane past B reads sample 0 and drops it
    const bool weighted = g.weight != nullptr;                       // uniform: a kernel argument
    float q[A], nxt[A], sel[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {                                    // every load of the lane on its way before the first use
        q[a] = g.q[at + a];
        nxt[a] = NEXT ? g.q_next[at + a] : 0.0f;
        sel[a] = MODE == TD_MODE_DOUBLE ? g.q_select[at + a] : nxt[a];      // without a q_select the choice is made on q_next itself
    }
    const int64_t action = g.action[is];
    const float ret = NEXT ? g.ret[is] : 0.0f, discount = NEXT ? g.discount[is] : 0.0f;
    const float y = NEXT ? 0.0f : g.y[is];
    const float weight = weighted ? g.weight[is] : 1.0f;

    const TdSample<A> o = td_sample<A, NEXT>(q, action, sel, nxt, ret, discount, y, weight, weighted, g.p);
    if (in) {
        if (o.bad && g.bad_rows) atomicAdd(g.bad_rows, 1);
        if (g.loss) g.loss[i] = o.loss;
        if (g.priority) g.priority[i] = o.priority;
        if (g.y_out) g.y_out[i] = o.y;
        if (g.grad_q) {
#pragma unroll
            for (int a = 0; a < A; ++a) g.grad_q[at + a] = o.grad[a];
        }
    }
    if (!g.partials) return;                                         // uniform: no statistics asked for
#pragma unroll
    for (int k = 0; k < TD_STATS; ++k) {
        const double s = wave_sum(in ? o.u[k] : 0.0);                // every lane of the wave is here: none has returned
        if (threadIdx.x == 0) g.partials[(size_t)blockIdx.x * TD_STATS + k] = s;
    }
}

__global__ __launch_bounds__(64) void k_q_reduce(const double* partials, long long W, int32_t B, double* stats, float* mean_loss) {
    reduce_partials<(1u << TD_GOOD)>(partials, W, B, stats, mean_loss);      // the number of good samples is not divided by B
}

#ifndef SNAC_C51L_WAVES
#define SNAC_C51L_WAVES 8
#endif
constexpr int C51L_WAVES = SNAC_C51L_WAVES;                          // waves per block
constexpr int C51L_SPW = 64 / C51L_WAVES;                            // samples a wave takes in turn
static_assert(C51L_WAVES >= 1 && C51L_WAVES <= 16 && C51L_SPW * C51L_WAVES == 64, "a block owns 64 samples");

struct C51LossArgs {
    int32_t B, K;
    const float* logits;
    const int64_t* action;
    const float* m;
    const float* weight;
    double scale;
    float* loss;
    float* grad;
    double* partials;
    int32_t* bad_rows;
};

struct C51Rows {                                                     // atom `lane` of the taken action's logits and of m
    float l, m;
};

// act < 0: the action is out of range and nothing is read through it
template <int A>
__device__ __forceinline__ C51Rows load_rows(const C51LossArgs& g, size_t b, int act, int lane, bool live) {
    C51Rows r;
    r.l = live && act >= 0 ? g.logits[(b * A + (size_t)(act < 0 ? 0 : act)) * (size_t)g.K + lane] : 0.0f;
    r.m = live ? g.m[b * (size_t)g.K + lane] : 0.0f;
    return r;
}

template <int A>
__global__ __launch_bounds__(64 * C51L_WAVES) void k_c51_loss(const C51LossArgs g) {
#pragma clang fp contract(off)
    __shared__ double u_lds[TD_STATS][64];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const long long first = (long long)blockIdx.x * 64 + (long long)wave * C51L_SPW;
    const int n = first >= g.B ? 0 : g.B - first < C51L_SPW ? (int)(g.B - first) : C51L_SPW;      // wave-uniform
    const bool live = lane < g.K, weighted = g.weight != nullptr;
    int acts = -1;                                                   // lane t: the action of the wave's sample t, -1 where out of range
    float weights = 1.0f;
    if (lane < n) {
        const int64_t a = g.action[first + lane];
        acts = a >= 0 && a < A ? (int)a : -1;
        if (weighted) weights = g.weight[first + lane];
    }
    C51Rows cur{0.0f, 0.0f};
    if (n > 0) cur = load_rows<A>(g, (size_t)first, __builtin_amdgcn_readlane(acts, 0), lane, live);
    for (int s = 0; s < n; ++s) {
        const size_t b = (size_t)first + s;
        const int act = __builtin_amdgcn_readlane(acts, s);
        const float wf = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(weights), s));
        C51Rows nxt = cur;
        if (s + 1 < n) nxt = load_rows<A>(g, b + 1, __builtin_amdgcn_readlane(acts, s + 1), lane, live);      // on their way during this sample
        bool bad = act < 0 || (weighted && (!(fabsf(wf) < INFINITY) || wf < 0.0f));
        bad |= __any(live && (!(fabsf(cur.l) < INFINITY) || !(fabsf(cur.m) < INFINITY))) != 0;
        double u[TD_STATS];
#pragma unroll
        for (int k = 0; k < TD_STATS; ++k) u[k] = 0.0;
        float ce32 = 0.0f, gj = 0.0f;
        if (!bad) {                                                  // wave-uniform
            float mx = live ? cur.l : -INFINITY;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));      // finite floats: the largest, in any order
            const double x = live ? (double)cur.l - (double)mx : 0.0;
            const double e = live ? spec_exp(x) : 0.0;
            const double S = tree_sum(e);
            const double T = tree_sum(e == 0.0 ? 0.0 : e * x);
            const double Lg = spec_log(S);
            const double lp = x - Lg, p = e / S, mj = (double)cur.m;
            const double ce = -tree_sum(live ? mj * lp : 0.0);
            const double M = tree_sum(mj);
            const double H = Lg - T / S;
            const double w = weighted ? (double)wf : 1.0;
            ce32 = (float)ce;
            gj = (float)(g.scale * (w * (M * p - mj)));
            u[0] = w * ce; u[1] = ce; u[2] = H; u[3] = M; u[6] = 1.0; u[7] = w;
        }
        if (lane == 0) {
            if (bad && g.bad_rows) atomicAdd(g.bad_rows, 1);
            if (g.loss) g.loss[b] = ce32;
            if (g.partials) {
#pragma unroll
                for (int k = 0; k < TD_STATS; ++k) u_lds[k][wave * C51L_SPW + s] = u[k];
            }
        }
        if (g.grad && live) {
            float* block = g.grad + (b * A) * (size_t)g.K + lane;
#pragma unroll
            for (int a = 0; a < A; ++a) block[(size_t)a * g.K] = a == act ? gj : 0.0f;      // the whole block; a bad sample's gj is 0
        }
        cur = nxt;
    }
    if (!g.partials) return;                                         // uniform over the block: no statistics asked for
    if (lane >= n && lane < C51L_SPW) {                              // the block's samples past B add 0.0
#pragma unroll
        for (int k = 0; k < TD_STATS; ++k) u_lds[k][wave * C51L_SPW + lane] = 0.0;
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int k = 0; k < TD_STATS; ++k) {
        const double sum = wave_sum(u_lds[k][lane]);                 // lane j holds sample j of the block: stage 1's order
        if (lane == 0) g.partials[(size_t)blockIdx.x * TD_STATS + k] = sum;
    }
}

}  // namespace

extern "C" int snac_td_loss(int32_t B, int32_t num_actions, const float* q, const int64_t* action, const float* y, const float* q_next,
                            const float* q_select, const float* ret, const float* discount, const float* weight, double delta, double scale,
                            float* loss, float* priority, float* y_out, float* grad_q, double* stats, float* mean_loss, double* partials,
                            int32_t* bad_rows, void* stream) {
    using namespace snac_detail;
    if (!q) return fail(SNAC_ERR_ARG, "null q");
    if (!action) return fail(SNAC_ERR_ARG, "null action");
    if (B < 1) return fail(SNAC_ERR_ARG, "B must be >= 1");
    const bool next = q_next || ret || discount;
    if (y && (next || q_select)) return fail(SNAC_ERR_ARG, "one target: y, or q_next, ret and discount, not both");
    if (!y && !next) return fail(SNAC_ERR_ARG, q_select ? "q_select belongs to q_next, ret and discount" : "a target is needed: y, or q_next, ret and discount");
    if (next && (!q_next || !ret || !discount)) return fail(SNAC_ERR_ARG, "q_next, ret and discount are needed together");
    if (!std::isfinite(delta) || delta < 0.0) return fail(SNAC_ERR_ARG, "delta must be finite and >= 0 (0: the squared error)");
    if (!std::isfinite(scale)) return fail(SNAC_ERR_ARG, "scale must be finite");
    if (stats && !partials) return fail(SNAC_ERR_ARG, "partials are needed for stats");
    if (!stats && mean_loss) return fail(SNAC_ERR_ARG, "mean_loss is stats[0]: stats is needed for it");
    if ((uintptr_t)action % 8) return fail(SNAC_ERR_ARG, "action must be 8-byte aligned");
    if (stats && ((uintptr_t)stats % 8 || (uintptr_t)partials % 8)) return fail(SNAC_ERR_ARG, "stats and partials must be 8-byte aligned");
    return by_actions(num_actions, [&](auto actions) -> int {
        constexpr int A = decltype(actions)::value;
        if (!loss && !priority && !y_out && !grad_q && !stats && !bad_rows) return SNAC_OK;      // nothing asked for
        const TdArgs g{B, q, action, y, q_next, q_select, ret, discount, weight, snac_spec::TdParams{delta, scale}, loss, priority, y_out, grad_q,
                       stats ? partials : nullptr, bad_rows};
        g_kernel = "k_td_loss";
        const long long W = ((long long)B + 63) / 64;                // waves, and rows of partials
        const hipStream_t s = (hipStream_t)stream;
        if (y) hipLaunchKernelGGL((k_td_loss<A, TD_MODE_Y>), dim3((unsigned)W), dim3(64), 0, s, g);
        else if (q_select) hipLaunchKernelGGL((k_td_loss<A, TD_MODE_DOUBLE>), dim3((unsigned)W), dim3(64), 0, s, g);
        else hipLaunchKernelGGL((k_td_loss<A, TD_MODE_NEXT>), dim3((unsigned)W), dim3(64), 0, s, g);
        if (stats) hipLaunchKernelGGL(k_q_reduce, dim3(1), dim3(64), 0, s, (const double*)partials, W, B, stats, mean_loss);
        return launched("snac_td_loss");
    });
}

extern "C" int snac_c51_loss(int32_t B, int32_t num_actions, int32_t atoms, const float* logits, const int64_t* action, const float* m,
                             const float* weight, double scale, float* loss, float* grad, double* stats, float* mean_loss, double* partials,
                             int32_t* bad_rows, void* stream) {
    using namespace snac_detail;
    if (!logits || !action || !m) return fail(SNAC_ERR_ARG, "null logits/action/m");
    if (B < 1) return fail(SNAC_ERR_ARG, "B must be >= 1");
    if (atoms < 2 || atoms > 64) return fail(SNAC_ERR_ARG, "atoms must be in [2, 64]");
    if (!std::isfinite(scale)) return fail(SNAC_ERR_ARG, "scale must be finite");
    if (stats && !partials) return fail(SNAC_ERR_ARG, "partials are needed for stats");
    if (!stats && mean_loss) return fail(SNAC_ERR_ARG, "mean_loss is stats[0]: stats is needed for it");
    if ((uintptr_t)action % 8) return fail(SNAC_ERR_ARG, "action must be 8-byte aligned");
    if (stats && ((uintptr_t)stats % 8 || (uintptr_t)partials % 8)) return fail(SNAC_ERR_ARG, "stats and partials must be 8-byte aligned");
    return by_actions(num_actions, [&](auto actions) -> int {
        constexpr int A = decltype(actions)::value;
        if (!loss && !grad && !stats && !bad_rows) return SNAC_OK;   // nothing asked for
        const C51LossArgs g{B, atoms, logits, action, m, weight, scale, loss, grad, stats ? partials : nullptr, bad_rows};
        g_kernel = "k_c51_loss";
        const long long W = ((long long)B + 63) / 64;                // blocks, and rows of partials
        const hipStream_t s = (hipStream_t)stream;
        hipLaunchKernelGGL(k_c51_loss<A>, dim3((unsigned)W), dim3(64 * C51L_WAVES), 0, s, g);
        if (stats) hipLaunchKernelGGL(k_q_reduce, dim3(1), dim3(64), 0, s, (const double*)partials, W, B, stats, mean_loss);
        return launched("snac_c51_loss");
    });
}
