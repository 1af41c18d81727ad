// k_policy_roll.hip -- snac_policy_rollout: T ticks of observe -> network -> draw -> step in ONE launch, the env state on chip from the
// first tick to the last.  include/snac_hip.h, "Acting with the device network over a rollout", has the rule; every piece of it is
// another unit's, run here between two barriers instead of between two launches: the K image and its reset / step (snac_dev.h, as
// k_rollout runs them), the layer loop (mlp_dev.h, k_mlp's) and the draw of a row of scores (policy_dev.h, k_policy_act's).
#include <cmath>
#include <cstddef>

#include "snac_units.h"
#include "mlp_rule.h"
#include "mlp_dev.h"
#include "policy_dev.h"

// k_policy_rollout<K>: envs are independent, so a block of 256 threads owns TR = 16 consecutive envs for all T ticks and nothing is
// synchronised across blocks.  LDS: the envs' K image (K*D<DYN, 16>, 2.4 / 5.0 / 21.4 KiB) beside k_mlp's arrays (activations, the
// weight tile: 60 928 bytes).  Wave 0 is the env wave, lane = env, and runs the image exactly as k_rollout's wave does (reset phase,
// K::step, the episodic sums in registers until the epilogue); all four waves run the layers and the row passes.  A tick:
//   wave 0     the reset phase; the envs' positions, plan rows and scalar slots into LDS (publish)
//   barrier
//   all        the input columns into act_a: the observation rows decoded from the image (only where the pass after the last step did
//              not already leave them there: the first tick, a tick with a reset, or no rows asked for) and, for a network that takes
//              them, the plans' cells from the table in memory (L2; act_a's upper rows do not survive a network of three layers)
//   all        mlp_layers (its first barrier orders the columns before their readers; it ends in one)
//   wave 0     per env: the scores out of LDS, the draw, K::step, the tick's outputs (coalesced spans of 16), publish
//   barrier
//   all        the row pass: the 16 rows decoded from the image (q = e * D + el: one contiguous span of the output per block, whatever
//              its alignment), each value also into act_a -- the next tick's input unless a reset intervenes
//   barrier    (the image is wave 0's again)
// The weights are read in place at every tick (L2 after the first); nothing of the net stays in LDS across ticks.  The observation
// dtype and the mode are run-time, uniform: six instantiations (kind x dynamic).  All arrays are indexed by unrolled constants.
namespace {

using namespace snac_detail;
using namespace snac_spec;
using namespace snac_mlp_dev;
using namespace snac_policy_dev;

struct RollArgs {
    KArgs a;                                                         // make_args: the state, the keys of streams 0 / 1, T, t0, obs_mode, the outputs of snac_rollout_rec
    snac_mlp net;
    int32_t mode, plan_in, has_value, obs_f64;
    uint32_t key_act;                                                // stream_key(seed, 5)
    double epsilon;
    const float* eps_env;
    float* value;
    float* logp;
    float* entropy;
    int32_t* bad_rows;
};

// value el of env e's canonical observation row, as write_obs decodes it: a window cell of the bordered image round (r, c), or one of
// the two scalar slots that write_scalars staged
template <class K>
__device__ __forceinline__ double row_value(uint32_t* img, int e, int el, int r, int c) {
    if (el >= K::W) return K::sc(img)[2 * e + (el - K::W)];
    if constexpr (K::D == 7) {
        return (double)K::hmap(img)[e * K::ES + r - 2 + el];
    } else {
        const int wi = el / 7, wj = el - 7 * wi;
        if constexpr (K::A == 8) {
            return (double)K::hmap(img)[e * K::ES + (r - 3 + wi) * 26 + (c - 3 + wj)];
        } else {
            const uint64_t w = K::cells(img)[(r - 3 + wi) * K::RS + e];
            return (double)(((int)((uint32_t)(w >> (2 * (c - 3 + wj))) << 30)) >> 30);   // signed 2-bit field: 0 / 1 / -1
        }
    }
}

template <class K>
__global__ __launch_bounds__(THREADS) void k_policy_rollout(const RollArgs g_) {
    const RollArgs& g = g_;
    static_assert(K::E == TR, "one env per row of the layer loop");
    constexpr int D = K::D, A = K::A, P = K::PLAN_CELLS;
    __shared__ float act_a[ACT_A_WORDS];
    __shared__ float act_b[ACT_B_WORDS];
    __shared__ __attribute__((aligned(16))) float wt[WT_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t img[K::LDS_WORDS];
    __shared__ int env_r[TR], env_c[TR], env_p[TR];
    __shared__ int any_reset;
    const KArgs& a = g.a;
    const int tid = threadIdx.x, lane = tid & 63;
    const bool env_wave = tid < 64;                                  // uniform per wave
    const int env0 = (int)blockIdx.x * TR;
    const int nenv = min(TR, a.n - env0);
    const bool active = env_wave && lane < nenv;
    const int env = env0 + (active ? lane : 0);
    const int32_t L = g.net.layers;
    const float* const res = mlp_result(L, act_a, act_b);

    Lane s;
    s.clear();
    s.r = 3; s.c = 3;                                                // idle lanes keep an in-range position
    int episode = 0;
    float eps_lane = 0.0f;
    EnvKeys sk{0, 0}, pk{0, 0}, ak{0, 0};
    if (env_wave) {
        if (active) {
            s.unpack(a.hdr[env]);
            episode = a.episode[env];
            if (g.eps_env) eps_lane = g.eps_env[env];
        }
        K::load_grid(img, a, env0, nenv, lane);
        for (int e = 0; e < nenv; ++e) K::load_plan(img, a, e, __builtin_amdgcn_readlane(s.pidx, e), lane);
        const uint64_t gid = (uint64_t)(a.env_id_base + env);
        sk = env_keys(a.key_step, gid), pk = env_keys(a.key_plan, gid), ak = env_keys(g.key_act, gid);
    }
    int d_eps = 0, d_ret = 0;
    long long d_iou = 0;
    auto publish = [&]() {                                           // wave 0: what the row passes read of the lanes' envs
        write_scalars<K, float, false>(img, s, a.total_step, lane, a);
        if (lane < TR) { env_r[lane] = s.r; env_c[lane] = s.c; env_p[lane] = s.pidx; }
    };
    // the 16 observation rows out of the image into act_a's first D rows and, with `out`, into the block's span of an output
    auto row_pass = [&](void* out) {
        for (int q = tid; q < TR * D; q += THREADS) {
            const int e = q / D, el = q - e * D;
            const bool live = e < nenv;
            const double v = live ? row_value<K>(img, e, el, env_r[e], env_c[e]) : 0.0;
            act_a[el * AS + e] = (float)v;
            if (out && live) {
                if (g.obs_f64) static_cast<double*>(out)[q] = v;
                else static_cast<float*>(out)[q] = (float)v;
            }
        }
    };
    bool rows_in_place = false;                                      // uniform: the last row pass left this tick's input in act_a

    for (int t = 0; t < a.T; ++t) {
        const size_t row = (size_t)t * (size_t)a.n + (size_t)env0;
        if (env_wave) {                                              // ---- the reset phase, as k_rollout's
            const bool nr = active && (s.flags & SNAC_FLAG_NEED_RESET);
            const bool some = __any(nr) != 0;
            if (some) {
                const int old_pidx = s.pidx, old_tb = s.tb;
                if (nr) {
                    episode += 1;
                    const int pidx = pick_plan<K>(a, pk, episode, old_pidx);
                    K::reset(a, s, pidx == old_pidx ? -1 : pidx);
                    if (pidx == old_pidx) { s.pidx = old_pidx; s.tb = old_tb; }
                }
                for (unsigned long long m = __ballot(nr); m; m &= m - 1) {
                    const int e = __ffsll(m) - 1;
                    const int pe = __builtin_amdgcn_readlane(s.pidx, e);
                    K::clear(img, e, lane);
                    if (pe != __builtin_amdgcn_readlane(old_pidx, e)) K::load_plan(img, a, e, pe, lane);
                }
            }
            if (some || t == 0) publish();
            if (lane == 0) any_reset = some ? 1 : 0;
        }
        __syncthreads();
        if (!rows_in_place || any_reset) row_pass(nullptr);          // ---- the input columns
        if (g.plan_in) {
            for (int q = tid; q < TR * P; q += THREADS) {
                const int e = q / P, cell = q - e * P;
                act_a[(D + cell) * AS + e] = e < nenv ? (float)K::plan_value(a, env_p[e], cell) : 0.0f;
            }
        }
        mlp_layers(g.net, act_a, act_b, wt, tid);                    // ---- the network

        if (env_wave) {                                              // ---- the draw and the step
            int reward = 0;
            bool done = false;
            // The section's arguments are read from the kernel-argument segment HERE, through an offset the compiler cannot see through:
            // hoisted out of the tick loop, the dozen output pointers and the keys hold scalar registers across the layer loop, and a
            // kernel at the scalar-register limit reserves a private segment (draw_action in snac_dev.h: the same device).
            int z = 0;
            asm volatile("" : "+s"(z));
            const RollArgs& g = ((const RollArgs*)__builtin_amdgcn_kernarg_segment_ptr())[z];
            const KArgs& a = g.a;
            if (active) {
                float y[A];
#pragma unroll
                for (int j = 0; j < A; ++j) y[j] = res[j * AS + lane];
                const uint32_t tau = a.t0 + (uint32_t)t;
                const uint32_t wa = rng_word(ak, tau);
                const double eps = g.eps_env ? (double)eps_lane : g.epsilon;
                PolicyDraw d;
                if (g.mode == SNAC_POLICY_CATEGORICAL) d = policy_draw<A, SNAC_POLICY_CATEGORICAL>(y, wa, eps, g.logp != nullptr, g.entropy != nullptr);
                else if (g.mode == SNAC_POLICY_GREEDY) d = policy_draw<A, SNAC_POLICY_GREEDY>(y, wa, eps, false, false);
                else d = policy_draw<A, SNAC_POLICY_EPS_GREEDY>(y, wa, eps, false, false);
                if (d.bad && g.bad_rows) atomicAdd(g.bad_rows, 1);
                if (g.logp) g.logp[row + lane] = d.logp;
                if (g.entropy) g.entropy[row + lane] = d.entropy;
                if (g.value) g.value[row + lane] = res[A * AS + lane];   // y[A] as it is (g.value is NULL unless dim[L] == A + 1)
                const uint32_t w = rng_word(sk, tau);
                const int act = d.action, k = 1 + (int)(((w & 0xffffu) * 3u) >> 16);
                K::step(img, a, s, act, k, a.ts_done, a.brick_gt, lane, reward, done);
                s.ep_ret = clamp16(s.ep_ret + reward);
                s.flags = done ? SNAC_FLAG_NEED_RESET : 0;
                if (a.reward) a.reward[row + lane] = (float)reward;
                if (a.done) a.done[row + lane] = done ? 1 : 0;
                if (a.actions_out) a.actions_out[row + lane] = (int8_t)act;
                if (a.step_size_out) a.step_size_out[row + lane] = (int8_t)k;
                if (a.plan_idx_out) a.plan_idx_out[row + lane] = (int16_t)s.pidx;
                if (a.first_out) a.first_out[row + lane] = s.cs == 1 ? 1 : 0;   // first step of its episode
            }
            if (__any(done)) {
                const double v = K::iou(img, s, active ? lane : 0);  // idle lanes stay inside the image
                if (done) { d_eps += 1; d_ret += s.ep_ret; d_iou += __double2ll_rn(v * FX40); }
            }
            publish();
        }
        __syncthreads();
        rows_in_place = a.obs_mode == SNAC_OBS_ALL || (a.obs_mode == SNAC_OBS_LAST && t == a.T - 1);
        if (rows_in_place) {                                         // ---- the rows after the step
            const size_t orow = (a.obs_mode == SNAC_OBS_ALL ? row : (size_t)env0) * D;
            row_pass(g.obs_f64 ? (void*)(static_cast<double*>(a.obs) + orow) : (void*)(static_cast<float*>(a.obs) + orow));
        }
        __syncthreads();
    }
    if (env_wave) {                                                  // ---- the epilogue, as k_rollout's
        K::store_grid(img, a, env0, nenv, lane);
        if (active) {
            a.hdr[env] = s.pack();
            a.episode[env] = episode;
            if (d_eps) {
                a.stat_episodes[env] += d_eps;
                a.stat_return[env] += d_ret;
                a.stat_iou_fx[env] += d_iou;
            }
        }
    }
}

template <template <bool, int> class KT>
void launch_kind(const snac_env_desc* d, const RollArgs& g, hipStream_t s) {
    const dim3 grid((unsigned)(((long long)g.a.n + TR - 1) / TR)), block(THREADS);
    if (d->dynamic != 0) hipLaunchKernelGGL((k_policy_rollout<KT<true, TR>>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((k_policy_rollout<KT<false, TR>>), grid, block, 0, s, g);
}

int aligned(const void* p, size_t n, const char* msg) { return ((uintptr_t)p % n) ? fail(SNAC_ERR_ARG, msg) : SNAC_OK; }

}  // namespace

extern "C" int snac_policy_rollout(const snac_env_desc* desc, const snac_state* st, const snac_mlp* net, int32_t T, uint32_t t0, int32_t mode,
                                   double epsilon, const float* epsilon_per_env, int obs_mode, void* obs, float* reward, uint8_t* done,
                                   const snac_rollout_record* rec, float* value, float* logp, float* entropy, int32_t* bad_rows, void* stream) {
    using namespace snac_detail;
    if (int rc = check_common(desc, st)) return rc;
    if (int rc = mlp_net_check(net)) return rc;
    if (T < 1) return fail(SNAC_ERR_ARG, "T must be >= 1");
    if (mode != SNAC_POLICY_CATEGORICAL && mode != SNAC_POLICY_GREEDY && mode != SNAC_POLICY_EPS_GREEDY)
        return fail(SNAC_ERR_ARG, "mode must be SNAC_POLICY_CATEGORICAL, _GREEDY or _EPS_GREEDY");
    if (!std::isfinite(epsilon) || epsilon < 0.0 || epsilon > 1.0) return fail(SNAC_ERR_ARG, "epsilon must be finite and in [0, 1]");
    if (epsilon_per_env && mode != SNAC_POLICY_EPS_GREEDY) return fail(SNAC_ERR_ARG, "epsilon_per_env belongs to the epsilon-greedy mode");
    if ((logp || entropy) && mode != SNAC_POLICY_CATEGORICAL) return fail(SNAC_ERR_ARG, "logp / entropy are defined by the categorical mode only");
    if (obs_mode == SNAC_OBS_TILED) return fail(SNAC_ERR_UNSUPPORTED, "SNAC_OBS_TILED is not a layout of snac_policy_rollout");
    if (obs_mode != SNAC_OBS_NONE && obs_mode != SNAC_OBS_ALL && obs_mode != SNAC_OBS_LAST) return fail(SNAC_ERR_ARG, "unknown obs_mode");
    if (obs_mode != SNAC_OBS_NONE && !obs) return fail(SNAC_ERR_ARG, "obs_mode set but obs is null");
    RollArgs g{};
    g.a = make_args(desc, st);
    if (g.a.variant) return fail(SNAC_ERR_UNSUPPORTED, "snac_policy_rollout takes the canonical observation layout only");
    const int D = base_obs_dim(desc->kind), P = desc->kind == SNAC_ENV_1D ? 30 : 400, A = desc->kind == SNAC_ENV_1D ? 3 : (desc->kind == SNAC_ENV_2D ? 5 : 8);
    const int32_t in = net->dim[0], out = net->dim[net->layers];
    if (in != D && in != D + P) return fail(SNAC_ERR_ARG, "dim[0] must be obs_dim, or obs_dim + the plan's cells (30 / 400)");
    if (out != A && out != A + 1) return fail(SNAC_ERR_ARG, "dim[layers] must be num_actions, or num_actions + 1 (the scores and the value)");
    if (value && out == A) return fail(SNAC_ERR_ARG, "value needs dim[layers] == num_actions + 1");
    const bool f64 = desc->obs_dtype == SNAC_OBS_F64;
    if (int rc = aligned(obs, f64 ? 8 : 4, "obs must be aligned as its element type")) return rc;
    if (int rc = aligned(epsilon_per_env, 4, "epsilon_per_env must be 4-byte aligned")) return rc;
    if ((uintptr_t)reward % 4 || (uintptr_t)value % 4 || (uintptr_t)logp % 4 || (uintptr_t)entropy % 4 || (uintptr_t)bad_rows % 4)
        return fail(SNAC_ERR_ARG, "reward, value, logp, entropy and bad_rows must be 4-byte aligned");
    if (rec && (uintptr_t)rec->plan_idx % 2) return fail(SNAC_ERR_ARG, "rec->plan_idx must be 2-byte aligned");
    g.a.T = T; g.a.t0 = t0; g.a.auto_reset = 1; g.a.obs_mode = obs_mode;
    g.a.obs = obs; g.a.reward = reward; g.a.done = done;
    if (rec) {
        g.a.actions_out = rec->actions; g.a.step_size_out = rec->step_size; g.a.plan_idx_out = rec->plan_idx; g.a.first_out = rec->first;
    }
    g.net = *net;
    g.mode = mode, g.plan_in = in != D, g.has_value = out != A, g.obs_f64 = f64;
    g.key_act = stream_key(desc->seed, 5);
    g.epsilon = epsilon, g.eps_env = epsilon_per_env;
    g.value = value, g.logp = logp, g.entropy = entropy, g.bad_rows = bad_rows;
    g_kernel = "k_policy_rollout";
    const hipStream_t s = (hipStream_t)stream;
    if (desc->kind == SNAC_ENV_1D) launch_kind<K1D>(desc, g, s);
    else if (desc->kind == SNAC_ENV_2D) launch_kind<K2D>(desc, g, s);
    else launch_kind<K3D>(desc, g, s);
    return launched("snac_policy_rollout");
}
