// k_tile.inc -- the tile kernels of rounds 1-2 (k_rollout / k_transition / k_aux: one tile of E envs per wave, K::step on the
// bordered LDS image, rows by write_obs) and their launch templates; included by k_tile1d.hip / k_tile2d.hip / k_tile3d.hip, which
// instantiate them for one env kind each.  Everything the specialised kernels do not take runs here.
#include "snac_units.h"

namespace {

// T fused vector steps (T = 1: one step() call) for one tile of E envs per wave.
// EXPL: actions and / or step sizes come from the caller's arrays.  The counter-RNG instantiation (EXPL = false) has no
// global load in its loop at all: with the null tests at run time the compiler joins both paths behind one
// `s_waitcnt vmcnt(0)`, and vmcnt counts the observation stores too -- every tick would wait for the previous tick's rows.
template <class K, typename OT, int WPB, bool EXPL, bool VAR>
__global__ __launch_bounds__(WPB * 64) void k_rollout(const KArgs a) {
    constexpr int E = K::E;
    const int LD = VAR ? a.ld : K::D;
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * WPB + (int)(threadIdx.x >> 6);
    const int env0 = __builtin_amdgcn_readfirstlane(tile * E);
    if (env0 >= a.n) return;
    const int nenv = min(E, a.n - env0);
    const bool active = lane < nenv;
    const int env = env0 + (active ? lane : 0);
    uint32_t* lds = wave_lds<K, WPB>();
    // 3D keeps no plan in LDS (a step needs one cell); the layout variants' plan tail needs all 400 every tick: its rows get a copy of
    // their own here, refilled when an env starts over on another row
    constexpr bool P3 = VAR && K::A == 8;
    __shared__ int16_t plan3_all[P3 ? WPB * E * 400 : 1];
    int16_t* const plan3 = plan3_all + (P3 ? (int)(threadIdx.x >> 6) * E * 400 : 0);
    auto load_plan3 = [&](int e, int pidx) {
        if constexpr (P3) {
            if (a.tail & SNAC_TAIL_PLAN) {
                const uint32_t* const src = (const uint32_t*)((const int16_t*)a.plans + (size_t)pidx * 400);
                uint32_t* const dst = (uint32_t*)(plan3 + e * 400);
                for (int i = lane; i < 200; i += 64) dst[i] = src[i];
            }
        }
    };
    Lane s;
    s.clear();
    s.r = 3; s.c = 3;                                                // idle lanes keep an in-range position
    int episode = 0;
    if (active) { s.unpack(a.hdr[env]); episode = a.episode[env]; }
    asm volatile("" : "+v"(episode));                                // waited for HERE, not in the loop's reset branch behind the row stores
    K::load_grid(lds, a, env0, nenv, lane);
    for (int e = 0; e < nenv; ++e) { K::load_plan(lds, a, e, __builtin_amdgcn_readlane(s.pidx, e), lane); load_plan3(e, __builtin_amdgcn_readlane(s.pidx, e)); }
    const uint64_t gid = (uint64_t)(a.env_id_base + env);
    const EnvKeys sk = env_keys(a.key_step, gid), pk = env_keys(a.key_plan, gid);
    int d_eps = 0, d_ret = 0;
    long long d_iou = 0;
    OT* const obs = (OT*)a.obs;
    for (int t = 0; t < a.T; ++t) {
        const size_t row = (size_t)t * (size_t)a.n + (size_t)env0;
        int reward = 0;
        bool done = false;
        const bool nr = active && a.auto_reset && (s.flags & SNAC_FLAG_NEED_RESET);
        if (__builtin_expect(__any(nr), 0)) {                        // rare paths out of line: a taken branch costs a lone wave ~30 cycles
            const int old_pidx = s.pidx, old_tb = s.tb;
            if (nr) {
                episode += 1;
                const int pidx = pick_plan<K>(a, pk, episode, old_pidx);
                K::reset(a, s, pidx == old_pidx ? -1 : pidx);   // -1: same plan again (static tables): keep tb, no load
                if (pidx == old_pidx) { s.pidx = old_pidx; s.tb = old_tb; }
            }
            for (unsigned long long m = __ballot(nr); m; m &= m - 1) {
                const int e = __ffsll(m) - 1;
                const int pe = __builtin_amdgcn_readlane(s.pidx, e);
                K::clear(lds, e, lane);
                // a vector load here waits for every observation store issued before it (vmcnt is in-order): skip it
                // when the env keeps its plan
                if (pe != __builtin_amdgcn_readlane(old_pidx, e)) { K::load_plan(lds, a, e, pe, lane); load_plan3(e, pe); }
            }
        }
        if (active) {
            const uint32_t w = rng_word(sk, a.t0 + (uint32_t)t);
            int act = draw_action<K::A>(w, a), k = 1 + (int)(((w & 0xffffu) * 3u) >> 16);
            if constexpr (EXPL) {
                if (a.actions) act = (int)a.actions[row + lane];
                if (a.step_size) k = min(max((int)a.step_size[row + lane], 1), 3);
            }
            K::step(lds, a, s, act, k, a.ts_done, a.brick_gt, lane, reward, done);
            s.ep_ret = clamp16(s.ep_ret + reward);
            s.flags = done ? SNAC_FLAG_NEED_RESET : 0;
            if (a.reward) a.reward[row + lane] = (float)reward;
            if (a.done) a.done[row + lane] = done ? 1 : 0;
            if (a.actions_out) a.actions_out[row + lane] = (int8_t)act;
            if (a.step_size_out) a.step_size_out[row + lane] = (int8_t)k;
            if (a.plan_idx_out) a.plan_idx_out[row + lane] = (int16_t)s.pidx;
            if (a.first_out) a.first_out[row + lane] = s.cs == 1 ? 1 : 0;   // first step of its episode
        }
        if (__builtin_expect(__any(done), 0)) {
            const double v = K::iou(lds, s, active ? lane : 0);      // idle lanes stay inside the wave's LDS slice
            if (done) { d_eps += 1; d_ret += s.ep_ret; d_iou += __double2ll_rn(v * FX40); }
        }
        if (a.obs_mode == SNAC_OBS_ALL || a.obs_mode == SNAC_OBS_TILED || (a.obs_mode == SNAC_OBS_LAST && t == a.T - 1)) {
            // SNAC_OBS_TILED: [ceil(N / 64)][T][64][LD] -- the tile's rows of step t follow its rows of step t - 1
            const size_t orow = a.obs_mode == SNAC_OBS_ALL ? row
                              : (a.obs_mode == SNAC_OBS_TILED ? ((size_t)(env0 >> 6) * (size_t)a.tiled_T + (size_t)(a.tiled_t0 + t)) * 64 + (size_t)(env0 & 63) : (size_t)env0);
            emit_obs<K, OT, VAR, true>(lds, obs + orow * LD, nenv, s, a, lane, StepOut{reward, done ? 1 : 0}, plan3);
        }
    }
    K::store_grid(lds, a, env0, nenv, lane);
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


// transition(state, action) of the MCTS variants (Env/2D/DMP_ENV_2D_dynamic_MCTS.py:117-175 and the eight sibling files;
// caller: script/MCTS/utils/mcts_Qvalue_dynamic.py:88,118): ONE step of the same K::step on an explicit state, batched over
// a.n tree edges.  The state arrays are a node pool; edge i reads row src_index[i] and writes row dst_index[i] (out of
// place), the observation / reward / done rows are per edge.  snac_transition: no auto-reset, no episodic sums (a search
// is not an episode).  snac_step is the same kernel on the identity rows with both switched on.
template <class K, typename OT, int WPB, bool VAR>
__global__ __launch_bounds__(WPB * 64) void k_transition(const KArgs a) {
    constexpr int E = K::E;
    const int LD = VAR ? a.ld : K::D;
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * WPB + (int)(threadIdx.x >> 6);
    const int env0 = __builtin_amdgcn_readfirstlane(tile * E);
    if (env0 >= a.n) return;
    const int nenv = min(E, a.n - env0);
    const bool active = lane < nenv;
    const int edge = env0 + (active ? lane : 0);
    uint32_t* lds = wave_lds<K, WPB>();
    Lane s;
    s.clear();
    s.r = 3; s.c = 3;
    int episode = 0;
    const size_t srow = row_of(a.src_index, a.pool, edge), drow = row_of(a.dst_index, a.pool, edge);
    if (active) { s.unpack(a.hdr[srow]); episode = a.episode[srow]; }
    const uint64_t gid = (uint64_t)(a.env_id_base + edge);
    // snac_step with auto_reset: an env whose previous step returned done starts a new episode first (as in k_rollout)
    const bool nr = active && a.auto_reset && (s.flags & SNAC_FLAG_NEED_RESET);
    if (nr) {
        const int old_pidx = s.pidx, old_tb = s.tb;
        episode += 1;
        const int pidx = pick_plan<K>(a, env_keys(a.key_plan, gid), episode, old_pidx);
        K::reset(a, s, pidx == old_pidx ? -1 : pidx);
        if (pidx == old_pidx) { s.pidx = old_pidx; s.tb = old_tb; }
    }
    // one step reads one plan cell (3D: one of four): fetch it now, next to the tile's records, instead of staging plans
    const typename K::PlanCell pc = K::fetch_plan_cell(a, s);
    int* const rows = (int*)K::sc(lds);                          // free until write_scalars: the tile's gather / scatter rows
    if (a.src_index && active) rows[lane] = (int)srow;
    K::load_grid(lds, a, env0, nenv, lane, a.src_index ? rows : nullptr);
    for (unsigned long long m = __ballot(nr); m; m &= m - 1) K::clear(lds, __ffsll(m) - 1, lane);
    if (active) K::put_plan_cell(lds, s, pc, lane);
    int reward = 0;
    bool done = false;
    if (active) {
        const uint32_t w = rng_word(env_keys(a.key_step, gid), a.t0);
        int act = draw_action<K::A>(w, a), k = 1 + (int)(((w & 0xffffu) * 3u) >> 16);
        if (a.use_scalar) { act = a.act_scalar; k = a.k_scalar; }   // snac_step_scalar: by value, no input arrays
        if (a.actions) act = (int)a.actions[edge];
        if (a.step_size) k = (int)a.step_size[edge];
        k = min(max(k, 1), 3);
        K::step(lds, a, s, act, k, a.ts_done, a.brick_gt, lane, reward, done);
        s.ep_ret = clamp16(s.ep_ret + reward);
        s.flags = done ? SNAC_FLAG_NEED_RESET : 0;
        if (a.reward) a.reward[edge] = (float)reward;
        if (a.done) a.done[edge] = done ? 1 : 0;
    }
    if (a.stats_on && __any(done)) {                             // snac_step: episodic sums (the IoU needs the whole plan)
        if constexpr (K::A != 8)
            for (unsigned long long m = __ballot(done); m; m &= m - 1) {
                const int e = __ffsll(m) - 1;
                K::load_plan(lds, a, e, __builtin_amdgcn_readlane(s.pidx, e), lane);
            }
        const double v = K::iou(lds, s, active ? lane : 0);
        if (done) {
            a.stat_episodes[drow] += 1;
            a.stat_return[drow] += s.ep_ret;
            a.stat_iou_fx[drow] += __double2ll_rn(v * FX40);
        }
    }
    if constexpr (VAR && K::A != 8) {
        // 1D / 2D: a row with the plan tail needs its env's whole plan: staged in LDS first (every load before the first row store: from
        // the table in memory each batch of 64 plan cells is a vector load behind the stores before it; 2D PPO rows at 16 384 envs:
        // 26.6 -> 19.3 us per tick).  3D keeps reading the table: its 800-byte plans cost more to stage than they save (130 -> 160 us
        // at 65 536 envs, six instead of nine waves per CU).
        if (a.obs && (a.tail & SNAC_TAIL_PLAN)) {
            for (int e = 0; e < nenv; ++e) K::load_plan(lds, a, e, __builtin_amdgcn_readlane(s.pidx, e), lane);
            emit_obs<K, OT, VAR, true>(lds, (OT*)a.obs + (size_t)env0 * LD, nenv, s, a, lane, StepOut{reward, done ? 1 : 0});
        } else if (a.obs) {
            emit_obs<K, OT, VAR>(lds, (OT*)a.obs + (size_t)env0 * LD, nenv, s, a, lane, StepOut{reward, done ? 1 : 0});
        }
    } else {
        if (a.obs) emit_obs<K, OT, VAR>(lds, (OT*)a.obs + (size_t)env0 * LD, nenv, s, a, lane, StepOut{reward, done ? 1 : 0});
    }
    if (a.dst_index && active) rows[lane] = (int)drow;           // the scalar slots have been written out by now
    K::store_grid(lds, a, env0, nenv, lane, a.dst_index ? rows : nullptr);
    if (active) { a.hdr[drow] = s.pack(); a.episode[drow] = episode; }
}


// reset(mask, plan_idx_in) / observe / iou on the same tile machinery
template <class K, typename OT, int WPB, bool VAR>
__global__ __launch_bounds__(WPB * 64) void k_aux(const KArgs a) {
    constexpr int E = K::E;
    const int LD = VAR ? a.ld : K::D;
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * WPB + (int)(threadIdx.x >> 6);
    const int env0 = __builtin_amdgcn_readfirstlane(tile * E);
    if (env0 >= a.n) return;
    const int nenv = min(E, a.n - env0);
    const bool active = lane < nenv;
    const int env = env0 + (active ? lane : 0);
    uint32_t* lds = wave_lds<K, WPB>();
    Lane s;
    s.clear();
    s.r = 3; s.c = 3;
    if (active) s.unpack(a.hdr[env]);
    K::load_grid(lds, a, env0, nenv, lane);
    if (a.aux_op == AUX_IOU)
        for (int e = 0; e < nenv; ++e) K::load_plan(lds, a, e, __builtin_amdgcn_readlane(s.pidx, e), lane);
    if (a.aux_op == AUX_RESET) {
        const bool doit = active && (a.mask ? a.mask[env] != 0 : true);
        for (unsigned long long m = __ballot(doit); m; m &= m - 1) K::clear(lds, __ffsll(m) - 1, lane);
        if (doit) {
            const int episode = a.episode[env] + 1;
            int pidx;
            if (a.plan_idx_in) pidx = a.plan_idx_in[env];
            else if (a.plan_scalar >= 0) pidx = a.plan_scalar;
            else pidx = pick_plan<K>(a, env_keys(a.key_plan, (uint64_t)(a.env_id_base + env)), episode, a.static_plan);
            pidx = min(max(pidx, 0), a.num_plans - 1);
            K::reset(a, s, pidx);
            a.hdr[env] = s.pack();
            a.episode[env] = episode;
        }
        K::store_grid(lds, a, env0, nenv, lane);
    }
    if (a.aux_op == AUX_IOU) {
        const double v = K::iou(lds, s, active ? lane : 0);      // 3D: from the running sum kept in the header
        if (active) a.out_f64[env] = v;
        return;
    }
    // SNAC_TAIL_RECORD outside a step: reward 0, done = the env's pending-reset flag
    if (a.obs) emit_obs<K, OT, VAR>(lds, (OT*)a.obs + (size_t)env0 * LD, nenv, s, a, lane, StepOut{0, (s.flags & SNAC_FLAG_NEED_RESET) ? 1 : 0});
}

template <class K, typename OT, int WPB>
void launch_k(Op op, const KArgs& a, hipStream_t s) {
    const int tiles = (a.n + K::E - 1) / K::E;
    const dim3 grid((unsigned)((tiles + WPB - 1) / WPB)), block(WPB * 64);
    if (a.variant) {                                             // layout variants: their own instantiations, the canonical ones stay lean
        if (op == OP_ROLLOUT) hipLaunchKernelGGL((k_rollout<K, OT, WPB, true, true>), grid, block, 0, s, a);
        else if (op == OP_TRANSITION) hipLaunchKernelGGL((k_transition<K, OT, WPB, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_aux<K, OT, WPB, true>), grid, block, 0, s, a);
        return;
    }
    if (op == OP_ROLLOUT) {
        if (a.actions || a.step_size) hipLaunchKernelGGL((k_rollout<K, OT, WPB, true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_rollout<K, OT, WPB, false, false>), grid, block, 0, s, a);
    }
    else if (op == OP_TRANSITION) hipLaunchKernelGGL((k_transition<K, OT, WPB, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_aux<K, OT, WPB, false>), grid, block, 0, s, a);
}

template <template <bool, int> class KT, bool DYN, int E, int WPB>
void launch_dt(Op op, int obs_dtype, const KArgs& a, hipStream_t s) {
    if (obs_dtype == SNAC_OBS_F32) launch_k<KT<DYN, E>, float, WPB>(op, a, s);
    else launch_k<KT<DYN, E>, double, WPB>(op, a, s);
}

template <template <bool, int> class KT, int WPB>
void launch_tile(Op op, bool dyn, int E, int obs_dtype, const KArgs& a, hipStream_t s) {
    if (E == 64) dyn ? launch_dt<KT, true, 64, WPB>(op, obs_dtype, a, s) : launch_dt<KT, false, 64, WPB>(op, obs_dtype, a, s);
    else if (E == 32) dyn ? launch_dt<KT, true, 32, WPB>(op, obs_dtype, a, s) : launch_dt<KT, false, 32, WPB>(op, obs_dtype, a, s);
    else if (E == 16) dyn ? launch_dt<KT, true, 16, WPB>(op, obs_dtype, a, s) : launch_dt<KT, false, 16, WPB>(op, obs_dtype, a, s);
    else dyn ? launch_dt<KT, true, 8, 1>(op, obs_dtype, a, s) : launch_dt<KT, false, 8, 1>(op, obs_dtype, a, s);
}

}  // namespace
