// snac_units.h -- what every translation unit of libsnac_hip.so includes (internal, not installed): the map of the units below, the
// shared device code (snac_dev.h, included from here and from nowhere else) and the host-side declarations that tie the units together:
// the shared checks, the dispatch, and the per-family launch functions that the dispatch in snac_hip.hip calls.  A new kernel family
// adds its line to the map and its shared check or launcher here; snac_dev.h stays as it is, and with it the stamp of the headline's
// counters (profiles/traffic.json).
//
// Integer / indexing work only -- no MFMA; the bound is HBM (observation rows written) or, for small batches, the chain of ticks.
// DESIGN.md section 3 has the table of kernels with their measured times.  Translation units (one object each, built in parallel):
//   k_roll2d.hip    k_rollout2d   the headline: 2D rollouts on tiles of 64 envs, lane = env in the transition AND in the observation rows;
//                                 plan rows per wave in LDS, refilled through the scalar cache; no vector load in the loop
//   k_roll2dt.hip   k_rollout2dt  2D rollouts of small and middle batches, time-parallel: one wave per env, lane = tick
//   k_roll1dt.hip   k_rollout1dt  the same idea for 1D
//   k_roll1dl.hip   k_rollout1dl  1D rollouts of large batches: lane = env, the headline kernel's shape (rows1d.h: the 1D rows of a wave as one run)
//   k_roll3db.hip   k_rollout3db  3D rollouts: one stepper wave (lane = env) and eight writer waves per 64 envs, one barrier per tick
//   k_roll3d.hip    k_rollout3d   3D rollouts of small / odd batches: 8 envs per wave, software-pipelined round the store stream
//   k_step.hip      k_step2d / 3d snac_step on identity rows: wide loads, rows through emit_tile; AUX forms: masked resets and observe without a step
//   k_step3dq.hip   k_step3dq     the canonical 3D snac_step: 16 envs per wave, four lanes per env
//   k_step1d.hip    k_step1d, k_edges1d   the 1D snac_step (canonical rows and the layout variants) and 1D tree edges
//   k_reset.hip     k_reset, k_iou        whole-batch resets without reading the old state; snac_iou lane-per-env
//   k_nodes.hip     k_edges1dp / 2dp / 3dp   tree edges on node pools of one record per node (one 128-byte line, 3D: seven), k_nodes_copy
//   k_nodes_obs.hip k_observe1dp / 2dp / 3dp   the observation rows of node records
//                   (nodes_dev.h: the record's map, its trip through LDS and the window decoders, for these two and k_eval.hip)
//   k_eval.hip      k_eval        default-policy evaluation of tree leaves in place on node pools: lane = leaf, the rollout and the sum fused
//   k_uct.hip       k_uct_select / backup / advance and their K-paths, PUCT, normalised and Gumbel forms: tree search over node pools
//   k_uct_play.hip, k_uct_reanalyse.hip   self-play and Reanalyse on those trees
//                   (uct_dev.h: the map of a statistics row in pieces and words, for these three)
//   k_mailbox.hip   k_mailbox     the resident stepper behind the drop-in classes (mailbox_host.h: the host half of its protocol)
//   k_trans.hip     k_transition2d / 3d, k_edges3d: single steps and tree edges with gathered rows
//   k_tile{1,2,3}d.hip  the tile kernels k_rollout / k_transition / k_aux (rounds 1-2) behind all of them (templates: k_tile.inc)
//   k_misc.hip      export / import / equality / plan generators / the episodic sums, with their entry points
//   k_replay.hip    k_gather      minibatches out of the replay ring: the tuple of a step (s, s', the plan), 4 samples a wave;
//                   k_gather_nstep / k_gather_windows   walks along an env's column of the ring: n-step transitions, episode windows;
//                   k_gather_onpolicy   PPO's minibatch: s, the plan and five scalars of a sample
//                   (at its head, once for all four: the argument head, a lane's sample pick, the ring's row address, the reset
//                   observation and the plan expansion; on the host the two halves of the shared check and by_kind)
//   k_onpolicy.hip  k_gae         generalised advantage estimation over a span of the ring: lane = env, the loads of a chunk of slots issued together
//   k_policy.hip    k_policy_act  one action per env from a row of policy scores (categorical / greedy / epsilon-greedy), logp and entropy: lane = env
//   k_dist.hip      k_c51_expect / k_c51_project   categorical (C51) value distributions: expected values, the choice of the next action and the
//                                 projected TD target: lane = atom, a wave per sample, the scatter turned into an ordered gather
//   k_soft.hip      k_soft_value  discrete SAC's soft state value, TD target, entropy and actor-loss gradient from one softmax: lane = sample
//                   (soft_rule.h: the per-sample rule, host and device)
//   k_ppo.hip       k_ppo_loss / k_ppo_reduce   PPO2's clipped loss, its gradient and its statistics: lane = sample, then the batch sums in a
//                                 fixed order: an xor butterfly per wave, one wave over the waves' partials (ppo_rule.h: the per-sample rule)
//   k_qloss.hip     k_td_loss / k_q_reduce      the TD loss of a minibatch of Q-values (DQN, double DQN, n-step, SAC's critics), its gradient, the
//                                 new priorities and its statistics: lane = sample (td_rule.h: the per-sample rule), then the batch sums
//                   k_c51_loss    Rainbow's cross-entropy of the projected target and the online logits, its gradient and statistics:
//                                 lane = atom, a block per 64 samples, the samples' contributions through LDS into the same sums
//   k_search.hip    k_search_loss / k_search_reduce   the loss of self-play positions (AlphaZero, Gumbel): the cross-entropy to the search's
//                                 distribution, the value error, their gradients, the new priorities and the statistics: lane = sample
//                                 (search_rule.h: the per-sample rule), then the batch sums
//   k_explore.hip   k_root_dirichlet / k_gumbel_scores   self-play's exploration noise from the counter RNG: Dirichlet noise into the roots'
//                                 priors, log priors plus Gumbel noise: lane = slot (b, a), eight lanes per tree, the row's softmax through
//                                 lane reads (explore_rule.h: the Gamma draw, the slots' pieces and the move by a temperature, which
//                                 k_uct_pick in k_uct_play.hip runs, host and device)
//                   (for k_ppo.hip, k_qloss.hip and k_search.hip: batch_sum.h, the wave's butterfly and the second stage of the batch sums; for
//                   k_dist.hip and k_c51_loss: lane_dev.h, the lane read, the DPP row move and the shuffle-down tree)
//                   (for k_policy.hip and the soft, PPO and search rules: softmax_rule.h, the float64 softmax of a row of scores in three steps, on
//                   spec_math.h's EXP and LOG; for those four units, k_dist.hip and k_qloss.hip: by_actions below, the choice of the A = 3 / 5 / 8 instance)
//   k_mlp.hip       k_mlp         the policy / value network of the PUCT search: an MLP of up to four dense layers, its softmax / value head
//                                 (softmax_rule.h, by_actions) and the search's "value the leaves" step in one launch: 16 rows per block,
//                                 activations and weight tiles in LDS, every output's sum one float64 chain in index order (mlp_rule.h: the
//                                 rule per output and per row, host and device)
//   k_mlp_grad.hip  k_mlp_grad_rows / chunk / reduce   the backward pass of that network, to one flat gradient of every weight and bias: the
//                                 activations recomputed by mlp_dev.h's layer loop and parked, the deltas downward with 16 rows per block,
//                                 then the sums over the batch as float64 chains per chunk of rows and over the chunks, in a stated order
//                                 (mlp_grad_rule.h: the rule per step, host and device)
//   k_adam.hip      k_adam_sumsq / k_adam_update / k_mlp_lerp   the optimiser step of that network from the flat gradient: the sum of
//                                 squares by batch_sum.h's butterfly per wave, then, with every block redoing the second stage from the
//                                 partials, the clip, Adam and the target's slow copy per parameter, written where the parameters lie
//                                 (adam_rule.h: the rule per parameter, host and device); the only kernels that write a snac_mlp's arrays
//   k_policy_roll.hip  k_policy_rollout   T ticks of observe -> network -> draw -> step in one launch: a block of 256 threads owns 16 envs,
//                                 their K image (wave 0: lane = env, as k_rollout) and their activations in LDS (mlp_dev.h: the layer loop,
//                                 for this unit and k_mlp.hip; policy_dev.h: the draw of snac_policy_act, for this unit and k_policy.hip)
//   snac_hip.hip    the C ABI of include/snac_hip.h and the dispatch: choose() decides kernel, size and form from one table of thresholds
//                   (KNOBS), launch() calls the launcher choose() named
//   snac_traj.hip   trajectory memory
// The env records are read from HBM once per launch, kept on chip for all T steps, written back once.  Rollout outputs are [T][N][D]
// or, with SNAC_OBS_TILED, tile-major [N / 64][T][64][D].
#pragma once
#include "snac_dev.h"

namespace snac_detail {
// which kernel the calling thread's last launch went to (snac_last_kernel())
extern thread_local const char* g_kernel;

// ---- host side, defined in snac_hip.hip
int check_layout(const snac_env_desc* d);
int base_obs_dim(int kind);
int tail_len(int kind, int tail);
int check_common(const snac_env_desc* d, const snac_state* st);   // ends with check_state_align
int check_state_align(const snac_state* st);                      // for the entry points that take a state without check_common
KArgs make_args(const snac_env_desc* d, const snac_state* st);
// the checks of the node-pool entry points (kind: the record's kind), defined in k_nodes.hip
int nodes_check(int kind, const snac_env_desc* d, const snac_state* st, const void* nodes, int32_t pool_rows, int32_t m);
// the checks the self-play and Reanalyse entry points share (num_actions, stats, B, cap, B * (cap + 1) rows), defined in k_uct_play.hip
int play_check(int A, const void* stats, int32_t rows, int32_t B, int32_t cap);
// the checks of a network descriptor (non-null, layers, dims, pointers and their alignment), defined in k_mlp.hip
int mlp_net_check(const snac_mlp* net);
// the checks of the entry points on rows of inputs (mlp_net_check, x non-null and aligned as its type, x_is_f64, rows), defined in k_mlp.hip
int mlp_check(const snac_mlp* net, const void* x, int x_is_f64, int32_t rows);
// ---- the dispatch, defined in snac_hip.hip.  choose() is the whole decision, a pure function of its arguments and tune(): the kernel, its
// size parameter E where it has several (tile size of the tile kernels; envs per block of k_rollout2db / 2dt / 1dt; envs per wave of
// k_step2d; edges per wave of k_transition2d; else 0) and its form where it has them (k_step2d / k_step3dq / k_step1d / k_rollout1dl:
// bit 0 non-temporal record loads, bit 1 non-temporal row stores; else 0).  launch() names the kernel for snac_last_kernel() and calls
// its launcher.  tests/native/dispatch_table.cpp pins choose() over a grid of calls against tests/golden/dispatch_table.txt, on the host.
enum Kernel { K_ROLLOUT, K_TRANSITION, K_AUX, K_RESET, K_IOU, K_STEP1D, K_STEP2D, K_STEP3D, K_STEP3DS, K_STEP3DQ, K_EDGES1D, K_EDGES2D, K_EDGES3D,
              K_TRANSITION2D, K_TRANSITION3D, K_ROLLOUT1DL, K_ROLLOUT1DT, K_ROLLOUT2D, K_ROLLOUT2DB, K_ROLLOUT2DT, K_ROLLOUT3D, K_ROLLOUT3DB, K_COUNT };
struct Choice { Kernel kernel; int E; int form; };
Choice choose(Op op, const snac_env_desc* d, const KArgs& a);
int launch(Op op, const snac_env_desc* d, const KArgs& a, void* stream);

// ---- the launch functions of the kernel families, each defined beside its kernels.  They launch what choose() decided (E, form: the
// fields of its Choice) and read no knob; what they still pick follows from the call's data alone (explicit actions, record outputs,
// identity rows, the row-length classes of the 1D layout variants)
void launch_tile1d(Op op, bool dyn, int E, int obs_dtype, const KArgs& a, hipStream_t s);      // k_tile1d.hip
void launch_tile2d(Op op, bool dyn, int E, int obs_dtype, const KArgs& a, hipStream_t s);      // k_tile2d.hip
void launch_tile3d(Op op, bool dyn, int E, int obs_dtype, const KArgs& a, hipStream_t s);      // k_tile3d.hip
void launch_roll2d(const snac_env_desc* d, const KArgs& a, hipStream_t s);                     // k_roll2d.hip
void launch_roll2db(const snac_env_desc* d, const KArgs& a, int E, hipStream_t s);             // k_roll2db.hip
void launch_roll2dbv(const snac_env_desc* d, const KArgs& a, int E, hipStream_t s);            // k_roll2dbv.hip: k_rollout2db for the layout variants
void launch_roll2dt(const snac_env_desc* d, const KArgs& a, int E, hipStream_t s);             // k_roll2dt.hip
void launch_roll1dt(const snac_env_desc* d, const KArgs& a, int E, hipStream_t s);             // k_roll1dt.hip
void launch_roll1dl(const snac_env_desc* d, const KArgs& a, int form, hipStream_t s);          // k_roll1dl.hip
void launch_roll3d(const snac_env_desc* d, const KArgs& a, hipStream_t s);                     // k_roll3d.hip
void launch_roll3db(const snac_env_desc* d, const KArgs& a, hipStream_t s);                    // k_roll3db.hip
void launch_roll3dbv(const snac_env_desc* d, const KArgs& a, hipStream_t s);                   // k_roll3dbv.hip: k_rollout3db for the layout variants
void launch_step1d(const snac_env_desc* d, const KArgs& a, int form, hipStream_t s);           // k_step1d.hip
void launch_aux1d(const snac_env_desc* d, const KArgs& a, hipStream_t s);                      // k_step1d.hip
void launch_edges1d(const snac_env_desc* d, const KArgs& a, hipStream_t s);                    // k_step1d.hip
void launch_step2d(const snac_env_desc* d, const KArgs& a, int E, int form, hipStream_t s);    // k_step.hip
void launch_aux2d(const snac_env_desc* d, const KArgs& a, hipStream_t s);                      // k_step.hip
void launch_step3d(const snac_env_desc* d, const KArgs& a, bool span, hipStream_t s);          // k_step.hip (span: k_step3ds)
void launch_step3dq(const snac_env_desc* d, const KArgs& a, int form, hipStream_t s);          // k_step3dq.hip
void launch_aux3d(const snac_env_desc* d, const KArgs& a, hipStream_t s);                      // k_step3dq.hip
void launch_trans2d(const snac_env_desc* d, const KArgs& a, int E, hipStream_t s);             // k_trans.hip
void launch_edges2d(const snac_env_desc* d, const KArgs& a, hipStream_t s);                    // k_trans.hip
void launch_trans3d(const snac_env_desc* d, const KArgs& a, hipStream_t s);                    // k_trans.hip
void launch_edges3d(const snac_env_desc* d, const KArgs& a, hipStream_t s);                    // k_trans.hip
void launch_reset(const snac_env_desc* d, const KArgs& a, hipStream_t s);                      // k_reset.hip
void launch_iou(const snac_env_desc* d, const KArgs& a, hipStream_t s);                        // k_reset.hip

// the four (dynamic, row type) instantiations a launcher chooses among: f(std::bool_constant<DYN>(), OT()) with OT = float / double
template <typename F>
void by_rows(const snac_env_desc* d, F f) {
    const bool f32 = d->obs_dtype == SNAC_OBS_F32;
    if (d->dynamic != 0) { if (f32) f(std::true_type(), float()); else f(std::true_type(), double()); }
    else { if (f32) f(std::false_type(), float()); else f(std::false_type(), double()); }
}

// the three action counts the units on rows of A scores are instantiated for: returns f(std::integral_constant<int, A>()), or the
// refusal of any other count
template <typename F>
int by_actions(int num_actions, F f) {
    switch (num_actions) {
        case 3: return f(std::integral_constant<int, 3>());
        case 5: return f(std::integral_constant<int, 5>());
        case 8: return f(std::integral_constant<int, 8>());
        default: return fail(SNAC_ERR_UNSUPPORTED, "num_actions must be 3, 5 or 8");
    }
}
}  // namespace snac_detail
