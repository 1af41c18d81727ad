/*
 * snac_hip.h -- C ABI of libsnac_hip.so: the MI355X (gfx950) batched mobile-construction simulator.
 *
 * Drop-in boundary for the env hot path of ai4ce/SNAC.  The reference has no FFI or plugin registry:
 * its "operator API" for this path is the Python class surface
 *     deep_mobile_printing_{1d1r,2d1r,3d1r}.reset()/step()/iou()
 *       Env/1D/DMP_Env_1D_static.py:66-151            Env/1D/DMP_Env_1D_dynamic_usedata_plan.py:40-133
 *       Env/2D/DMP_Env_2D_static.py:54-154            Env/2D/DMP_Env_2D_dynamic_usedata_plan.py:34-147
 *       Env/3D/DMP_simulator_3d_static_circle.py:67-276
 *       Env/3D/DMP_simulator_3d_dynamic_triangle_usedata.py:45-277
 *     VectorizedEnvWrapper.reset()/step()  multiprocess.py:15-32   and its driver loop multiprocess.py:78-84
 * which snac_amd/ re-exports under the same module and class names on top of the entry points below
 * (binding stubs: INTEGRATION.md).  Each entry point names the reference code it replaces.
 *
 * Conventions
 *   - Plain C types only.  Every pointer inside snac_state and every array argument is a DEVICE pointer
 *     owned by the caller (e.g. torch tensors).  The env entry points allocate nothing and keep no state of their own
 *     beyond a thread-local error string; the exceptions are the optional trajectory-memory allocator
 *     (snac_traj_alloc / snac_traj_free below), which keeps a mutex-protected table of the blocks it has handed out, and the
 *     table of action distributions (snac_action_dist).
 *     Input and output ARRAYS (actions, step sizes, obs, reward, done) may also lie in
 *     page-locked host memory, which is mapped into the device's address space: the kernels then read / write them over the
 *     bus themselves and a host-side caller only waits (snac_stream_sync) -- no copy command.
 *   - All work is enqueued on the caller's hipStream_t (`stream`, passed as void*; NULL = default
 *     stream), asynchronously, without host synchronisation.
 *   - Return value: SNAC_OK or a negative snac_status; snac_last_error() describes the last failure on
 *     the calling thread.
 *   - One process per GPU; envs are independent, so multi-GPU use shards envs by `env_id_base`.
 *
 * State layout in HBM (N = num_envs, all arrays env-major so one wavefront reads one env's record with
 * unit-stride lanes):
 *   hdr      snac_env_hdr[N]      16-byte packed scalars (one dwordx4 per env)
 *   episode  int32[N]             number of resets performed - 1
 *   grid     1D: int16[N][32]     heights of the 30 interior cells (2 pad); frame cells are implicit -1
 *            2D: uint32[N][20]    occupancy bit-board, row i = interior row i, bit j = interior col j
 *            3D: int16[N][400]    heights of the 20x20 interior, row-major
 *   plans    1D: int16[P][32]  2D: uint32[P][20]  3D: int16[P][400]   (interior cells, same indexing)
 *   plan_tb  int16[P]             total_brick of each plan (2D: after the floor of 30)
 *   stats    int64[N] x 3         finished episodes, sum of their integer returns, sum of
 *                                 llrint(IoU * 2^40) at episode end
 * The -1 frame of the reference's environment_memory is a pure function of the coordinates and is
 * never stored.  Interior values are exactly the reference's (2D cells are {0,1} after every step).
 *
 * Counter RNG (used when `actions` / `step_size` / plan indices are not supplied explicitly)
 *   mix32(x): x^=x>>16; x*=0x7feb352d; x^=x>>15; x*=0x846ca68b; x^=x>>16          (32-bit wrap-around)
 *   key(seed,stream) = mix32(lo32(seed) ^ mix32(hi32(seed) + 0x9E3779B9*(stream+1)))
 *   e0 = mix32(key ^ mix32(lo32(env) + 0x85EBCA6B*hi32(env) + 0x1B873593))
 *   e1 = mix32((key + 0x27D4EB2F) ^ mix32((lo32(env) ^ 0x165667B1) + 0xC2B2AE35*hi32(env)))
 *   word(seed,stream,env,t) = mix32(mix32(e0 ^ (0x9E3779B9*t)) + e1)
 *   stream 0 (per env, tick t):     action = ((word>>16) * num_actions) >> 16
 *                                   step_size = 1 + (((word & 0xffff) * 3) >> 16)
 *     with an action distribution (snac_env_desc.action_dist != 0, a handle of snac_action_dist): A = num_actions,
 *     thresholds cdf[0 .. A-2], nondecreasing, each in [0, 65536], u = word >> 16:
 *                                   action = #{ j < A-1 : u >= cdf[j] }
 *                                   (action j has probability (cdf[j] - cdf[j-1]) / 65536, cdf[-1] = 0, cdf[A-1] = 65536)
 *     and the step size as above.  The uniform table cdf[j] = ceil(65536 * (j+1) / A) draws exactly the actions of the
 *     multiply: floor(u * A / 65536) counts the j >= 1 with u * A >= 65536 * j, i.e. u >= ceil(65536 * j / A).
 *   stream 1 (per env, episode e):  plan_idx = (word * num_plans) >> 32
 *   stream 2 (per plan row):        the plan generator (snac_make_plans with vertices NULL)
 *   stream 3 (per env, move t):     the move a self-play search samples from its root's visits (snac_uct_pick_moves):
 *                                   u = (word * total) >> 32, action = the lowest a with N_0 + ... + N_a > u
 *   stream 4 (per sample, draw d):  the entry a prioritised-replay tree draws (snac_prio_sample; "Prioritised replay" below):
 *                                   r = (word(.., 2 * d) << 32) | word(.., 2 * d + 1), keyed by sampler_id + j for sample j of a call
 *   stream 5 (per env, tick t):     the action a policy's scores give (snac_policy_act; "Acting from a policy" below): categorical
 *                                   u = (word * total) >> 32 over integer weights, epsilon-greedy from word >> 16 and word & 0xffff
 *   stream 6 (per root slot, move t): the Gamma draws of the Dirichlet root noise (snac_explore_root_dirichlet; "Exploration noise" below)
 *   stream 7 (per root slot, move t): the Gumbel noise of the root scores (snac_explore_gumbel_scores; there)
 *   env = env_id_base + local index, so results do not depend on how envs are sharded over GPUs.  The node-pool entry points key edge /
 *   leaf i of a call by env_id_base + i; a search with K paths per tree hands them its B * K slots with env_id_base * K in the descriptor,
 *   so that slot k of tree b draws with (env_id_base + b) * K + k, its slot in the search over all envs ("K paths per tree" below).
 */
#ifndef SNAC_HIP_H
#define SNAC_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNAC_ABI_VERSION 12

typedef enum snac_status {
    SNAC_OK = 0,
    SNAC_ERR_ARG = -1,         /* bad argument (null pointer, unknown kind, size mismatch) */
    SNAC_ERR_HIP = -2,         /* a HIP call failed; message holds hipGetErrorString */
    SNAC_ERR_UNSUPPORTED = -3
} snac_status;

enum { SNAC_ENV_1D = 1, SNAC_ENV_2D = 2, SNAC_ENV_3D = 3 };
enum { SNAC_OBS_F64 = 0, SNAC_OBS_F32 = 1 };
enum { SNAC_OBS_NONE = 0, SNAC_OBS_ALL = 1, SNAC_OBS_LAST = 2, SNAC_OBS_TILED = 3 };
enum { SNAC_FLAG_NEED_RESET = 1 };   /* snac_env_hdr.flags: the last step returned done */
/* snac_env_desc.rules: the termination tests of the env copies under script/PPO (and script/Rainbow/env/Env2D.py:166), which
 * write `>` where the canonical classes write `>=`:
 *   SNAC_RULE_BRICK_GT  done when count_brick > total_brick   (script/PPO/1d_dynamic/DMP_Env_1D_dynamic_usedata_plan.py:93,
 *                       script/PPO/2d_static/DMP_Env_2D_static.py:137, script/PPO/3d_static/DMP_simulator_3d_static_circle.py:205)
 *   SNAC_RULE_TIME_GT   done when count_step > total_step     (script/PPO/3d_static/DMP_simulator_3d_static_circle.py:221) */
enum { SNAC_RULE_BRICK_GT = 1, SNAC_RULE_TIME_GT = 2 };
/* Observation-layout variants of the reference's env copies, as flags of the same kernels (snac_env_desc.frame_value /
 * obs_scalars / obs_tail).  A row of `obs` is then   [window, scalar, scalar | position | plan | record]   with
 * snac_obs_dim(desc) values; every kernel that writes observations (reset, step, rollout, transition, observe) honours them.
 *   frame_value   value shown for the frame cells of the window (and by snac_export_grid): -1 (0 is read as -1), or 2 --
 *                 Env/2D/DMP_Env_2D_static_Lnet.py:61-64 fills the frame with 2.  1D / 2D only (the 3D rules test -1).
 *   obs_scalars   SNAC_SCALARS_RAW: count_brick, count_step; SNAC_SCALARS_NORM: count_brick/total_brick,
 *                 count_step/total_step; SNAC_SCALARS_DEFAULT: raw for dynamic == 0, normalised for dynamic == 1 (the
 *                 canonical classes).  The L-Net 2D class normalises with a static plan (DMP_Env_2D_static_Lnet.py:75);
 *                 the env copies under script/PPO return raw counters with dataset plans
 *                 (script/PPO/2d_dynamic/DMP_Env_2d_dynamic_usedata_plan.py:70-71).
 *   obs_tail      bit set, appended in this order:
 *     SNAC_TAIL_POSITION  1D: position (Env/1D/DMP_Env_1D_static_Lnet.py:83 -> 8 values); 2D / 3D: row, col
 *     SNAC_TAIL_PLAN      the env's plan, 1D: 30 heights, 2D / 3D: input_plan 20x20 row-major -- the flat observation of
 *                         script/PPO/{1d,2d,3d}_dynamic (37 / 451 values)
 *     SNAC_TAIL_RECORD    8 values: reward, done, pos_r, pos_c, count_brick, count_step, total_brick, plan_idx of the env
 *                         after the step -- everything a single-env caller reads back, in ONE row (one D2H copy).  A row
 *                         written outside a step (snac_reset, also for the envs its mask leaves alone; snac_observe)
 *                         reports reward 0 and done = the env's pending-reset flag */
enum { SNAC_SCALARS_DEFAULT = 0, SNAC_SCALARS_RAW = 1, SNAC_SCALARS_NORM = 2 };
enum { SNAC_TAIL_POSITION = 1, SNAC_TAIL_PLAN = 2, SNAC_TAIL_RECORD = 4 };

/* constants of one env kind: the reference's __init__ blocks (Env/1D/DMP_Env_1D_static.py:7-29,
 * Env/2D/DMP_Env_2D_dynamic_usedata_plan.py:7-32, Env/3D/DMP_simulator_3d_static_circle.py:8-40,
 * Env/3D/DMP_simulator_3d_dynamic_triangle_usedata.py:7-43) */
typedef struct snac_sizes {
    int32_t obs_dim;          /* state_dim: 7 / 51 / 51 */
    int32_t num_actions;      /* action_dim: 3 / 5 / 8 */
    int32_t total_step;       /* 750 / 600 / 1300 (3D static) or 1000 (3D dynamic) */
    int32_t half_window;      /* HALF_WINDOW_SIZE: 2 / 3 / 3 */
    int32_t env_height, env_width;     /* 1 x 34 / 26 x 26 */
    int32_t plan_height, plan_width;   /* 1 x 30 / 20 x 20 */
    int32_t grid_elems, grid_elem_bytes;   /* per-env record of snac_state.grid */
    int32_t plan_elems, plan_elem_bytes;   /* per-plan record of snac_state.plans */
} snac_sizes;

typedef struct snac_env_hdr {   /* 16 bytes, 16-byte aligned */
    int8_t  pos_r, pos_c;       /* position_memory[-1] in bordered coordinates (1D: pos_r, pos_c = 0) */
    uint8_t flags;              /* SNAC_FLAG_* */
    uint8_t reserved;
    int16_t count_brick, count_step, total_brick, plan_idx;
    int16_t ep_return;          /* integer return of the running episode (rewards are integers) */
    int16_t cross;              /* 3D: running sum of min(height, plan) over the interior (numerator of iou()) */
} snac_env_hdr;

typedef struct snac_env_desc {
    int32_t kind;               /* SNAC_ENV_* */
    int32_t dynamic;            /* 0: static-plan class (obs scalars cb, cs); 1: *_usedata class (cb/tb, cs/T) */
    int32_t num_envs;           /* N on this GPU */
    int32_t num_plans;          /* P rows in plans / plan_tb */
    int32_t obs_dtype;          /* SNAC_OBS_F64 (reference dtype) or SNAC_OBS_F32 (= (float) of the f64 value) */
    int32_t static_plan;        /* plan row used by resets when dynamic == 0 or no plan index is supplied */
    uint64_t seed;              /* counter-RNG seed */
    int64_t env_id_base;        /* global id of local env 0 */
    int32_t total_step;         /* time limit, at most 3000; 0 = the class constant (750 / 600 / 1300 static 3D / 1000 dynamic 3D).
                                   The 3D L-Net variant runs the dynamic rules with 1300
                                   (Env/3D/DMP_simulator_3d_static_circle_Lnet.py:28) */
    int32_t rules;              /* SNAC_RULE_* bits; 0 = the canonical classes */
    int32_t frame_value;        /* 0 / -1: the canonical -1; 2: the 2D L-Net frame (1D / 2D only) */
    int32_t obs_scalars;        /* SNAC_SCALARS_* */
    int32_t obs_tail;           /* SNAC_TAIL_* bits */
    int32_t action_dist;        /* 0: uniform counter-RNG actions; else a handle of snac_action_dist registered for the kind's
                                   num_actions: the distribution of the actions the counter RNG draws (explicit actions are
                                   unaffected) */
} snac_env_desc;

/* Alignment of the state arrays.  The kernels read the caller's arrays with wide and with scalar loads, whatever kernel the dispatch
 * picks, so each array of snac_state starts at an address that is a multiple of (bytes):
 *     hdr            16    one int4 per env
 *     episode         4    natural
 *     grid           16    records read and written as 16-byte pieces (uint4)
 *     plans          16    rows read as 16-byte pieces (uint4) and through the scalar cache
 *     plan_tb         4    fetched as the aligned 32-bit word that holds the row (the half by row & 1)
 *     stat_episodes   8    natural
 *     stat_return     8    natural
 *     stat_iou_fx     8    natural
 * Every entry point that takes a snac_state tests these before any HIP call and refuses a state that breaks one: SNAC_ERR_ARG,
 * "snac_state.plan_tb must be 4-byte aligned".  A precondition, not a dispatch condition: no kernel is chosen by it.  Whatever an allocator
 * returns (hipMalloc, a torch tensor) meets all of them; a caller that packs its state into one allocation, or passes a slice of a table
 * (plan_tb + k), has to keep them itself -- a slice of plan_tb starts at an even row.
 * plan_tb's word read: for an odd num_plans the word of the last row also covers the two bytes after the array.  They lie inside the same
 * aligned 4-byte word as the row (so on the same page: the read cannot fault), their value is never used, and nothing is written there.
 * The per-element inputs of the entry points -- mask, plan_idx_in, actions, step_size, src_index, dst_index -- may sit at the natural
 * alignment of their element type (1, 2, 1, 1, 4, 4 bytes); where an output or another array needs more, its entry point says so. */
typedef struct snac_state {
    snac_env_hdr* hdr;          /* [N] */
    int32_t* episode;           /* [N] */
    void* grid;                 /* [N][grid_elems] */
    const void* plans;          /* [P][plan_elems] */
    const int16_t* plan_tb;     /* [P] */
    int64_t* stat_episodes;     /* [N] */
    int64_t* stat_return;       /* [N] */
    int64_t* stat_iou_fx;       /* [N] */
} snac_state;

int snac_version(void);
const char* snac_last_error(void);
/* name of the kernel the calling thread's last launch through this library went to ("k_rollout2d", "k_step3d", "k_rollout" for
 * the tile kernels, ...): diagnostics -- which of the specialised kernels a call took depends on batch size, alignment, layout and
 * the tuning switches, and a measurement should name what it measured (bench.py's roofline.kernel) */
const char* snac_last_kernel(void);
/* the dispatch table: one line "ENV_VARIABLE=value  # what it decides" per batch-size threshold / switch that selects a kernel
 * (effective values: the defaults measured on the build pool, or their environment overrides); tools/retune.py re-measures them */
int snac_tuning(char* out, int32_t cap);

/* Register an action distribution for the counter RNG ("Counter RNG" above): the num_actions - 1 thresholds cdf[], nondecreasing,
 * each in [0, 65536].  *handle (>= 1) is what snac_env_desc.action_dist takes.  The entries live in a process-wide table (mutex-
 * protected, entries immutable, handles process-local); registering the same table again returns the same handle.  SNAC_ERR_ARG
 * for num_actions outside 2 .. 8, invalid thresholds, or a full table (1024 distinct entries).  No device is needed. */
int snac_action_dist(int32_t num_actions, const uint32_t* cdf, int32_t* handle);

/* constants of (kind, dynamic); replaces the attribute reads of the reference constructors */
int snac_env_sizes(int kind, int dynamic, snac_sizes* out);

/* values per observation row for this descriptor: obs_dim of the kind plus its obs_tail (8 for the 1D L-Net class,
 * 451 for the PPO 2D / 3D dataset classes); negative snac_status on a bad descriptor */
int snac_obs_dim(const snac_env_desc* desc);

/* reset(): Env/2D/DMP_Env_2D_dynamic_usedata_plan.py:34-66 and the five sibling reset()s;
 * VectorizedEnvWrapper.reset / reset_at (multiprocess.py:20-23).
 *   mask        uint8[N] or NULL: reset env i iff mask[i] != 0 (NULL = all)
 *   plan_idx_in int16[N] or NULL: plan row per env (the reference's index_random / sequential index);
 *               NULL = counter RNG stream 1 when dynamic, desc->static_plan otherwise
 *   obs         [N][obs_dim] of obs_dtype or NULL: observation of every env after the call */
int snac_reset(const snac_env_desc* desc, const snac_state* st, const uint8_t* mask, const int16_t* plan_idx_in,
               void* obs, void* stream);

/* step(): Env/2D/DMP_Env_2D_dynamic_usedata_plan.py:85-147 and siblings, for all N envs
 * (VectorizedEnvWrapper.step, multiprocess.py:24-32), fused with observation_/_get_obs and the reward.
 *   t           tick: index of this vector step (keys the counter RNG)
 *   actions     int8[N] or NULL (counter RNG);  step_size int8[N] in {1,2,3} or NULL (counter RNG) --
 *               the value the reference draws with np.random.randint(1, 4) at the top of step()
 *   auto_reset  != 0: an env whose previous step returned done is reset first (plan from the counter RNG)
 *   obs [N][obs_dim] or NULL, reward float[N] or NULL, done uint8[N] or NULL
 * Actions outside [0, num_actions) only advance count_step (the reference raises).  Explicit step sizes are clamped into
 * {1,2,3} -- the only values the reference's randint(1, 4) produces -- so that no input can move an agent off the plan area. */
int snac_step(const snac_env_desc* desc, const snac_state* st, uint32_t t, const int8_t* actions,
              const int8_t* step_size, int auto_reset, void* obs, float* reward, uint8_t* done, void* stream);

/* snac_step with ONE action and ONE step size for every env, passed by value -- the call of a single-env caller
 * (the drop-in classes: env.step(action) with the step size the host drew from np.random, N = 1): no host-to-device
 * copy precedes the launch; with SNAC_TAIL_RECORD the whole result comes back in one row.  action: any int (values outside
 * [0, num_actions) only advance count_step); step_size is clamped into {1,2,3}. */
int snac_step_scalar(const snac_env_desc* desc, const snac_state* st, uint32_t t, int32_t action, int32_t step_size,
                     int auto_reset, void* obs, float* reward, uint8_t* done, void* stream);

/* snac_reset of every env onto plan row `plan_idx`, passed by value (the single-env caller's reset()) */
int snac_reset_scalar(const snac_env_desc* desc, const snac_state* st, int32_t plan_idx, void* obs, void* stream);

/* Block the calling thread until everything enqueued on `stream` has finished (hipStreamSynchronize).  The single-env caller's
 * read-back: `obs` of snac_step_scalar / snac_reset_scalar may point into page-locked host memory (hipHostMalloc, a pinned
 * torch tensor: mapped into the GPU's address space), the kernel then stores its row there itself and this wait is all that
 * separates the launch from reading it -- env.step(action) -> (obs, reward, done) of the reference classes
 * (Env/2D/DMP_Env_2D_dynamic_usedata_plan.py:85-147) as one launch and one wait, no copy command. */
int snac_stream_sync(void* stream);

/* Trajectory memory (optional; every entry point takes any device pointer).  The reference has no counterpart: its driver
 * loop (multiprocess.py:78-84) drops each step's arrays.  On MI355X the physical address space behaves as slices of 32 GiB:
 * write streams confined to one slice reach ~5.7 TB/s, spread over two or more ~7.1 (tools/wr_blocks.hip).
 * A hipMalloc block of 16 GB is one physical run, inside one slice unless it happens to straddle a boundary.  A block from here
 * is ONE contiguous virtual range backed -- through the HIP virtual-memory API -- by 32 MB chunks of physical memory from
 * different slices taking turns, so the [T][N][obs_dim] output of snac_rollout keeps two slices busy at any time: the headline
 * pass takes 2.33-2.40 ms instead of 2.75-2.95 (tools/mem_ab.py).  Which slice a chunk lies in cannot be asked of the driver; it
 * is measured: groups of 16 handles are timed together with a reference group under the rollout's own store pattern -- partners
 * in another slice run 20 % faster -- and the block alternates chunks of the two kinds.
 *   snac_traj_alloc_ex  `bytes` (rounded up to whole 32 MB handles, or 2 MB pages below that; blocks under 1 GiB are one plain
 *                     run) on `device`, read / write for that device; *out is an ordinary device pointer, contiguous, 2 MB-
 *                     aligned.  pool_cap_bytes: how much device memory the measurement may hold BEYOND the block while it runs
 *                     (0 = 64 GiB).  The pool starts at the block + 8 GiB and grows in steps of 8 GiB only until both kinds of
 *                     chunk are there in sufficient number; it never takes more than half of what is free next to the block nor
 *                     the last 4 GiB, and is released before the call returns.  With too little room, or without a usable
 *                     measurement, the block falls back to three runs created 32 GiB apart.  stream: the probe kernels, the
 *                     check and their waits run on this stream (NULL = the default stream); the call returns when they are done.
 *                     How a measured block is built (round 4): the probe writes the headline rollout's own store shape (a wave's
 *                     26 112-byte tile per step, 16 bytes per lane, 1 KiB per store instruction, 1024 waves); the block is a
 *                     sequence of 1 GiB WINDOWS, each the 16 chunks of a group from the reference's slice and the 16 chunks of a
 *                     group from another slice taking turns, and every window is timed as that pair BEFORE it is used (a pair
 *                     that misses the fast level is taken apart); the mapped block is then timed again, EVERY window and once as
 *                     a whole, and rebuilt from a larger pool (twice at most) if a window runs like a single slice.  What was
 *                     measured stays with the block: snac_traj_describe.
 *                     Every block is also CHECKED before it is handed out: a pattern written by one kernel is read back by
 *                     another and, one word per chunk, by a copy.  A block that fails its check is SNAC_ERR_HIP, never a silent
 *                     retry.  Typically 0.1-1 s for the headline's 16 GB.  SNAC_ERR_HIP when memory runs out.
 *                     SNAC_TRAJ_PROBE=0 skips the measurement, SNAC_TRAJ_DEBUG=1 prints it.
 *   snac_traj_alloc   the same with the default pool cap on the default stream.
 *   snac_traj_free    waits for the whole device to go idle (hipDeviceSynchronize: no kernel may still be writing the block),
 *                     unmaps and releases the block's memory.  Its address range stays reserved and is never handed out again (a
 *                     recycled range has been seen to serve stale translations, tools/vmm_stale.hip; a stale pointer faults instead
 *                     of hitting someone else's data): every block of 1 GiB or more costs its own size plus its probe ranges in
 *                     ADDRESS SPACE for the life of the process -- no memory; 47 bits last for more than a thousand headline-sized
 *                     blocks; snac_traj_reserved_bytes() says how much is held that way.  NULL is a no-op; a pointer that did not
 *                     come from snac_traj_alloc is SNAC_ERR_ARG.  (The Python wrapper frees a block when the last tensor viewing
 *                     it dies, so the device-wide wait can come from a garbage collection.)
 * The caller owns the block; the library keeps only what it needs to unmap and to describe it. */
int snac_traj_alloc_ex(size_t bytes, int device, size_t pool_cap_bytes, void* stream, void** out);
int snac_traj_alloc(size_t bytes, int device, void** out);
int snac_traj_free(void* ptr);
/* how a live block of snac_traj_alloc is backed (diagnostics): one of the values below, or SNAC_ERR_ARG for any other pointer */
#define SNAC_TRAJ_ONE_RUN 1      /* below 1 GiB: handles in creation order */
#define SNAC_TRAJ_THREE_RUNS 2   /* the fallback: three runs created 32 GiB apart, chunk j -> run j % 3 */
#define SNAC_TRAJ_MEASURED 3     /* windows of 1 GiB: chunks of the reference group's slice and of another slice in turn, every
                                    window timed as the pair it is */
int snac_traj_layout(const void* ptr);
/* what the allocator measured while it built a live block (all times in microseconds per GiB written under the rollout's store
 * shape; zeros for the layouts that are not measured).  A caller -- bench.py's `placement` -- can tell from this alone whether the
 * block it was given runs at the two-slice level: windows_slow == 0 and block_us_per_gib close to fast_us_per_gib. */
#define SNAC_TRAJ_INFO_WINDOWS 64
typedef struct snac_traj_info {
    int32_t layout;                  /* SNAC_TRAJ_* */
    int32_t rebuilds;                /* measured blocks built and thrown away before this one (0 .. 2) */
    int32_t pool_groups;             /* 512 MB groups the pool held when the block was assembled */
    int32_t probe_launches;          /* launches of the probe kernel for this block (the last attempt) */
    int32_t windows;                 /* 1 GiB windows timed in the finished block */
    int32_t windows_slow;            /* of those: above 1.08 x fast_us_per_gib (0 unless the last rebuild still had one) */
    float self_us_per_gib;           /* the reference group written as a pair with itself: the scale the classes are judged on */
    float fast_us_per_gib;           /* median over the partners in another slice than the reference */
    float slow_us_per_gib;           /* median over the partners in the reference's slice */
    float window_max_us_per_gib;     /* the finished block: its slowest window ... */
    float window_mean_us_per_gib;    /* ... the mean over its windows ... */
    float block_us_per_gib;          /* ... and all of it in one launch */
    float build_ms;                  /* wall time of the whole snac_traj_alloc call */
    uint64_t bytes;                  /* mapped size */
    float window_us[SNAC_TRAJ_INFO_WINDOWS];   /* the first 64 windows, in address order */
} snac_traj_info;
int snac_traj_describe(const void* ptr, snac_traj_info* out);
/* address space (bytes) of ranges this process has unmapped and keeps reserved (see snac_traj_free) */
uint64_t snac_traj_reserved_bytes(void);

/* the driver loop of multiprocess.py:78-84 -- T vector steps with auto-reset, fused in one launch with the
 * env state held on chip.
 *   actions / step_size   int8[T][N] or NULL (counter RNG, ticks t0 .. t0+T-1)
 *   obs_mode              SNAC_OBS_ALL: obs is [T][N][obs_dim]; SNAC_OBS_LAST: obs is [N][obs_dim] and
 *                         receives the last step only; SNAC_OBS_NONE: obs ignored; SNAC_OBS_TILED: every observation, tile-major --
 *                         obs is [ceil(N / 64)][T][64][obs_dim], the row of (t, env) at ((env / 64) * T + t) * 64 + env % 64: each
 *                         tile of 64 envs streams through its own contiguous region instead of jumping N rows per step
 *                         (the build's own layout for trajectories that stay on the GPU: up to 7.1 instead of 6.0 TB/s of
 *                         writes where the tensor lies well; the envs of a ragged last tile beyond N
 *                         are not written)
 *   reward float[T][N] or NULL, done uint8[T][N] or NULL */
int snac_rollout(const snac_env_desc* desc, const snac_state* st, int32_t T, uint32_t t0, const int8_t* actions,
                 const int8_t* step_size, int obs_mode, void* obs, float* reward, uint8_t* done, void* stream);

/* snac_rollout that also records, per env-step, what a replay memory needs besides obs / reward / done (SURVEY.md
 * section 8 row f1): the action taken and the step size used (useful when they come from the counter RNG), the plan
 * row in effect, and whether the step was the first of its episode.  Every member is [T][N] or NULL. */
typedef struct snac_rollout_record {
    int8_t* actions;
    int8_t* step_size;
    int16_t* plan_idx;
    uint8_t* first;
} snac_rollout_record;
int snac_rollout_rec(const snac_env_desc* desc, const snac_state* st, int32_t T, uint32_t t0, const int8_t* actions,
                     const int8_t* step_size, int obs_mode, void* obs, float* reward, uint8_t* done,
                     const snac_rollout_record* rec, void* stream);

/* snac_rollout_rec with SNAC_OBS_TILED into a RING of `ring_ticks` steps: obs is [ceil(N / 64)][ring_ticks][64][obs_dim] and this
 * launch writes the steps first_tick .. first_tick + T - 1 of it (first_tick + T <= ring_ticks; the caller splits a wrap into
 * two launches).  reward / done / rec stay [T][N] (the caller passes the ring's own slices).  The tile-major replay ring of
 * snac_amd.ReplayRing(layout="tiled"): a tile of 64 envs streams through its own contiguous region of the ring. */
int snac_rollout_tiled(const snac_env_desc* desc, const snac_state* st, int32_t T, uint32_t t0, const int8_t* actions,
                       const int8_t* step_size, int32_t ring_ticks, int32_t first_tick, void* obs, float* reward, uint8_t* done,
                       const snac_rollout_record* rec, void* stream);

/* Minibatch assembly for the replay memory of the DQN / DRQN scripts (store_memory / learning_process,
 * script/DQN/2d/DQN_2d_dynamic.py:122-124,145-166): the tuples (s, a, r, s', plan) are not stored, they are gathered from
 * the rollout output ring  obs_ring[cap][N][obs_dim] (obs_dtype)  filled by snac_rollout(_rec) with SNAC_OBS_ALL:
 *   s'   = obs_ring[tick][env]
 *   s    = obs_ring[tick-1 mod cap][env], or the reset observation when first_ring[tick][env] != 0
 *   plan = the env's input_plan (2D / 3D: 20x20, 1D: 30 heights) expanded from the plan table
 * for `batch` samples (tick_idx[b], env_idx[b]); outputs are float32 as the scripts feed them to the networks:
 * s_out / s_next_out [batch][obs_dim], plan_out [batch][400 | 30] or NULL (2D / 3D: 16-byte aligned, it is written four cells at a time).  a, r, done are plain gathers of the [cap][N]
 * arrays and stay with the caller. */
int snac_replay_gather(const snac_env_desc* desc, const snac_state* st, int32_t cap, const void* obs_ring,
                       const uint8_t* first_ring, const int16_t* plan_idx_ring, const int32_t* tick_idx,
                       const int32_t* env_idx, int32_t batch, float* s_out, float* s_next_out, float* plan_out,
                       void* stream);
/* the same from a tile-major ring obs_ring[ceil(N / 64)][cap][64][obs_dim] (filled by snac_rollout_tiled); first_ring and
 * plan_idx_ring stay [cap][N] */
int snac_replay_gather_tiled(const snac_env_desc* desc, const snac_state* st, int32_t cap, const void* obs_ring,
                             const uint8_t* first_ring, const int16_t* plan_idx_ring, const int32_t* tick_idx,
                             const int32_t* env_idx, int32_t batch, float* s_out, float* s_next_out, float* plan_out,
                             void* stream);

/* n-step transitions and episode windows: walks along one env's column of the ring from a sample (t, i), bounded by the episode flags
 * and by the ring's ends, one launch each.  first_ring / done_ring (uint8), reward_ring (float32), action_ring (int8) and plan_idx_ring
 * are the [cap][N] arrays snac_rollout_rec fills; obs_ring is [cap][N][obs_dim], or with tiled != 0 the tile-major ring of
 * snac_replay_gather_tiled.  slot(k) = (t + k) mod cap.  "The tuple of a step" is snac_replay_gather's: s' is the step's own row, s the
 * previous slot's row or the reset observation when first is set; the same row lengths are supported (the base row plus the position
 * tail, else SNAC_ERR_UNSUPPORTED), outputs are float32, indices are clamped into range, plan_out may be NULL (2D / 3D: 16-byte aligned).
 * action_out is int64 and done_out / mask_out are bytes 0 / 1.  Every argument is checked before any HIP call (cap >= 2, batch >= 0, n / L
 * in [1, 64], newest / oldest in [0, cap), gamma finite, no null array); batch == 0 returns SNAC_OK without a launch.  No host
 * synchronisation.
 *
 * snac_replay_gather_nstep (Rainbow's multi-step memory): newest = (head - 1) mod cap, the slot written last.  Take steps k = 0, 1, ...
 * and stop after step k when  done_ring[slot(k)] != 0,  or k + 1 == n,  or slot(k) == newest,  or first_ring[slot(k + 1)] != 0 (an
 * episode that ended without done, e.g. a ring attached after a reset).  m = k + 1 steps were taken, 1 <= m <= n.  Per sample:
 *   s_out, action_out   those of step 0                          s_next_out   the row of step m - 1
 *   done_out            done_ring[slot(m - 1)] != 0              steps_out    m
 *   return_out          g = 0.0 (double); for k = m - 1 down to 0: g = (double)reward_ring[slot(k)] + gamma * g, product and sum each
 *                       rounded (no fused multiply-add); then (float)g
 *   discount_out        d = 1.0 (double); m times d = d * gamma; (float)d, or 0.0f when done_out
 *   plan_out            the plan row at step 0
 * The caller's target is return + discount * max_a Q(s_next).  With n = 1 every output is snac_replay_gather's tuple of (t, i), with
 * return == reward and discount == (float)gamma or 0.
 *
 * snac_replay_gather_windows (DRQN's Memory.get_batch): the window ENDS at (t, i).  oldest = (head - valid_ticks) mod cap, the oldest
 * addressable transition (its predecessor row is still in the ring).  Start with len = 1 and extend to the earlier step while
 * len < L,  the window's earliest step is not at oldest,  the earliest step has first == 0  and the step before it has done == 0.
 * Outputs are [batch][L][..]: position j < len holds the tuple of step (t - len + 1 + j) mod cap -- s_out, s_next_out, action_out,
 * reward_out, done_out -- and positions j >= len are zero in every output; mask_out[b][j] = j < len, length_out[b] = len (int32).  Valid
 * steps come first, so a recurrent net starts from its zero state at the window's real start.  plan_out [batch][400 | 30]: the plan row at
 * the window's last step.  The len + 1 distinct rows of a window are read once each (consecutive tuples chain: s[j + 1] == s_next[j]).
 * With L = 1 this is snac_replay_gather's tuple again. */
int snac_replay_gather_nstep(const snac_env_desc* desc, const snac_state* st, int32_t cap, int32_t tiled, const void* obs_ring,
                             const uint8_t* first_ring, const uint8_t* done_ring, const float* reward_ring, const int8_t* action_ring,
                             const int16_t* plan_idx_ring, int32_t newest, const int32_t* tick_idx, const int32_t* env_idx, int32_t batch,
                             int32_t n, double gamma, float* s_out, float* s_next_out, float* plan_out, int64_t* action_out,
                             float* return_out, float* discount_out, uint8_t* done_out, int32_t* steps_out, void* stream);
int snac_replay_gather_windows(const snac_env_desc* desc, const snac_state* st, int32_t cap, int32_t tiled, const void* obs_ring,
                               const uint8_t* first_ring, const uint8_t* done_ring, const float* reward_ring, const int8_t* action_ring,
                               const int16_t* plan_idx_ring, int32_t oldest, const int32_t* tick_idx, const int32_t* env_idx, int32_t batch,
                               int32_t L, float* s_out, float* s_next_out, float* plan_out, int64_t* action_out, float* reward_out,
                               uint8_t* done_out, uint8_t* mask_out, int32_t* length_out, void* stream);

/* ---- On-policy rollouts (the reference's script/PPO; snac_amd/onpolicy.py: RolloutBuffer; k_onpolicy.hip, k_replay.hip): generalised
 * advantage estimation over a span of the ring, and a PPO minibatch in one launch.
 *
 * snac_gae: reward, done, value, adv and ret are [cap][N].  The span is the `count` slots from `first`, taken modulo cap as in
 * snac_uct_returns: slot(j) = (first + j) mod cap, j < count; slot(count - 1) is the newest.  value[slot][i] is the critic's value of the
 * observation env i acted on in that slot; bootstrap[i] is the value of env i's current observation, after the newest slot (NULL: zeros).
 * Per env i, from the newest slot back to the oldest, in float64:
 *     c = gamma * lambda            (rounded once, before the loop)
 *     nv = bootstrap[i]; a = 0.0
 *     for each slot, newest first:
 *         r, v, d = reward, value, done != 0
 *         delta = (r + (d ? 0.0 : gamma * nv)) - v
 *         a     = delta + (d ? 0.0 : c * a)
 *         adv[slot][i] = (float)a;  ret[slot][i] = (float)(a + v);  nv = v
 * Every product, sum and difference is rounded on its own (no fused multiply-add).  done cuts both the bootstrap and the trace: an episode
 * end is terminal, as in the reference's PPO2 (there is no separate time-limit flag).  Slots outside the span are not written.  adv and ret
 * must not alias reward, done, value or bootstrap, or each other (documented, not checked).  Checks, all before any HIP call: N >= 1,
 * cap >= 1, first in [0, cap), count in [0, cap], gamma and lambda finite, no null among reward / done / value / adv / ret; count == 0
 * returns SNAC_OK without a launch.  No host synchronisation.
 *
 * snac_replay_gather_onpolicy: per sample (t, i) = (tick_idx[b], env_idx[b]), clamped into range,
 *   s_out       the observation acted on: snac_replay_gather's s (the previous slot's row, or the reset observation when
 *               first_ring[t][i] != 0); there is no s_next
 *   plan_out    the plan row as in snac_replay_gather, [batch][400 | 30]; may be NULL (2D / 3D: 16-byte aligned)
 *   action_out  (int64) action_ring[t][i];  value_out, logp_out, ret_out: the float32 entries at [t][i] of their rings
 *   adv_out     adv_ring[t][i], or with norm != NULL (two floats on the device, {mean, rstd}) (adv - mean) * rstd in float32, difference
 *               and product each rounded
 * The conventions are snac_replay_gather_nstep's: tiled != 0 is the tile-major obs_ring, both ring dtypes, the same row lengths (the base
 * row plus the position tail, else SNAC_ERR_UNSUPPORTED), every argument checked before any HIP call (cap >= 2, batch >= 0, no null ring,
 * index or output array but plan_out, plan_out needs plan_idx_ring), batch == 0 returns SNAC_OK without a launch, no host synchronisation. */
#define SNAC_GAE_CHUNK 16 /* slots whose loads snac_gae's kernel issues together (a span's chunk boundaries, for the tests) */
int snac_gae(int32_t N, int32_t cap, int32_t first, int32_t count, double gamma, double lambda, const float* reward, const uint8_t* done,
             const float* value, const float* bootstrap, float* adv, float* ret, void* stream);
int snac_replay_gather_onpolicy(const snac_env_desc* desc, const snac_state* st, int32_t cap, int32_t tiled, const void* obs_ring,
                                const uint8_t* first_ring, const int16_t* plan_idx_ring, const int8_t* action_ring, const float* value_ring,
                                const float* logp_ring, const float* adv_ring, const float* ret_ring, const float* norm,
                                const int32_t* tick_idx, const int32_t* env_idx, int32_t batch, float* s_out, float* plan_out,
                                int64_t* action_out, float* value_out, float* logp_out, float* adv_out, float* ret_out, void* stream);

/* ---- Acting from a policy (snac_amd/batched.py: sample_actions / epsilon_greedy; snac_amd/onpolicy.py: act_logits; k_policy.hip): one
 * action per env from a row of A = num_actions float32 scores (a policy's logits, or Q-values), in one launch, drawn from counter-RNG stream
 * 5 so that a trained run does not depend on how its envs are sharded.  The model-free counterpart of snac_uct_pick_moves: the choice is
 * made in integers.
 *
 * snac_policy_act: scores is [N][A], A the num_actions of desc->kind, rows contiguous, the base aligned as a float (a slice of a tensor
 * will do).  Env i of the call draws with  w = word(desc->seed, 5, desc->env_id_base + i, t).  Per row, s_a = scores[i][a]:
 *     m    = s_0; for a = 1 .. A-1: if (s_a > m) m = s_a                    (float compares; m is the largest score)
 *     bad  = some s_a is a NaN or +inf, or m is -inf (every score -inf).  A bad row is drawn in every mode as if all its scores were 0
 *            (m = 0 too), and adds one to bad_rows[0] (int32 on the device, an atomic add; bad_rows may be NULL).
 *     g    = the lowest a with s_a == m                                     (the greedy action; +0 and -0 tie)
 *   mode SNAC_POLICY_CATEGORICAL (softmax sampling).  In float64, every product, sum, difference and quotient rounded on its own (no fused
 *   multiply-add), sums in index order starting from 0.0:
 *     x_a   = (double)s_a - (double)m                      e_a = EXP(x_a)
 *     w_a   = (uint64)floor(e_a * 2^28)                    (exactly 2^28 for a = g; 0 for s_a = -inf or x_a below about -19.4)
 *     total = w_0 + ... + w_{A-1}   (<= 2^31)              u = ((uint64)w * total) >> 32
 *     action = the lowest a with w_0 + ... + w_a > u       (an action of weight 0 is never drawn)
 *     S     = e_0 + ... + e_{A-1}                          T = sum of (e_a == 0 ? 0.0 : e_a * x_a)
 *     logp[i]    = (float)(x_action - LOG(S))
 *     entropy[i] = (float)(LOG(S) - T / S)
 *   mode SNAC_POLICY_GREEDY: action = g.
 *   mode SNAC_POLICY_EPS_GREEDY: eps = epsilon_per_env ? epsilon_per_env[i] : epsilon (Ape-X's per-actor epsilons);
 *     v = floor((double)eps * 65536.0); eps_fx = v >= 65536 ? 65536 : v > 0 ? (uint32)v : 0   (a NaN gives 0)
 *     action = (w >> 16) < eps_fx ? ((w & 0xffff) * A) >> 16 : g
 *   logp and entropy are defined by the categorical mode only and must be NULL in the other two.
 * EXP and LOG are these sequences of float64 operations, not a library's (each line's operations rounded one by one, left to right as
 * parenthesised; constants in C's hexadecimal notation):
 *     LOG2E = 0x1.71547652b82fep+0   LN2_HI = 0x1.62e42feep-1   LN2_LO = 0x1.a39ef35793c76p-33     (k * LN2_HI is exact for |k| < 2^20)
 *   EXP(x), x <= 0:  0.0 when x < -45.0 (also -inf: below 2^-53, it would not change S); else
 *     k = rint(x * LOG2E)  (ties to even)      r = (x - k * LN2_HI) - k * LN2_LO              (|r| < 0.3466)
 *     p = c_13; for n = 12 down to 0: p = p * r + c_n,   c_n = 1.0 / n!  (n! is exact in float64; the quotient rounded)
 *     EXP = ldexp(p, (int)k)                   (exact: no subnormal for k >= -65)
 *   LOG(S), 1 <= S <= 8:
 *     f, e = frexp(S)  (S = f * 2^e, 0.5 <= f < 1);  if f < 0x1.6a09e667f3bcdp-1 (sqrt 1/2): f = f * 2.0, e = e - 1
 *     z = (f - 1.0) / (f + 1.0);  z2 = z * z   (|z| < 0.1716)
 *     q = d_10; for n = 9 down to 0: q = q * z2 + d_n,   d_n = 1.0 / (2 n + 1)
 *     LOG = (double)e * LN2_HI + ((2.0 * z) * q + (double)e * LN2_LO)
 *   Both stay within 1e-12 (absolute) of the exact functions over x in [-45, 0] and S in [1, 8]; the truncated series leave less than 5e-18.
 *   LOG holds the same bound over S in [1, 64], where snac_c51_loss uses it (frexp takes the exponent, the series sees f alone).
 * Outputs: action int8[N], logp float[N], entropy float[N]; each may be NULL, and with all three NULL nothing is launched.  The kernel never
 * writes an action outside [0, A), reads scores only and writes nothing but the outputs given and bad_rows[0].
 * Checks, all before any HIP call: desc and scores non-null, desc->kind one of SNAC_ENV_*, N >= 1, mode one of the three, epsilon finite and
 * in [0, 1] (every mode), epsilon_per_env NULL unless the mode is SNAC_POLICY_EPS_GREEDY, logp and entropy NULL unless it is
 * SNAC_POLICY_CATEGORICAL.  desc->num_envs is not read: N is the number of rows.  No host synchronisation. */
enum { SNAC_POLICY_CATEGORICAL = 0, SNAC_POLICY_GREEDY = 1, SNAC_POLICY_EPS_GREEDY = 2 };
int snac_policy_act(const snac_env_desc* desc, int32_t N, uint32_t t, int32_t mode, const float* scores, double epsilon,
                    const float* epsilon_per_env, int8_t* action, float* logp, float* entropy, int32_t* bad_rows, void* stream);

/* ---- Distributional targets (the reference's script/Rainbow; snac_amd/distributional.py: CategoricalSupport; k_dist.hip): the expected
 * values of categorical (C51) value distributions, the greedy / double-DQN choice of the next action, and the projection of the
 * distributional TD target onto the support, each in one launch and by a rule that restates in numpy byte for byte: no atomics on
 * floats, every sum in a stated order.
 *
 * Support: K = atoms, 2 <= K <= 64, vmin < vmax, both finite.  dz = (vmax - vmin) / (double)(K - 1), computed once on the host in double;
 * z_i = vmin + (double)i * dz.  All arithmetic below is float64, and every product, sum, difference and quotient is rounded on its own (no
 * fused multiply-add).  Distributions are float32, [B][A][K] with A = num_actions (3, 5 or 8, else SNAC_ERR_UNSUPPORTED), contiguous, the
 * base aligned as a float (a row is 204 bytes at K = 51).
 *
 * The expected value E(p) of a row p[0..K):
 *     x_j = (double)p_j * z_j for j < K, x_j = 0.0 for K <= j < 64
 *     for s = 32, 16, 8, 4, 2, 1:  x_j = x_j + x_{j+s} for every j < s     (all j of a step together: a shuffle-down tree, lane = atom)
 *     E(p) = x_0
 * snac_c51_expect: q[b][a] = (float)E(p[b][a]); q is [B][A].
 *
 * snac_c51_project, per sample b:
 *   The choice.  q_a = E(p_select[b][a]), with p_select = p_next when it is NULL (double DQN gives the online network's distributions as
 *   p_select and the target network's as p_next).  best = q_0, a_star = 0; for a = 1 .. A-1: if (q_a > best) { best = q_a; a_star = a; }.
 *   So ties go to the lowest index, a NaN never wins, and no input gives an a_star outside [0, A).  q_star[b] = (float)E(p_next[b][a_star]).
 *   The projection.  r = (double)ret[b], d = (double)discount[b], p_i = (double)p_next[b][a_star][i], acc[0..K) = 0.0.
 *   For i = 0 .. K-1, in this order:
 *     t = r + d * z_i;   t = t < vmin ? vmin : t;   t = t > vmax ? vmax : t
 *     pos = (t - vmin) / dz;   l = min((int)floor(pos), K - 1);   f = pos - (double)l
 *     if l == K - 1:  acc[l] = acc[l] + p_i
 *     else:           acc[l] = acc[l] + p_i * (1.0 - f);  then  acc[l+1] = acc[l+1] + p_i * f
 *   m[b][j] = (float)acc[j].  (The l, l + 1, fraction form of the textbook's floor / ceil projection: it needs none of its l == u repairs
 *   and stays within 2^-24 of it.)  The rule fixes the order of the additions into each acc[j] -- i ascending, within one i the lower term
 *   first -- not how a kernel finds them.
 *   Bad samples.  A sample whose ret or discount is not finite, or whose discount < 0, gets a row m[b] of zeros, a_star[b] = 0,
 *   q_star[b] = 0 and adds one to bad_rows[0] (int32 on the device, an atomic add).  Probabilities are not checked: a NaN in p_next shows
 *   in m (and in q_star); it never indexes anything.
 * Outputs: m float[B][K]; a_star int8[B], q_star float[B] and bad_rows may each be NULL and are then not written.  The kernels read their
 * inputs only and write nothing but the outputs given.  Checks, all before any HIP call: p (p_next), ret, discount, m (q) non-null,
 * B >= 1, atoms in [2, 64], vmin and vmax finite with vmin < vmax, num_actions 3, 5 or 8.  No host synchronisation. */
int snac_c51_expect(int32_t B, int32_t num_actions, int32_t atoms, double vmin, double vmax, const float* p, float* q, void* stream);
int snac_c51_project(int32_t B, int32_t num_actions, int32_t atoms, double vmin, double vmax, const float* p_next, const float* p_select,
                     const float* ret, const float* discount, float* m, int8_t* a_star, float* q_star, int32_t* bad_rows, void* stream);

/* ---- Soft values (discrete SAC) (the reference's script/SAC; snac_amd/sac.py: SoftValue; k_soft.hip, soft_rule.h): the three losses of
 * discrete SAC are functions of one softmax of the policy's logits and one elementwise minimum of two critics over A = num_actions values
 * per sample.  One launch gives the soft state value, the TD target, the entropy and the gradient of the actor loss with respect to the
 * logits, by a rule that restates in numpy byte for byte; the entropy is snac_policy_act's, the same bytes.
 *
 * Inputs per sample b: logits[b][A], q1[b][A] and q2[b][A] (q2 may be NULL: one critic), float32, rows contiguous, every base aligned as
 * a float (a slice of a tensor will do); ret[b] and discount[b], float32, read only for y; alpha[0], one float32 on the device (the
 * temperature is a learned parameter; no host synchronisation).  A = 3, 5 or 8, else SNAC_ERR_UNSUPPORTED.
 * All arithmetic is float64, every product, sum, difference and quotient rounded on its own (no fused multiply-add), sums in index order
 * starting from 0.0; EXP and LOG are the sequences of "Acting from a policy".  With l_a = logits[b][a]:
 *     m      = l_0; for a = 1 .. A-1: if (l_a > m) m = l_a                     (float compares, as snac_policy_act)
 *     x_a    = (double)l_a - (double)m             e_a = EXP(x_a)
 *     S      = e_0 + ... + e_{A-1}                 T = sum of (e_a == 0 ? 0.0 : e_a * x_a)            L = LOG(S)
 *     live_a = e_a != 0                            (not live: l_a = -inf, or more than 45 below the largest -- a masked action)
 *     pi_a   = e_a / S                             lp_a = x_a - L
 *     qm_a   = (double)(q2 && q2_a < q1_a ? q2_a : q1_a)                       (a float compare; a NaN in q2 never wins)
 *     al     = (double)alpha[0]
 *     d_a    = live_a ? qm_a - al * lp_a : 0.0
 *     V      = sum of (live_a ? pi_a * d_a : 0.0)
 *     v[b]       = (float)V
 *     y[b]       = (float)((double)ret[b] + (double)discount[b] * V)
 *     entropy[b] = (float)(L - T / S)
 *     grad[b][a] = live_a ? (float)(scale * (pi_a * (V - d_a))) : 0.0f         (scale: e.g. 1.0 / B for the mean over a minibatch)
 *   grad is the derivative with respect to the logits of the actor loss J = sum_a pi_a (al * log pi_a - qm_a) = -V, with qm and al held
 *   constant: dJ/dl_j = pi_j ((al * lp_j - qm_j) - J) = pi_j (V - d_j) (DESIGN.md section 3.10 derives it).
 *   Masked actions.  A q-value at a masked action is never read into a sum: a NaN there does not show, and grad there is exactly 0.
 *   A q-value that is not finite at a live action shows in that sample's v, y and grad as the rule's operations carry it (a NaN, or an
 *   infinity); which NaN is not part of the rule.  It never indexes anything.
 *   Bad samples.  A sample is bad if some l_a is a NaN or +inf or every l_a is -inf; if y is asked for and ret or discount is not finite
 *   or discount < 0; or if alpha[0] is read (below) and is not finite or negative -- then every sample of the call is bad.  A bad sample
 *   gets v = y = entropy = 0, a row of zeros in grad, and adds one to bad_rows[0] (int32 on the device, an atomic add).
 * Outputs: v float[B], y float[B], entropy float[B], grad float[B][A] and bad_rows may each be NULL and are then not written; with v, y,
 * entropy and grad all NULL nothing is launched.  With v, y and grad all NULL (the entropy alone) q1, q2 and alpha are not read and may
 * be NULL; otherwise q1 and alpha are required.  ret and discount are required when y is given and must be NULL when it is not.  The
 * kernel reads its inputs only and writes nothing but the outputs given.
 * Checks, all before any HIP call: logits non-null, B >= 1, scale finite, the pointers as just stated, num_actions 3, 5 or 8.  No host
 * synchronisation. */
int snac_soft_value(int32_t B, int32_t num_actions, const float* logits, const float* q1, const float* q2, const float* alpha,
                    const float* ret, const float* discount, double scale, float* v, float* y, float* entropy, float* grad,
                    int32_t* bad_rows, void* stream);

/* ---- PPO loss (the reference's script/PPO) (stable-baselines PPO2's update; snac_amd/ppo.py: PPOLoss; k_ppo.hip, ppo_rule.h): the
 * clipped surrogate, the (clipped) value loss and the entropy bonus of a minibatch, the mean of their sum, its gradient with respect to
 * the logits and to the value in closed form, and PPO2's diagnostics (approximate KL, clip fraction), in one call of two launches.  Every
 * sum over the batch is a float64 sum in the order stated below, so that two runs, and numpy, give the same bytes.
 *
 * Inputs per sample i: logits[i][A], logp_old[i], adv[i], value[i], value_old[i], ret[i], float32, rows contiguous, every base aligned
 * as a float (a slice of a tensor will do); action[i], int64 (what snac_replay_gather_onpolicy writes), 8-byte aligned.  A = 3, 5 or 8,
 * else SNAC_ERR_UNSUPPORTED.  Parameters: clip > 0; clip_vf (negative: the value function is not clipped and value_old must be NULL;
 * >= 0: PPO2's cliprange_vf, and value_old is required); vf_coef, ent_coef; scale (e.g. 1.0 / B for the gradient of the mean).
 * All arithmetic is float64, every product, sum, difference and quotient rounded on its own (no fused multiply-add), sums in index order
 * starting from 0.0; EXP and LOG are the sequences of "Acting from a policy".  With l_a = logits[i][a]:
 *     m, x_a, e_a, S, T, L = LOG(S), live_a, pi_a = e_a / S, lp_a = x_a - L      exactly as in "Soft values (discrete SAC)"
 *     H      = L - T / S                                                         (snac_policy_act's entropy, the same bytes)
 *     lp     = lp_action                                (the taken action's; picked by compares, never by an index into memory)
 *     d      = lp - (double)logp_old      clamped = |d| > 20.0      dc = d < -20.0 ? -20.0 : d > 20.0 ? 20.0 : d
 *     r      = dc <= 0 ? EXP(dc) : 1.0 / EXP(-dc)                                (EXP keeps its stated domain x <= 0)
 *     lo     = 1.0 - clip, hi = 1.0 + clip  (once per call)                      rc = r < lo ? lo : r > hi ? hi : r
 *     s1     = r * adv, s2 = rc * adv      Lpi = -(s2 < s1 ? s2 : s1)            g = (!(s2 < s1) && !clamped) ? -(adv * r) : 0.0
 *     dv     = value - ret
 *     clip_vf < 0:   Lv = 0.5 * (dv * dv), gv = dv
 *     clip_vf >= 0:  u = value - value_old, uc = u < -clip_vf ? -clip_vf : u > clip_vf ? clip_vf : u, dc2 = (value_old + uc) - ret,
 *                    q1 = dv * dv, q2 = dc2 * dc2;  q2 > q1 ? (Lv = 0.5 * q2, gv = (u == uc ? dc2 : 0.0)) : (Lv = 0.5 * q1, gv = dv)
 *     kl     = 0.5 * (dc * dc)      clipped = |r - 1.0| > clip                   (PPO2's approxkl and clipfrac, per sample)
 *     total  = (Lpi + vf_coef * Lv) - ent_coef * H
 *     loss[i]           = (float)total
 *     grad_logits[i][a] = live_a ? (float)(scale * (g * ((a == action ? 1.0 : 0.0) - pi_a) + ent_coef * (pi_a * (lp_a + H)))) : 0.0f
 *     grad_value[i]     = (float)(scale * (vf_coef * gv))
 *   g is dLpi/dlp, and dlp/dl_a = (a == action) - pi_a, dH/dl_a = -pi_a (lp_a + H); gv is dLv/dvalue.  action, logp_old, adv, ret and
 *   value_old are constants of the loss.  Where |d| > 20 the ratio stands at e^(+-20) and carries no gradient.  On a clip boundary
 *   (r == lo or hi, or u == +-clip_vf) the gradient is the unclipped side's.
 *   Bad samples.  A sample is bad if some l_a is a NaN or +inf or every l_a is -inf; if action is outside [0, A) or the taken action has
 *   no weight (e_action == 0: masked, or more than 45 below the largest); or if logp_old, adv, value, ret -- or value_old, when
 *   clip_vf >= 0 -- is not finite.  A bad sample gets loss = grad_value = 0 and a row of zeros in grad_logits, contributes 0.0 to every
 *   sum below, and adds one to bad_rows[0] (int32 on the device, an atomic add).
 *   The statistics.  Every sample has eight contributions u[0..8) = total, Lpi, Lv, H, kl, clipped ? 1.0 : 0.0, 1.0, clamped ? 1.0 : 0.0
 *   (all 0.0 for a bad sample).  The order of their sums is part of this interface.  Stage 1, per wave w of 64 consecutive samples
 *   (the last one filled up with 0.0):
 *       for off = 32, 16, 8, 4, 2, 1:  u_j = u_j + u_{j ^ off} for every j < 64 (all j of a step together);   partials[w][k] = u_0
 *     -- in numpy: u = u[:, :h] + u[:, h:] for h = 32, 16, 8, 4, 2, 1.  Stage 2, with W = ceil(B / 64) waves:
 *       t_j = 0.0; for w = j, j + 64, j + 128, ... < W: t_j = t_j + partials[w][k]      (j < 64; increasing w)
 *       then the same butterfly over t_0 .. t_63, and sum_k = t_0.
 *     stats[k] = sum_k / (double)B for k < 6: the means over B of total, Lpi, Lv, H and kl, and the clip fraction (bad samples count
 *     in B and add nothing); stats[6] = sum_6, the number of good samples; stats[7] = sum_7, the number of clamped ones.
 *     mean_loss[0] = (float)stats[0].
 * Outputs: loss float[B], grad_logits float[B][A], grad_value float[B], mean_loss float[1] and bad_rows may each be NULL and are then not
 * written.  stats double[SNAC_PPO_STATS] may be NULL: then nothing is reduced and the second launch does not happen (mean_loss must be
 * NULL too).  stats needs partials: ceil(B / 64) * SNAC_PPO_STATS doubles of caller-owned scratch, 8-byte aligned as stats is; its
 * contents after the call are stage 1's rows.  With every output NULL nothing is launched.  The kernels read their inputs only and write
 * nothing but the outputs given and partials.
 * Checks, all before any HIP call: logits, action, logp_old, adv, value, ret non-null; B >= 1; clip finite and > 0; clip_vf, vf_coef,
 * ent_coef and scale finite; value_old given exactly when clip_vf >= 0; partials with stats, stats with mean_loss; the 8-byte
 * alignments; num_actions 3, 5 or 8.  Both launches go on `stream`; no host synchronisation. */
#define SNAC_PPO_STATS 8
int snac_ppo_loss(int32_t B, int32_t num_actions, const float* logits, const int64_t* action, const float* logp_old, const float* adv,
                  const float* value, const float* value_old, const float* ret, double clip, double clip_vf, double vf_coef, double ent_coef,
                  double scale, float* loss, float* grad_logits, float* grad_value, double* stats, float* mean_loss, double* partials,
                  int32_t* bad_rows, void* stream);

/* ---- Q-learning losses (the reference's script/DQN, script/DRQN and script/Rainbow, and SAC's critics; snac_amd/qloss.py: TDLoss;
 * k_qloss.hip, td_rule.h): the temporal-difference loss of a minibatch of Q-values -- the greedy or double-DQN target, the squared or
 * Huber error, the importance weights of prioritised replay, the mean -- with its gradient with respect to q in closed form, the new
 * priorities |td| and the batch statistics, in one call of two launches.  The conventions are "PPO loss"'s: all arithmetic is float64,
 * every product, sum, difference and quotient rounded on its own (no fused multiply-add); rows contiguous, every base aligned as a
 * float; action int64, 8-byte aligned; A = num_actions is 3, 5 or 8, else SNAC_ERR_UNSUPPORTED.
 *
 * snac_td_loss.  Inputs per sample b: q[b][A] float32 and action[b]; then exactly one of two target modes.  Mode Y: y[b] float32, a
 * target computed elsewhere (snac_soft_value's y for SAC's critics); q_next, q_select, ret and discount are NULL.  Mode NEXT:
 * q_next[b][A] (the target network's values of s_next), ret[b], discount[b] (mb["return"], mb["discount"] of an n-step sample, or the
 * reward and gamma * (1 - done)) and optionally q_select[b][A] (the online network's values of s_next: double DQN; NULL: q_next
 * itself); y is NULL.  weight[b] float32, the importance weights, may be NULL.  delta: 0 gives the squared error of
 * torch.nn.functional.mse_loss, > 0 gives huber_loss(delta=).  scale: e.g. 1.0 / B for the gradient of the mean.
 *     qa   = q[b][action]                       (picked by compares over a = 0 .. A-1, never by an index into registers or memory)
 *     NEXT:  s = q_select ? q_select[b] : q_next[b];  best = s_0, a_star = 0; for a = 1 .. A-1: if (s_a > best) { best = s_a; a_star = a; }
 *            (float compares: ties go to the lowest index, a NaN never wins)           qn = (double)q_next[b][a_star]
 *            yv = (double)ret[b] + (double)discount[b] * qn
 *     Y:     yv = (double)y[b]
 *     td   = (double)qa - yv                    ab = |td|
 *     delta == 0:  L = td * td                                                        g = 2.0 * td                        lin = false
 *     delta  > 0:  lin = ab > delta;  L = lin ? delta * (ab - 0.5 * delta) : 0.5 * (td * td);   g = lin ? (td < 0 ? -delta : delta) : td
 *     w    = weight ? (double)weight[b] : 1.0   total = w * L
 *     loss[b] = (float)L        priority[b] = (float)ab        y_out[b] = (float)yv
 *     grad_q[b][a] = a == action ? (float)(scale * (w * g)) : 0.0f                    (the whole row is written)
 *     u[0..8) = total, L, ab, qa, yv, lin ? 1.0 : 0.0, 1.0, w
 *   g is dL/dqa; the target, the weight and the action are constants of the loss.  loss is the unweighted error and priority the new
 *   priority of prioritised replay (snac_prio_update takes it as it is).  The casts are plain: a |td| beyond float32's range shows as inf.
 *   Bad samples.  A sample is bad if action is outside [0, A); if qa is not finite; in mode NEXT if ret or discount is not finite,
 *   discount < 0, or qn is not finite; in mode Y if y is not finite; or if weight is given and is not finite or negative.  A bad sample
 *   gets zeros in every per-sample output, contributes 0.0 to every u, and adds one to bad_rows[0] (int32 on the device, an atomic add).
 *   A Q-value at an action that is neither taken nor chosen is never read into anything: a NaN there does not show.
 *   The statistics.  The two stages of "PPO loss", in its order, over the eight contributions u: partials[w][k] of the waves of 64
 *   consecutive samples, then the sums.  stats[k] = sum_k / (double)B for k != 6: the mean weighted loss, the mean loss, the mean |td|,
 *   the mean Q taken, the mean target, Huber's linear fraction, and (k = 7) the mean weight; stats[6] = sum_6, the number of good
 *   samples.  mean_loss[0] = (float)stats[0].
 * Outputs: loss, priority, y_out float[B], grad_q float[B][A], mean_loss float[1] and bad_rows may each be NULL and are then not written.
 * stats double[SNAC_Q_STATS] may be NULL: then nothing is reduced and the second launch does not happen (mean_loss must be NULL too).
 * stats needs partials: ceil(B / 64) * SNAC_Q_STATS doubles of caller-owned scratch, 8-byte aligned as stats is.  With every output NULL
 * nothing is launched.  The kernels read their inputs only and write nothing but the outputs given and partials.
 * Checks, all before any HIP call: q and action non-null; B >= 1; exactly one of y and (q_next, ret, discount) -- all three -- given,
 * q_select only with them; delta finite and >= 0; scale finite; partials with stats, stats with mean_loss; the 8-byte alignments;
 * num_actions 3, 5 or 8.  Both launches go on `stream`; no host synchronisation.
 *
 * snac_c51_loss (Rainbow's cross-entropy; snac_amd/distributional.py: CategoricalSupport.loss).  Inputs per sample b: logits[b][A][K]
 * float32, the raw output of the network (no softmax), K = atoms in [2, 64]; action[b]; m[b][K] float32, the row snac_c51_project writes;
 * weight[b] float32 or NULL; scale.  TREE(v) is the shuffle-down tree of "Distributional targets" over v_0 .. v_63 with v_j = 0.0 for
 * j >= K:  for s = 32, 16, 8, 4, 2, 1: v_j = v_j + v_{j+s} for every j < s (all j of a step together); TREE(v) = v_0.  EXP and LOG are
 * the sequences of "Acting from a policy"; LOG is used here over [1, 64] and stays within 1e-12 of the exact logarithm there as well
 * (its frexp takes any exponent; the series does not see it).  With l_j = logits[b][action][j]:
 *     mx  = the largest l_j (float)              x_j = (double)l_j - (double)mx         e_j = EXP(x_j)
 *     S   = TREE(e)   (1 <= S <= K)              T = TREE(e_j == 0 ? 0.0 : e_j * x_j)   Lg = LOG(S)
 *     lp_j = x_j - Lg      p_j = e_j / S         mj = (double)m[b][j]
 *     ce  = -TREE(mj * lp_j)                     M = TREE(mj)                           H = Lg - T / S
 *     w   = weight ? (double)weight[b] : 1.0     total = w * ce
 *     loss[b] = (float)ce                                              (unweighted: it is the new priority of prioritised replay)
 *     grad[b][a][j] = a == action ? (float)(scale * (w * (M * p_j - mj))) : 0.0f        for every a < A, j < K (the whole block is written)
 *     u[0..8) = total, ce, H, M, 0.0, 0.0, 1.0, w
 *   d ce / d l_j = M p_j - mj, since d lp_i / d l_j = (i == j) - p_j; m, the weight and the action are constants.
 *   Bad samples.  A sample is bad if action is outside [0, A) -- nothing is read through such an action --; if some l_j or m_j with j < K
 *   is not finite; or if weight is given and is not finite or negative.  A bad sample gets loss 0, a block of zeros in grad, zeros in u,
 *   and adds one to bad_rows[0].
 *   The statistics: as snac_td_loss's, over these u: stats = the mean weighted loss, the mean loss, the mean entropy of the online
 *   distribution of the action taken, the mean target mass, 0, 0, the number of good samples (not divided), the mean weight.
 * Outputs: loss float[B], grad float[B][A][K], mean_loss float[1] and bad_rows may each be NULL; stats, partials and mean_loss as above.
 * Checks, all before any HIP call: logits, action and m non-null; B >= 1; atoms in [2, 64]; scale finite; partials with stats, stats with
 * mean_loss; the 8-byte alignments; num_actions 3, 5 or 8.  Both launches go on `stream`; no host synchronisation. */
#define SNAC_Q_STATS 8
int snac_c51_loss(int32_t B, int32_t num_actions, int32_t atoms, const float* logits, const int64_t* action, const float* m, const float* weight,
                  double scale, float* loss, float* grad, double* stats, float* mean_loss, double* partials, int32_t* bad_rows, void* stream);
int snac_td_loss(int32_t B, int32_t num_actions, const float* q, const int64_t* action, const float* y, const float* q_next,
                 const float* q_select, const float* ret, const float* discount, const float* weight, double delta, double scale,
                 float* loss, float* priority, float* y_out, float* grad_q, double* stats, float* mean_loss, double* partials,
                 int32_t* bad_rows, void* stream);

/* ---- Search loss (AlphaZero / Gumbel self-play) (snac_amd/search_loss.py: SearchLoss; k_search.hip, search_rule.h): the loss of a
 * minibatch of self-play positions -- the cross-entropy of the network's policy to the search's distribution pi (the visit distribution,
 * or the improved policy of the Gumbel search), the squared or Huber error of its value to the return z, the importance weights of
 * prioritised replay, the mean -- with its gradient with respect to the logits and the value in closed form, the new priorities
 * |value - z| and the batch statistics, in one call of two launches.  The conventions are "PPO loss"'s: all arithmetic is float64, every
 * product, sum, difference and quotient rounded on its own (no fused multiply-add), sums in index order starting from 0.0; rows
 * contiguous, every base aligned as a float; A = num_actions is 3, 5 or 8, else SNAC_ERR_UNSUPPORTED.  EXP and LOG are the sequences of
 * "Acting from a policy".
 *
 * Inputs per sample b: logits[b][A] float32, the raw output of the policy head (no softmax; -inf masks an action), value[b] float32;
 * pi[b][A] float32 and z[b] float32 (what SelfPlay.sample() gives); weight[b] float32, the importance weights, may be NULL.  pi need not
 * sum to 1: a row of zeros and a scaled row are legal.  vf_coef >= 0 weighs the value error; delta: 0 gives the squared error, > 0
 * Huber's; scale: e.g. 1.0 / B for the gradient of the mean.  With l_a = logits[b][a]:
 *     m, x_a, e_a, S, T, L = LOG(S), p_a = e_a / S, lp_a = x_a - L          exactly as in "Soft values (discrete SAC)"
 *     H    = L - T / S                                                       (snac_policy_act's entropy, the same bytes)
 *     M    = sum_a (double)pi_a                  Lpi = -(sum_a (pi_a == 0 ? 0.0 : (double)pi_a * lp_a))
 *     dv   = (double)value - (double)z           ab = |dv|
 *     delta == 0:  Lv = dv * dv                                                       g = 2.0 * dv
 *     delta  > 0:  lin = ab > delta;  Lv = lin ? delta * (ab - 0.5 * delta) : 0.5 * (dv * dv);  g = lin ? (dv < 0 ? -delta : delta) : dv
 *     per  = Lpi + vf_coef * Lv                  w = weight ? (double)weight[b] : 1.0               total = w * per
 *     loss[b] = (float)per        priority[b] = (float)ab
 *     grad_logits[b][a] = l_a == -inf ? 0.0f : (float)(scale * (w * (M * p_a - (double)pi_a)))
 *     grad_value[b]     = (float)(scale * (w * (vf_coef * g)))
 *     agree = the first largest l_a and the first largest pi_a sit at the same index      (each: best = v_0, at = 0; for a = 1 .. A-1:
 *             if (v_a > best) { best = v_a; at = a; } -- float compares, ties go to the lowest index)
 *     u[0..8) = total, Lpi, Lv, H, ab, agree ? 1.0 : 0.0, 1.0, w
 *   d Lpi / d l_a = M p_a - pi_a, since d lp_i / d l_a = (i == a) - p_a; pi, z and the weight are constants of
 *   the loss.  lp_a is x_a - L and not LOG(p_a): it is finite for every finite logit, also more than 45 below the largest, where EXP
 *   gives e_a = 0 -- there p_a is 0 and the gradient is -scale w pi_a.  loss is the unweighted loss and priority the new priority of
 *   prioritised replay (snac_prio_update takes it as it is).
 *   Bad samples.  A sample is bad if some l_a is a NaN or +inf or every l_a is -inf; if some pi_a is not finite or is < 0 (-0.0 is a
 *   zero); if pi_a > 0 where l_a is -inf (a target on a masked action; with pi_a == 0 a masked action is fine); if value or z is not
 *   finite; or if weight is given and is not finite or negative.  A bad sample gets zeros in every per-sample output, contributes 0.0 to
 *   every u, and adds one to bad_rows[0] (int32 on the device, an atomic add).
 *   The statistics.  The two stages of "PPO loss", in its order, over the eight contributions u: partials[w][k] of the waves of 64
 *   consecutive samples, then the sums.  stats[k] = sum_k / (double)B for k != 6: the mean weighted loss, the mean cross-entropy, the mean
 *   value error, the mean entropy of the policy, the mean |value - z|, the fraction of samples whose largest logit is the search's
 *   choice, and (k = 7) the mean weight; stats[6] = sum_6, the number of good samples.  mean_loss[0] = (float)stats[0].
 * Outputs: loss, priority, grad_value float[B], grad_logits float[B][A], mean_loss float[1] and bad_rows may each be NULL and are then not
 * written.  stats double[SNAC_SEARCH_STATS] may be NULL: then nothing is reduced and the second launch does not happen (mean_loss must be
 * NULL too).  stats needs partials: ceil(B / 64) * SNAC_SEARCH_STATS doubles of caller-owned scratch, 8-byte aligned as stats is.  With
 * every output NULL nothing is launched.  The kernels read their inputs only and write nothing but the outputs given and partials.
 * Checks, all before any HIP call: logits, value, pi and z non-null; B >= 1; vf_coef and delta finite and >= 0; scale finite; partials
 * with stats, stats with mean_loss; the 8-byte alignments; num_actions 3, 5 or 8.  Both launches go on `stream`; no host
 * synchronisation. */
#define SNAC_SEARCH_STATS 8
int snac_search_loss(int32_t B, int32_t num_actions, const float* logits, const float* value, const float* pi, const float* z,
                     const float* weight, double vf_coef, double delta, double scale, float* loss, float* priority, float* grad_logits,
                     float* grad_value, double* stats, float* mean_loss, double* partials, int32_t* bad_rows, void* stream);

/* ---- Policy / value network on the device (snac_amd/mlp.py: DeviceMLP; k_mlp.hip, mlp_rule.h): the small MLP that guides the PUCT
 * search -- an observation row through one to four dense layers, ReLU between them, A + 1 outputs: the logits of the priors and the
 * value -- as ONE launch, with its softmax / value head and, in snac_mlp_uct_value_leaves, with the search's "value the leaves" step
 * behind it.  The gradients of its weights are the next section's ("Backward pass of the device network").  The weights are read in place, at every launch, from the
 * arrays the network descriptor points to (torch.nn.Linear's parameters as they lie in memory): an update enqueued on the stream before a
 * launch is seen by it, and nothing is copied or kept between launches.
 *
 * The network.  snac_mlp: 1 <= layers = L <= 4 dense layers of dimensions dim[0 .. L]; dim[0], the input width, 1 .. 512; the hidden
 * widths dim[1 .. L-1] 1 .. 256; dim[L] 1 .. 64.  Layer l has w[l] float32 [dim[l+1]][dim[l]] row-major and b[l] float32 [dim[l+1]],
 * each 4-byte aligned; entries past L are ignored.
 * The input.  x: rows of dim[0] values, contiguous, float32 (x_is_f64 = 0, 4-byte aligned) or float64 (x_is_f64 = 1, 8-byte aligned)
 * rounded to float32 first (what obs.to(torch.float32) does).  No wider alignment is assumed of any array.
 * Output j of a layer with K inputs x[0 .. K):
 *     acc = (double)b[j];   for i = 0, 1, .., K-1 in that order:  acc = acc + (double)W[j][i] * (double)x[i]
 *   The product of two float32 values is exact in float64, so a fused multiply-add and a multiply followed by an add give the same
 *   bits: the step rounds once, in the addition.  The sum of one output is never split or re-associated (how rows and outputs are
 *   mapped to lanes is free and cannot be seen in the result).
 *     a hidden output:          acc < 0.0 ? 0.0f : (float)acc         (ReLU; a NaN stays a NaN, -0.0 stays -0.0)
 *     an output of layer L-1:   (float)acc
 * The head (dim[L] == A + 1 with A = num_actions 3, 5 or 8; y the row of outputs): the logits are y[0 .. A) and
 *     m, x_a, e_a = EXP(x_a), S        exactly as in "Acting from a policy" (-inf masks an action: e_a = 0)
 *     priors[a] = (float)(e_a / S)     value = (double)y[A]
 *   A row is bad if some logit is a NaN or +inf, if every logit is -inf, or if y[A] is not finite: it gets priors of +0.0 in every place
 *   and value 0.0 and adds one to bad_rows[0] (int32 on the device, an atomic add).  logits, where asked for, receives the raw row
 *   y[0 .. A] of every row, bad or not.
 *
 * snac_mlp_forward        y[rows][dim[L]] float32: the outputs of the last layer.
 * snac_mlp_policy_value   priors float32 [rows][A], value float64 [rows], logits float32 [rows][A + 1], bad_rows: each may be NULL and is then
 *                         not written.
 * snac_mlp_uct_value_leaves   for the S = B * paths slots of a PUCT iteration (obs: their leaves' observation rows): the head, then
 *     term     = first_has[s] ? done[first_idx[s]] != 0 : stats[leaf[s]].terminal != 0     (first_idx clamped into [0, S), leaf into
 *                [0, stats_rows): the expander's done for a leaf made in this iteration, else the stored node's terminal word)
 *     value[s] = term ? 0.0 : value        est[s] = est[s] + value[s]        (one float64 addition)        priors[s][0 .. A) written whole
 *   first_has, done: uint8 [S]; first_idx, leaf: int32 [S]; stats: the rows of snac_uct_node as int32 words; priors, value, est and
 *   bad_rows may each be NULL.  This is what snac_amd/uct.py's UCTSearch runs between its selection and its backup when its evaluator is
 *   a DeviceMLP, in place of the evaluator's launches and the torch operations behind them.
 * Checks, all before any HIP call: net, its layers, every dim, its pointers and their alignment; x non-null and aligned as its type;
 * x_is_f64 0 or 1; rows >= 1; num_actions 3, 5 or 8 (else SNAC_ERR_UNSUPPORTED) and dim[L] == num_actions + 1; the alignment of every
 * output (float64: 8 bytes, else 4); the fused step's inputs non-null, stats_rows >= 1.  With every output NULL nothing is launched.
 * The kernel reads its inputs only and writes nothing but the outputs given; the launch goes on `stream`; no host synchronisation.
 * snac_last_kernel() names k_mlp_forward, k_mlp_policy_value or k_mlp_value_leaves. */
typedef struct snac_mlp {
    int32_t layers;
    int32_t dim[5];
    const float* w[4];
    const float* b[4];
} snac_mlp;
int snac_mlp_forward(const snac_mlp* net, const void* x, int x_is_f64, int32_t rows, float* y, void* stream);
int snac_mlp_policy_value(const snac_mlp* net, int32_t num_actions, const void* x, int x_is_f64, int32_t rows, float* priors, double* value,
                          float* logits, int32_t* bad_rows, void* stream);
int snac_mlp_uct_value_leaves(const snac_mlp* net, int32_t num_actions, const void* obs, int obs_is_f64, int32_t S, const uint8_t* first_has,
                              const int32_t* first_idx, const uint8_t* done, const int32_t* stats, int32_t stats_rows, const int32_t* leaf,
                              float* priors, double* value, double* est, int32_t* bad_rows, void* stream);

/* ---- Backward pass of the device network (snac_amd/mlp.py: DeviceMLP.backward, train_forward; k_mlp_grad.hip, mlp_grad_rule.h): from
 * the gradient of a scalar loss to the network's outputs to its gradient to every weight and bias, by float64 chains over exact products
 * in a stated order, as the forward rule's: the same inputs give the same bytes on every run.
 *
 * Notation.  The network is snac_mlp as above; layer l (0 .. L-1) maps h_l (width d_l = dim[l]) to h_{l+1} with W_l [d_{l+1}][d_l] and
 * b_l.  h_0 is the input row rounded to float32; h_1 .. h_L are the forward rule's own float32 activations, bit for bit -- the launch
 * sequence recomputes them and keeps nothing from an earlier forward call.  grad_y: float32 [rows][d_L], contiguous, 4-byte aligned: the
 * gradient to the outputs as the loss kernels write it, already divided by the batch size.
 * Per row b, from the top down:
 *     delta_L[k] = grad_y[b][k], as it is
 *     for l = L-1, L-2, .., 1 and every unit i of h_l:
 *         acc = 0.0;   for k = 0, 1, .., d_{l+1}-1 in that order:  acc = acc + (double)W_l[k][i] * (double)delta_{l+1}[k]
 *         delta_l[i] = h_l[i] <= 0.0f ? 0.0f : (float)acc
 *   The product of two float32 values is exact in float64, so a fused multiply-add and a multiply followed by an add give the same
 *   bits.  The chain of one unit is never split or re-associated.  The test h <= 0 is torch's threshold_backward: a unit cut to +0.0 or
 *   left at -0.0 passes nothing, a NaN activation passes acc.  delta_l is rounded to float32, so that the products below are exact too.
 *   delta_0, the gradient to the input, is not computed.
 * Over the batch, for every weight W_l[j][i] and bias b_l[j], with C = SNAC_MLP_GRAD_CHUNK: the rows are cut into chunks c = 0, 1, ..;
 * chunk c holds the rows [c C, min((c + 1) C, rows)).
 *     part_c = 0.0;   for b ascending in chunk c:  part_c = part_c + (double)delta_{l+1}[b][j] * (double)h_l[b][i]
 *                                         (a bias:  part_c = part_c + (double)delta_{l+1}[b][j])
 *     total = 0.0;    for c ascending:  total = total + part_c
 *     accumulate == 0:  g = (float)total          accumulate == 1:  g = (float)((double)g_old + total)
 *   The two-level association is part of the rule and shows in the bits.  How chunks, outputs and rows are mapped to blocks and lanes
 *   is free and cannot be seen in the result.  No float atomics.
 * Non-finite values.  Nothing is screened and there is no bad_rows: a non-finite grad_y or activation propagates as IEEE arithmetic says,
 * 0 * inf = NaN included.  (The loss kernels already zero the gradients of their bad samples.)
 * The result.  grad: one contiguous float32 array of P = sum over l of d_{l+1} (d_l + 1) values, 4-byte aligned: layer 0's weights
 * ([d_1][d_0] row-major), then layer 0's bias, then layer 1's weights, and so on.
 *
 * snac_mlp_backward_work_bytes   host only: the bytes of workspace a call needs,
 *     8 * chunks * P  +  4 * rows * 2 * (d_1 + .. + d_{L-1})        chunks = ceil(rows / C)
 *   the float64 partials of every parameter for every chunk, then the float32 hidden activations h_1 .. h_{L-1} and deltas
 *   delta_1 .. delta_{L-1} of every row (h_0 is read from x and delta_L from grad_y, where they lie).  A refused network (the limits of
 *   every dim, as above; its pointers are not looked at) or rows < 1: -1, with snac_last_error set.
 * snac_mlp_backward   work: the caller's buffer, 8-byte aligned, of work_bytes >= the size above; its contents before the call do not
 *   matter, and no byte past that size is written.  Checks, all before any HIP call: the network and x, x_is_f64 and rows as in the
 *   section above; grad_y and grad non-null and 4-byte aligned; accumulate 0 or 1; work non-null and 8-byte aligned; work_bytes large
 *   enough.  Three launches (two for L = 1) on `stream`, no host synchronisation; they read the inputs and the weights only and write
 *   only grad and work.  Each launch's error is looked at before the next.  snac_last_kernel() names
 *   the last kernel launched: k_mlp_grad_reduce, the last of the sequence, after a call that succeeded. */
#define SNAC_MLP_GRAD_CHUNK 256
int64_t snac_mlp_backward_work_bytes(const snac_mlp* net, int32_t rows);
int snac_mlp_backward(const snac_mlp* net, const void* x, int x_is_f64, int32_t rows, const float* grad_y, float* grad, int32_t accumulate,
                      void* work, int64_t work_bytes, void* stream);

/* ---- Optimiser step of the device network (snac_amd/optim.py: DeviceAdam; k_adam.hip, adam_rule.h): the global gradient norm, the
 * clip, Adam and the slow copy of a target network, read from the flat gradient of the section above and written into the parameters
 * where they lie, by a float64 rule in a stated order, as two launches with nothing waiting.  After it a whole update of the network is
 * device calls whose every output byte is stated here: forward, loss, backward, step.
 *
 * Notation.  The network is snac_mlp as above; P and the flat layout are snac_mlp_backward's: per layer the weights row-major, then the
 * bias.  theta[p] is the parameter at flat index p, read and written in the array w[l] / b[l] it belongs to: no flat copy of the
 * parameters exists.  g (the flat gradient, read only), m and v (Adam's moments, the caller's, read and written) are float32 [P],
 * 4-byte aligned.  Every float64 operation below is one operation of the rule, rounded on its own (no contraction).
 * Sum of squares, in the order of "PPO loss" with one column.  W = ceil(P / 64).  Lane j of wave w holds
 *     u = (double)g[p] * (double)g[p]   for p = 64 w + j < P,   else 0.0                  (the product of two float32 is exact)
 *   the xor butterfly u_j = u_j + u_{j ^ off}, off = 32, 16, .., 1 gives partials[w].  Stage two: lane j adds partials[j],
 *   partials[j + 64], .. in ascending order from 0.0, and the same butterfly gives ss.
 * Norm and clip.  norm = sqrt(ss).  max_norm == 0: coef = 1.0.  Otherwise c = max_norm / (norm + 1e-6) and coef = c < 1.0 ? c : 1.0
 *   (torch's clip_grad_norm_ and its constants).
 * A bad step: ss is not finite, that is, some g is a NaN or an infinity.  No byte of any parameter, of m, v or the target is written;
 *   bad_steps[0] gets an atomic add of 1; norm_out, where given, receives {norm, 0.0}.
 * Per parameter, with lr, beta1, beta2, eps, bias1 = 1 - beta1^t and bias2 = 1 - beta2^t given as doubles by the caller (nothing here
 * raises to a power):
 *     gd     = coef * (double)g[p]
 *     m'     = (float)(beta1 * (double)m[p] + (1.0 - beta1) * gd)
 *     v'     = (float)(beta2 * (double)v[p] + (1.0 - beta2) * (gd * gd))
 *     denom  = sqrt((double)v') / sqrt(bias2) + eps
 *     theta' = (float)((double)theta[p] - (lr / bias1) * ((double)m' / denom))
 *   The stored, rounded m' and v' are what the update reads, so a step continued from stored state is the same step.  Float32
 *   subnormals are kept, not flushed.  Nothing but ss is screened: eps = 0 with v' = 0 gives what IEEE says.
 * Target (optional): a second snac_mlp of the same dims, written in place.  tau == 1.0: tgt' = theta', the bits copied; otherwise
 *     tgt' = (float)((double)tgt + tau * ((double)theta' - (double)tgt))
 * How flat indices are mapped to blocks and lanes is free and cannot be seen in the result.  No float atomics.
 *
 * snac_mlp_adam_step   THIS AND snac_mlp_lerp ARE THE ONLY ENTRY POINTS THAT WRITE THE ARRAYS A snac_mlp POINTS TO (its fields are
 *   declared const float* for every reader; here the network's w[l] / b[l], and the target's, are outputs).  target may be NULL; tau is
 *   then ignored.  norm_out: double[2] = {norm, coef}, 8-byte aligned, may be NULL.  bad_steps: int32, may be NULL.  partials:
 *   ceil(P / 64) doubles of the caller's scratch, 8-byte aligned, never NULL; nothing past them is written.  Two launches on `stream`,
 *   k_adam_sumsq and k_adam_update: every block of the second redoes stage two from the partials -- the same order, so the same bits in
 *   every block -- so neither a grid synchronisation nor a third launch is needed.  Each launch's error is looked at before the next; no
 *   host synchronisation; snac_last_kernel() names k_adam_update.  The kernels read grad and write only the parameter arrays, m, v, the
 *   target's arrays, partials, norm_out and bad_steps.  Checks, all before any HIP call: the network as in snac_mlp_forward; grad, m, v
 *   and partials non-null and aligned (norm_out and bad_steps aligned where given); grad, m and v pairwise distinct; lr and eps finite
 *   and >= 0; beta1 and beta2 in [0, 1); bias1 and bias2 in (0, 1]; max_norm finite and >= 0; with a target: its layers and every dim
 *   equal to the network's, its pointers non-null, 4-byte aligned and none equal to a pointer of the network, and tau in (0, 1].
 * snac_mlp_lerp   the target's rule alone, with theta in place of theta': DQN's hard copy every K ticks (tau = 1) and SAC's lerp per
 *   step.  One launch (k_mlp_lerp); the network's checks and the target's checks above. */
int snac_mlp_adam_step(const snac_mlp* net, const float* grad, float* m, float* v, double lr, double beta1, double beta2, double eps,
                       double bias1, double bias2, double max_norm, const snac_mlp* target, double tau, double* norm_out, double* partials,
                       int32_t* bad_steps, void* stream);
int snac_mlp_lerp(const snac_mlp* target, const snac_mlp* net, double tau, void* stream);

/* ---- Acting with the device network over a rollout (snac_amd/batched.py: rollout_policy; k_policy_roll.hip): T ticks of
 * observe -> network -> draw -> step in ONE launch, the env state on chip from the first tick to the last.  The join of snac_rollout_rec
 * (whose actions are the counter RNG's or the caller's) and snac_mlp_forward / snac_policy_act (one launch each per tick): a model-free
 * actor's loop, or the greedy evaluation episodes of a trained network, without a launch between two ticks.  Nothing here is a new rule:
 * every step is another section's, in this order.  N = desc->num_envs; env i, tick tau = t0 + j (uint32: it wraps), j = 0 .. T-1:
 *   1. Reset.  If the env's header has SNAC_FLAG_NEED_RESET it starts a new episode exactly as snac_step(auto_reset = 1) does (the plan
 *      row from counter-RNG stream 1 keyed by the episode, the episode counter, the grid emptied).
 *   2. Input.  The canonical observation row that snac_observe would write now (obs_dim values of desc->obs_dtype), each rounded to
 *      float32 as in "Policy / value network on the device".  If net->dim[0] == obs_dim + P (P = 30 for 1D, 400 for 2D / 3D) the row is
 *      followed by the P cells of the env's plan, row-major (SNAC_TAIL_PLAN's values): what
 *      torch.cat([obs.float(), env.input_plan().float().flatten(1)], 1) holds.  dim[0] must be obs_dim or obs_dim + P.
 *   3. Network.  y = the outputs of layer L-1 by the rule of "Policy / value network on the device", unchanged.  dim[L] must be A or
 *      A + 1, A the kind's num_actions.
 *   4. Draw.  The rule of snac_policy_act, unchanged, on the scores y[0 .. A) with w = word(desc->seed, 5, desc->env_id_base + i, tau):
 *      the same three modes, epsilon rules and bad-row rule (drawn as if every score were 0, one more in bad_rows[0]).
 *      logp[j][i], entropy[j][i]: the categorical mode's, NULL in the other modes.  value[j][i] = y[A], the float32 as it is, finite or
 *      not (it does not make a row bad here); NULL when dim[L] == A.
 *   5. Step.  snac_step's tick tau with that action and the step size of counter-RNG stream 0 (step_size NULL).  The outputs are
 *      snac_rollout_rec's: obs ([T][N][obs_dim] for SNAC_OBS_ALL, [N][obs_dim] for SNAC_OBS_LAST, untouched for SNAC_OBS_NONE;
 *      SNAC_OBS_TILED: SNAC_ERR_UNSUPPORTED), reward float [T][N], done uint8 [T][N], and rec's actions, step_size, plan_idx and first
 *      (1 on the first step of an episode), each [T][N].  Every output may be NULL, rec too.
 * Afterwards the state arrays of st (headers, grids, episode counters, episodic sums) are what T calls of snac_step(auto_reset = 1)
 * with those actions would have left.  Envs do not interact: a batch split into shards by env_id_base gives the same bytes.
 * All three kinds, static and dynamic, desc->rules, both observation dtypes; the canonical layout only (a frame_value, obs_scalars or
 * obs_tail that changes the row: SNAC_ERR_UNSUPPORTED).  Any N >= 1; nothing of the caller's is assumed wider-aligned than its element
 * type, except the state arrays ("Alignment of the state arrays").  The weights are read in place during the launch.
 * Checks, all before any HIP call: those of snac_rollout_rec on desc and st; net, its layers, dims, pointers and their alignment; T >= 1;
 * mode, epsilon, epsilon_per_env, logp and entropy as snac_policy_act; obs_mode and obs; the canonical layout; dim[0] and dim[L] as
 * above; value NULL when dim[L] == A; every array aligned as its element type.  One launch on `stream`, no host synchronisation.
 * snac_last_kernel() names k_policy_rollout. */
int snac_policy_rollout(const snac_env_desc* desc, const snac_state* st, const snac_mlp* net, int32_t T, uint32_t t0, int32_t mode,
                        double epsilon, const float* epsilon_per_env, int obs_mode, void* obs, float* reward, uint8_t* done,
                        const snac_rollout_record* rec, float* value, float* logp, float* entropy, int32_t* bad_rows, void* stream);

/* ---- plan generators: the hindsight classes of the reference draw a fresh random plan per reset --
 * random triangles in 2D / 3D (create_plan, Env/2D/DMP_Env_2D_dynamic_hindsight_replay_usedata.py:37-59: three vertices from
 * np.random.randint(0, 20, size=3) twice, cv2.polylines (+ cv2.fillPoly when dense), redrawn until more than 50 (dense) / 20
 * (sparse) cells are set; the datasets of 400 / 50 / 50 plans were made this way) and random sine curves in 1D (create_plan,
 * Env/1D/DMP_Env_1D_dynamic_hindsight_replay.py:29-42: k1 = uniform(3, 12), k2 = randint(1, 4), phase = uniform(-1, 1) pi,
 * y = round(k1 sin(2 pi / 30 (k2 x + phase)) + 20)).  snac_make_plans writes rows [first, first + count) of st->plans and
 * st->plan_tb (the caller's tables, in the layout of desc->kind) on the device, one wavefront per plan:
 *   vertices NULL   counter RNG stream 2 keyed by (seed, plan_id_base + row): attempt a uses words 4a, 4a+1, 4a+2 (vertex v:
 *                   x = ((word & 0xffff) * 20) >> 16, y = ((word >> 16) * 20) >> 16), redrawn (at most 64 times) until the
 *                   area threshold is passed; 1D: words 0, 1, 2 -> k1 = 3 + 9 u, k2 = 1 + (word * 3 >> 32), phase = (2 u - 1) pi
 *                   with u = word * 2^-32, y = rint(fma(k1, sin(..), 20)) with the sine specified in snac_hip.hip (spec_sin)
 *   vertices        int8[count][6] = x0 y0 x1 y1 x2 y2 (2D / 3D): ONE rasterisation per row, no redraw -- the caller draws the
 *                   vertices (the drop-in classes take them from np.random like the reference) and loops on area_out
 *   sparse          0: outline + interior, threshold 50; 1: outline only, threshold 20; 3D plans also need fewer than 110 cells
 *                   (script/HumanPlayerGUI/env/Env3D.py:360-364, how the 3D datasets were drawn)
 *   area_out        int32[count] or NULL: number of cells set (1D: total_brick); NEGATIVE (-cells) for a row whose 64 redraws were
 *                   all rejected (probability ~ 0): the last triangle stands, with total_brick >= 1
 * Rasteriser: cv2's own rules for this call restated (LineIterator with leftToRight for the outline, the 16.16 fixed-point
 * scanline fill of FillEdgeCollection for dense plans; snac_hip.hip tri_row).  cv2 itself is not available where this was
 * built, but its OUTPUT is: all 1000 2D dataset plans the reference ships, drawn by its authors with this code, are
 * reproduced bit for bit from their vertices (tests/test_plan_generators.py, tests/golden/dataset_triangles.npz).  What stays
 * unpinned is the np.random stream a seeded script sees (the counter RNG draws the vertices here; the drop-in class passes
 * np.random's vertices in).  2D total_brick = max(area, 30); 3D plan = mask * 6, total_brick = 6 area. */
int snac_make_plans(const snac_env_desc* desc, const snac_state* st, int32_t first, int32_t count, int32_t sparse,
                    uint64_t seed, int64_t plan_id_base, const int8_t* vertices, int32_t* area_out, void* stream);

/* ---- hindsight relabelling on the device: the DRQN_hindsight scripts replay a finished episode on a
 * second env whose plan has been overwritten with the episode's own final grid
 * (script/DRQN_hindsight/2d/DRQN_hindsight_2D_dynamic.py:270-282: env_hindsight.plan[3:23, 3:23] =
 *  env_train.environment_memory[3:23, 3:23]; 1D: script/DRQN_hindsight/1d/DRQN_hindsight_1D_static.py:243).  That overwrite as one
 * launch: for i in [0, m)
 *     plan row first + i of st  <-  max(interior of grid i, 0)          (2D: the 0 / 1 board; 1D / 3D: the heights)
 *     st->plan_tb[first + i]    <-  total_brick[i], or (NULL) the total_brick in the header of source env i
 * The grids come EITHER from the packed records of a batch -- src (its grid and hdr; src_envs rows; src_rows int32[m] picks the
 * envs, NULL: env i) -- OR from environment_memory double[m][env_height][env_width] in the reference's own format (frame values
 * are ignored; total_brick is then required).  st and src may be the same batch.  The relabel rollout is then snac_rollout on a
 * batch whose env i was reset onto row first + i with the recorded actions and step sizes (snac_amd/hindsight.py). */
int snac_plans_from_grids(const snac_env_desc* desc, const snac_state* st, int32_t m, int32_t first, const snac_state* src,
                          int32_t src_envs, const int32_t* src_rows, const double* environment_memory,
                          const int32_t* total_brick, void* stream);

/* current observation of every env without stepping: observation_() + the hstack of
 * Env/2D/DMP_Env_2D_dynamic_usedata_plan.py:64-72 */
int snac_observe(const snac_env_desc* desc, const snac_state* st, void* obs, void* stream);

/* iou(): Env/1D/DMP_Env_1D_static.py:138-151, Env/3D/DMP_simulator_3d_static_circle.py:257-276, and the
 * caller-side boolean IoU of the 2D scripts (script/DQN/2d/DQN_2d_dynamic.py:63-71).  out: double[N] */
int snac_iou(const snac_env_desc* desc, const snac_state* st, double* out, void* stream);

/* the batch's three episodic sums in ONE launch: out3[0 .. 2] = the sums over all N envs of st->stat_episodes, stat_return and
 * stat_iou_fx (int64, modulo 2^64: exactly what adding the arrays up in any order gives).  out3: int64[3] on the device, written by
 * the launch (nothing is read from it).  scratch: int64[SNAC_SUMS_SCRATCH_WORDS] on the device, OWNED BY THE CALLER: zeroed once when
 * it is created and never touched by anyone else; every call leaves it zeroed where it has to be (the launch's last block takes the
 * partial sums out and sets its ticket back to 0), so no call is preceded by a fill.  Calls that may run at the same time -- two
 * batches on two streams -- need a scratch each; calls on one stream may share one.  The per-env arrays stay the only record of the
 * sums: nothing is kept between calls.  Pointers 8-byte aligned.  Arguments are checked before any HIP call; the call does not
 * change what snac_last_kernel() names. */
#define SNAC_SUMS_SCRATCH_WORDS (3 * 64 + 1)
int snac_episodic_sums(const snac_env_desc* desc, const snac_state* st, int64_t* out3, int64_t* scratch, void* stream);

/* environment_memory as the reference holds it: out is double[N][env_height][env_width] with the -1 frame */
int snac_export_grid(const snac_env_desc* desc, const snac_state* st, double* out, void* stream);

/* ---- the resident single-env stepper (round 5): what the drop-in classes step through.
 * The reference's scripts drive ONE env, one env.step(action) per loop turn (script/DQN/2d/DQN_2d_dynamic.py:214;
 * Env/2D/DMP_Env_2D_dynamic_usedata_plan.py:85-147 is 9 us of Python per step).  Through snac_step_scalar such a step is one launch and
 * one stream wait (15 us).  A mailbox keeps ONE wavefront resident instead: it polls a doorbell in coherent page-locked host memory,
 * steps the envs of a small batch (N = 1: the drop-in classes; up to 256: an env per lane, 64 envs per wavefront, a launch per wavefront) with the kind's own step rules, writes the observation row (obs_dim values of obs_dtype, layout of desc,
 * tails included) into the mailbox over the bus, acknowledges, and writes the env's state through to st behind the acknowledgement
 * (snac_mailbox_settle waits for that: call it before any other entry point reads or changes st).  The wave leaves by itself after idle_us microseconds without a command
 * (0 = 1000) and on snac_mailbox_quit / _destroy; snac_mailbox_step arms (launches) one when none is resident.
 *   snac_mailbox_touch   the caller has changed st through another entry point (reset, plan row, import ...) and has waited for it:
 *                        the wave reloads the records before its next step
 *   snac_mailbox_step    semantics of snac_step_scalar(desc, st, t, action, step_size, auto_reset = 0, row, NULL, NULL) + a wait;
 *                        episodic sums are updated like snac_step's.  A wave whose launch is still QUEUED (behind kernels that fill the
 *                        device) is waited for, up to SNAC_MAILBOX_TIMEOUT_S seconds (default 120); then the command is WITHDRAWN
 *                        (replaced by a quit of the same sequence number: a wave that starts later leaves without stepping) and the
 *                        call returns SNAC_ERR_HIP with st as the last acknowledged step left it -- or SNAC_OK if the step was served
 *                        while it was being withdrawn.  (A batch of several waves whose launch the limit cut in two: the error string
 *                        names the waves, as a bit mask, whose 64 envs each HAVE taken the step; the others have not.)
 *                        The mailbox belongs to the device that was current at snac_mailbox_create:
 *                        its waves are launched there whatever is current later.  While a thread keeps stepping, a wave stays
 *                        resident: a device-wide synchronisation (hipDeviceSynchronize, hipFree) in ANOTHER thread returns only once the
 *                        stepping pauses for idle_us -- synchronise streams or events there instead
 *   snac_mailbox_row     the row (host pointer, valid until destroy; also a device pointer: the launch path may write it too)
 *   snac_mailbox_stats   out[0] launches, out[1] steps served, out[2] a wave is resident, out[3] idle_us, out[4..7] the last step in ticks of
 *                        the GPU's 100 MHz clock: transition, row stores issued, fence before the acknowledgement, write-through behind it */
typedef struct snac_mailbox snac_mailbox;
int snac_mailbox_create(const snac_env_desc* desc, uint32_t idle_us, snac_mailbox** out);
double* snac_mailbox_row(snac_mailbox* mb);
int snac_mailbox_touch(snac_mailbox* mb);
int snac_mailbox_step(snac_mailbox* mb, const snac_env_desc* desc, const snac_state* st, int32_t action, int32_t step_size);
/* the same for a batch of up to 256 envs (wavefront w takes envs [64 w, 64 w + 64), env 64 w + e on lane e; every wavefront is a launch
 * of its own on a stream of its own and polls the same doorbell) -- the reference's VectorizedEnvWrapper
 * (multiprocess.py:15-32, default --num_envs 3): actions / step_size int8[num_envs] in host memory; rows [num_envs][obs_dim] in
 * snac_mailbox_row, rewards float[num_envs] in snac_mailbox_reward, done flags uint8[num_envs] in snac_mailbox_done */
int snac_mailbox_step_n(snac_mailbox* mb, const snac_env_desc* desc, const snac_state* st, const int8_t* actions, const int8_t* step_size);
float* snac_mailbox_reward(snac_mailbox* mb);
uint8_t* snac_mailbox_done(snac_mailbox* mb);
int snac_mailbox_settle(snac_mailbox* mb);   /* wait until st holds the last acknowledged step (the write-through trails the acknowledgement) */
int snac_mailbox_quit(snac_mailbox* mb);
int snac_mailbox_destroy(snac_mailbox* mb);
int snac_mailbox_stats(const snac_mailbox* mb, uint32_t out[8]);

/* ---- tree search: the MCTS variants of the reference (Env/1D/DMP_Env_1D_{static,dynamic}_MCTS*.py,
 * Env/2D/DMP_ENV_2D_{static,dynamic}_MCTS*.py, Env/3D/DMP_simulator_3d_*_MCTS*.py; nine files) ----
 *
 * transition(state, action, is_model_dynamic) -> (state', obs, reward, done)
 * (Env/2D/DMP_ENV_2D_dynamic_MCTS.py:117-175, Env/1D/DMP_Env_1D_dynamic_MCTS.py:82-139,
 *  Env/3D/DMP_simulator_3d_static_circle_MCTS.py:215-288, Env/3D/DMP_simulator_3d_dynamic_triangle_MCTS.py:195-277;
 *  called once per tree edge by script/MCTS/utils/mcts_Qvalue_dynamic.py:88,118), batched over m edges.
 * The state arrays of `st` are used as a NODE POOL of desc->num_envs rows.  For i in [0, m):
 *     row dst_index[i]  <-  step(row src_index[i], actions[i], step size i)        (index NULL: row i)
 * with the step rules of (kind, dynamic), no auto-reset, and no change to the episodic sums: the running return, episode
 * counter, plan row and total_brick travel with the state; SNAC_FLAG_NEED_RESET records `done`.
 *   actions / step_size   int8[m] or NULL = counter RNG stream 0 keyed by (env_id_base + i, t)
 *   obs                   [m][obs_dim] (obs_dtype) or NULL;  reward float[m] / done uint8[m] or NULL
 * Indices are clamped into the pool.  A destination row must not be the source row of a DIFFERENT edge of the same call
 * (dst_index[i] == src_index[i], i.e. in place, is fine); several edges may share a source. */
int snac_transition(const snac_env_desc* desc, const snac_state* st, int32_t m, const int32_t* src_index,
                    const int32_t* dst_index, uint32_t t, const int8_t* actions, const int8_t* step_size, void* obs,
                    float* reward, uint8_t* done, void* stream);

/* ---- 2D node pools with ONE record per node (round 6).  A tree edge reads its parent at a random row; in the arrays of snac_state
 * that is three lines of memory (header, episode counter, board: the memory side reads whole 128-byte lines) for 100 bytes.  A
 * snac_node2d holds the three in one line: an edge reads one line and writes one.  The pool is caller-owned, 128-byte aligned.
 *   snac_nodes2d_pack        node record node_rows[i] (NULL: i)  <-  batch row rows[i] (NULL: i) of st, i in [0, m)
 *   snac_nodes2d_unpack      the inverse: batch row rows[i] of st  <-  node record node_rows[i]
 *   snac_transition_nodes2d  snac_transition on the pool: record dst_index[i] <- step(record src_index[i], actions[i], step size i);
 *                            st supplies the plan table (plans, plan_tb) only; same rules, outputs and index conventions; the
 *                            canonical observation layout (variants: snac_transition); 2D kinds only */
typedef struct snac_node2d {    /* 128 bytes, 128-byte aligned */
    snac_env_hdr hdr;
    int32_t episode;
    int32_t zero0[3];
    uint32_t board[20];         /* the grid record of the 2D kinds: row word q, bit j = interior cell (q, j) */
    uint32_t zero1[4];
} snac_node2d;
int snac_nodes2d_pack(const snac_env_desc* desc, const snac_state* st, const int32_t* rows, int32_t m, snac_node2d* nodes, int32_t pool_rows,
                      const int32_t* node_rows, void* stream);
int snac_nodes2d_unpack(const snac_env_desc* desc, const snac_node2d* nodes, int32_t pool_rows, const int32_t* node_rows, int32_t m, snac_state* st,
                        const int32_t* rows, void* stream);
int snac_transition_nodes2d(const snac_env_desc* desc, const snac_state* st, snac_node2d* nodes, int32_t pool_rows, int32_t m,
                            const int32_t* src_index, const int32_t* dst_index, uint32_t t, const int8_t* actions, const int8_t* step_size,
                            void* obs, float* reward, uint8_t* done, void* stream);

/* ---- 1D and 3D node pools with ONE record per node: the same idea and the same index, clamping and error conventions as the 2D
 * pools above, for transition(state, action) of Env/1D/DMP_Env_1D_dynamic_MCTS.py:82-139 (static: DMP_Env_1D_static_MCTS.py) and
 * Env/3D/DMP_simulator_3d_static_circle_MCTS.py:215-288, DMP_simulator_3d_dynamic_triangle_MCTS.py:195-277.  In the arrays of
 * snac_state a 1D parent is three lines for 84 bytes (header, episode counter, 64-byte grid record) and a 3D parent nine lines (the
 * 800 bytes of heights at offset r * 800 span seven, plus the header's and the counter's); a snac_node1d is one line, a snac_node3d
 * seven whole lines.  Every pad word is zero after a pack and stays zero after a transition.  Each entry point accepts its own kind
 * only and the canonical observation layout (layout variants: SNAC_ERR_UNSUPPORTED); no auto-reset, no episodic sums. */
typedef struct snac_node1d {    /* 128 bytes, 128-byte aligned: ONE line */
    snac_env_hdr hdr;
    int32_t episode;
    int32_t zero0[3];
    int16_t cells[32];          /* the grid record of the 1D kinds: 30 interior heights + 2 pad (zero) */
    uint32_t zero1[8];
} snac_node1d;
typedef struct snac_node3d {    /* 896 bytes, 128-byte aligned: seven lines */
    snac_env_hdr hdr;
    int32_t episode;
    int32_t zero0[3];
    int16_t heights[400];       /* the grid record of the 3D kinds: the 20x20 interior, row-major */
    uint32_t zero1[16];
} snac_node3d;
int snac_nodes1d_pack(const snac_env_desc* desc, const snac_state* st, const int32_t* rows, int32_t m, snac_node1d* nodes, int32_t pool_rows,
                      const int32_t* node_rows, void* stream);
int snac_nodes1d_unpack(const snac_env_desc* desc, const snac_node1d* nodes, int32_t pool_rows, const int32_t* node_rows, int32_t m, snac_state* st,
                        const int32_t* rows, void* stream);
int snac_transition_nodes1d(const snac_env_desc* desc, const snac_state* st, snac_node1d* nodes, int32_t pool_rows, int32_t m,
                            const int32_t* src_index, const int32_t* dst_index, uint32_t t, const int8_t* actions, const int8_t* step_size,
                            void* obs, float* reward, uint8_t* done, void* stream);
int snac_nodes3d_pack(const snac_env_desc* desc, const snac_state* st, const int32_t* rows, int32_t m, snac_node3d* nodes, int32_t pool_rows,
                      const int32_t* node_rows, void* stream);
int snac_nodes3d_unpack(const snac_env_desc* desc, const snac_node3d* nodes, int32_t pool_rows, const int32_t* node_rows, int32_t m, snac_state* st,
                        const int32_t* rows, void* stream);
int snac_transition_nodes3d(const snac_env_desc* desc, const snac_state* st, snac_node3d* nodes, int32_t pool_rows, int32_t m,
                            const int32_t* src_index, const int32_t* dst_index, uint32_t t, const int8_t* actions, const int8_t* step_size,
                            void* obs, float* reward, uint8_t* done, void* stream);

/* (position, environment_memory, count_brick, count_step) tuples of the reference (the `state` of the MCTS variants,
 * Env/2D/DMP_ENV_2D_dynamic_MCTS.py:88-91) -> pool rows dst_index[i] (NULL: row i); the inverse of snac_export_grid plus
 * the header.  position int32[m][2] (row, col; 1D: position, ignored), count_brick / count_step int32[m],
 * plan_idx int32[m] or NULL (the row keeps its plan), total_brick int32[m] or NULL (plan_tb of the plan row),
 * environment_memory double[m][env_height][env_width].  The running return restarts at 0; values are clamped into the
 * ranges the kernels index with. */
int snac_import_state(const snac_env_desc* desc, const snac_state* st, int32_t m, const int32_t* dst_index,
                      const int32_t* position, const int32_t* count_brick, const int32_t* count_step,
                      const int32_t* plan_idx, const int32_t* total_brick, const double* environment_memory, void* stream);

/* equality_operator(o1, o2) (np.array_equal of two observations, Env/2D/DMP_ENV_2D_dynamic_MCTS.py:254-258; how
 * script/MCTS/utils/mcts_Qvalue_dynamic.py:100-106 recognises an already-expanded child), for m pairs:
 *     out[i] = all(obs_a[idx_a[i]] == obs_b[idx_b[i]])        (index NULL: row i; rows of obs_dim values, obs_dtype)
 * rows_a / rows_b: number of rows of the two arrays (indices are clamped). */
int snac_obs_equal(const snac_env_desc* desc, const void* obs_a, const int32_t* idx_a, int32_t rows_a, const void* obs_b,
                   const int32_t* idx_b, int32_t rows_b, int32_t m, uint8_t* out, void* stream);

/* The "Evaluation" block of the vanilla MCTS procedure (script/MCTS/utils/mcts.py:100-110): from a leaf, default-policy steps until
 * `terminal` or the horizon, `estimate += reward * gamma**t` in that order.  The steps are a snac_rollout of the forked leaves without
 * observation rows (reward / done [H][m]); this call does the sums on the device, one leaf per lane, sequentially in t, each product
 * and each sum rounded to float64 (no fused multiply-add) -- what the reference's python floats do:
 *     alive = !terminal[i];  for t in 0 .. H - 1 while alive:  est[i] += (double)reward[t][i] * gpow[t];  steps[i] += 1;  alive = !done[t][i]
 * est [m]: in = the leaf's first reward (the reference's `estimate = reward`), out = the estimate; steps [m] out (may be NULL);
 * terminal [m] may be NULL (no leaf is terminal); gpow [H] = gamma**t as the CALLER's pow computes it (device memory, like the rest). */
int snac_discounted_return(int32_t H, int32_t m, const float* reward, const uint8_t* done, const uint8_t* terminal, const double* gpow,
                           double* est, int64_t* steps, void* stream);

/* The same evaluation IN PLACE on a node pool (snac_node1d / 2d / 3d above), one fused launch: no fork, no reward / done arrays.  For every
 * leaf i in [0, m), from record node_rows[i] (NULL: i; clamped into the pool as in snac_transition_nodes*), what snac_discounted_return
 * computes over a rollout of the forked leaf (script/MCTS/utils/mcts.py:100-110):
 *     alive = !(record.hdr.flags & SNAC_FLAG_NEED_RESET)
 *     for t in 0 .. H - 1 while alive:  (action, k) = counter RNG stream 0 keyed by (env_id_base + i, t0 + t);  step the leaf with the
 *                                       rules of (kind, dynamic, desc->rules);  est[i] += (double)reward * gpow[t];  steps[i] += 1;  alive = !done
 * product and sum each rounded to float64 (no fused multiply-add).  est [m] in / out as in snac_discounted_return (in: the first reward);
 * steps [m] out, may be NULL; gpow [H] device memory.  st supplies the plan table (plans, plan_tb) only.  The pool is READ ONLY: no
 * record, batch row or episodic sum changes, and there is no auto-reset.  H == 0: est stays, steps are written as zero; m == 0: nothing.
 * With t0 = 0 the actions are those BatchedDMPEnv.evaluate (fork + snac_rollout + snac_discounted_return) draws for the same leaves.
 * Each entry point accepts its own kind and the canonical layout only (SNAC_ERR_UNSUPPORTED), with the argument checks of the other
 * node entry points, before any HIP call. */
int snac_evaluate_nodes1d(const snac_env_desc* desc, const snac_state* st, const snac_node1d* nodes, int32_t pool_rows, int32_t m,
                          const int32_t* node_rows, int32_t H, uint32_t t0, const double* gpow, double* est, int64_t* steps, void* stream);
int snac_evaluate_nodes2d(const snac_env_desc* desc, const snac_state* st, const snac_node2d* nodes, int32_t pool_rows, int32_t m,
                          const int32_t* node_rows, int32_t H, uint32_t t0, const double* gpow, double* est, int64_t* steps, void* stream);
int snac_evaluate_nodes3d(const snac_env_desc* desc, const snac_state* st, const snac_node3d* nodes, int32_t pool_rows, int32_t m,
                          const int32_t* node_rows, int32_t H, uint32_t t0, const double* gpow, double* est, int64_t* steps, void* stream);

/* The observation rows of node records (what a policy / value network reads of a search's leaves; k_nodes_obs.hip): for i in [0, m),
 * obs[i] = the canonical row (obs_dim values of desc->obs_dtype) of record node_rows[i] (NULL: record i; clamped into the pool as in
 * snac_transition_nodes*) -- byte for byte what snac_observe writes for a batch row into which that record was unpacked, for every record,
 * one with SNAC_FLAG_NEED_RESET included (no reset, no step: the record's own position, grid and counters).  st supplies the plan table
 * only; the pool is READ ONLY; several i may name one record.  Each entry point accepts its own kind and the canonical layout only
 * (SNAC_ERR_UNSUPPORTED), with the argument checks of the other node entry points and obs non-null, before any HIP call; m == 0: nothing. */
int snac_observe_nodes1d(const snac_env_desc* desc, const snac_state* st, const snac_node1d* nodes, int32_t pool_rows, int32_t m,
                         const int32_t* node_rows, void* obs, void* stream);
int snac_observe_nodes2d(const snac_env_desc* desc, const snac_state* st, const snac_node2d* nodes, int32_t pool_rows, int32_t m,
                         const int32_t* node_rows, void* obs, void* stream);
int snac_observe_nodes3d(const snac_env_desc* desc, const snac_state* st, const snac_node3d* nodes, int32_t pool_rows, int32_t m,
                         const int32_t* node_rows, void* obs, void* stream);

/* ---- UCT tree search over node pools: selection, backup and re-rooting (k_uct.hip).  B independent trees, one path per tree per iteration;
 * tree b owns node rows [b * cap, (b + 1) * cap) of a node pool and of the statistics array below (its root: row b * cap; its j-th
 * allocated node: row b * cap + j), and rows B * cap + b are per-tree scratch rows that never become nodes.  An iteration is
 *     snac_uct_select -> snac_transition_nodes{1,2,3}d (B edges src[b] -> dst[b], action[b], step_size NULL)
 *                     -> est[b] = expanded[b] ? reward[b] : r_leaf[b] -> snac_evaluate_nodes{1,2,3}d (node_rows = leaf) -> snac_uct_backup
 * all on one stream, with no host synchronisation (snac_amd/uct.py: UCTSearch).
 * Selection, per tree, from the root, at most cap steps; at node n:
 *   terminal: stop, leaf = n;  else an untried action (child[a] == -1) and fewer than cap nodes used (used[b]): expand the lowest such a
 *   into row b * cap + used[b] (child[a] set, used[b] += 1), leaf = that row;  else children: descend to the one with the largest
 *       U = child_value[a] / child_visits[a] + c * (log_table[visits(n)] * rsqrt_table[child_visits[a]])
 *   in float64, no contraction, in that order (ties: the lowest a; table indices clamped to [0, table_len - 1]);  else stop, leaf = n.
 *   Expanded: src = n, dst = the new row, action = a.  Not expanded: src = leaf, dst = B * cap + b, action = 0 (the result is unused),
 *   r_leaf = the leaf's stored reward.  log_table[i] = sqrt(log(i)), rsqrt_table[i] = 1 / sqrt(i), computed by the caller.
 * Backup, per tree: an expanded leaf's row is written whole (parent = src, action, reward and terminal = the transition's reward /
 *   done, no children, no visits); then G = est[b] and, from the leaf up to the root, visits += 1, value_sum += G (mirrored into the
 *   parent's child_visits / child_value), G = reward(parent) + gamma * G, each operation rounded to float64 (no contraction).
 * Child row indices are clamped into their tree's rows.  Both entry points check every argument before any HIP call: num_actions
 * 3, 5 or 8; no null pointer; B >= 1; cap >= 1; B * (cap + 1) within stats_rows and int32; table_len >= 2; stats 128-byte aligned.
 * Re-rooting after a move (snac_uct_advance): tree b plays actions[b] (clamped into [0, num_actions)); base = b * cap, R = its root.
 *   Terminal root (R.terminal != 0): the tree is unchanged (statistics, records, used[b]); reward_out[b] = 0, done_out[b] = 1.
 *   Tried action (c = R.child[actions[b]] >= 0): the new tree is the subtree of c -- c and every node whose parent chain reaches c,
 *     renumbered in increasing old row order (c -> base), used[b] = their number.  A child's row is always above its parent's, so the
 *     compacted tree again has its root at base, its nodes in [base, base + used[b]) and parent < child: selection and backup run on
 *     it unchanged.  child[] and parent are remapped to the new rows; every other field moves bit for bit (child_visits, child_value,
 *     action, terminal, visits, value_sum, reward, zero), except that the new root gets parent = -1, action = -1, reward = 0 (its
 *     terminal, visits and value_sum stay).  Each kept node's record (record_bytes: 128 for 1D / 2D, 896 for 3D) moves with its
 *     statistics row, byte for byte.  reward_out[b] / done_out[b] = c's stored reward / terminal.
 *   Untried action (child == -1): the new tree is one node, the transition of R by actions[b]: the caller has run that edge just before
 *     into the tree's scratch record (B * cap + b), with its reward / done in edge_reward[b] / edge_done[b]; that record goes to base,
 *     the root's statistics start fresh (children -1, no visits, W = 0, terminal = edge_done[b]), used[b] = 1; the outputs are the
 *     edge's reward and done.
 *   Rows [base + used[b], base + cap) and the scratch rows hold unspecified contents afterwards (statistics and records); nothing reads
 *   them before they are written whole.  work: caller scratch of 2 * B * cap int32 (an old -> new and a new -> old map per tree).  No
 *   host synchronisation.  Checks before any HIP call, beside those above: records non-null and 128-byte aligned; record_bytes 128 or
 *   896; B * (cap + 1) within record_rows; no null per-tree array; work non-null.
 * K paths per tree and iteration (snac_uct_select_paths / snac_uct_backup_paths; paths = K >= 1, tree parallelism with virtual loss).
 *   Slot s = b * K + k is path k of tree b.  Every per-slot array (src, dst, action, leaf, expanded, r_leaf, reward, done, est,
 *   first_slot) has B * K entries; used keeps B.  The scratch row of slot s is row B * cap + s, so the node pool and the statistics
 *   array need B * (cap + K) rows (snac_uct_advance keeps using scratch row B * cap + b, which lies inside that range; nothing reads a
 *   scratch row across calls).  Counter words: the transition and evaluation launches of an iteration key slot s by the descriptor's
 *   env_id_base + s.  The caller passes them a copy of the env's descriptor with env_id_base * K, so that path k of tree b draws with
 *   (env_id_base + b) * K + k -- the slot of global tree env_id_base + b in one search over all envs -- and a shard of the trees searches
 *   exactly as the whole does; env_id_base * K and (env_id_base + B) * K - 1 must fit int64.  Everything per tree (snac_uct_advance's
 *   edge, snac_uct_pick_moves, the env's reset) keeps the env's own env_id_base.  An iteration is
 *     snac_uct_select_paths -> snac_transition_nodes* (B * K edges) -> est[s] = first_slot[s] >= 0 ? reward[first_slot[s]] : r_leaf[s]
 *                           -> snac_evaluate_nodes* (B * K leaves, several slots may name one row) -> snac_uct_backup_paths.
 *   Selection, per tree, paths k = 0 .. K - 1 strictly in that order.  u0 = used[b] on entry; a row >= b * cap + u0 is FRESH (made by
 *   an earlier path of this launch: its record and its header do not exist yet).  P(x) = the number of earlier paths of this launch
 *   that pass through or end at node x (the in-flight count); 0 everywhere when the launch starts.  Path k walks from the root as in
 *   snac_uct_select, except:
 *     - arriving at a fresh row stops the path there: leaf = that row, not expanded, first_slot[s] = the slot that expanded it;
 *     - U of child a of node n is, in float64, no contraction, in this order:
 *         Np = N_c + P_c;  q = (W_c - virtual_loss * (double)P_c) / (double)Np;  e = log_table[N(n) + P(n)] * rsqrt_table[Np];
 *         U = q + c * e     (table indices clamped as above; ties: the lowest a; every P = 0 gives snac_uct_select's U bit for bit);
 *     - when the path has its leaf, P += 1 on every node of the path, the leaf included, and an expansion (child[a] = the new row,
 *       used[b] += 1) is visible to path k + 1.
 *   Outputs per slot as snac_uct_select's, with dst = B * cap + s when not expanded, and: an expanded slot has first_slot[s] = s; a
 *   slot that is neither expanded nor on a fresh leaf has first_slot[s] = -1.  A not-expanded slot's src is its leaf, EXCEPT on a fresh
 *   leaf, where src is the tree's root row (the fresh row is the destination of its expander's edge in the same transition launch,
 *   and no destination may be another edge's source); its r_leaf is 0 there (unused).  The caller's tables must reach
 *   N(root) + K: table_len > the largest visit count + K.
 *   Backup, per tree: first every expanded slot's row is written whole as in snac_uct_backup; then paths k = 0 .. K - 1 in that order
 *   each walk from their leaf to the root as there (G = est[s]).  Shared ancestors receive their additions in slot order.  After the
 *   backup every in-flight count is 0 again.
 *   Where P lives: P of child a of node n is n's zero[1 + a], counted up by the selection on the way down and cleared by the backup's
 *   walks; a node's own P is that entry of its parent and the root's is k.  zero[0] of a fresh row holds its expander's slot until the
 *   backup writes the row.  The one-path entry points and snac_uct_advance neither read nor write these words (advance moves them,
 *   zero, bit for bit).
 *   Checks before any HIP call: those of the one-path entry points with B * (cap + paths) rows; paths >= 1; B * paths within int32;
 *   virtual_loss finite; first_slot non-null.
 * PUCT: a caller's policy / value function in place of UCB1 and the rollout (snac_uct_select_puct / snac_uct_set_priors; UCTSearch(evaluator=)).
 *   A node carries a prior per action (prior[a], float32, words 48-55).  An iteration is
 *     snac_uct_select_puct -> snac_transition_nodes* (B * K edges) -> snac_observe_nodes* (the B * K leaves) -> the caller's function:
 *     priors [B * K][A], value [B * K] -> est[s] = (double)first[s] + (leaf_terminal[s] ? 0 : (double)value[s]), where first[s] =
 *     first_slot[s] >= 0 ? reward[first_slot[s]] : r_leaf[s] and leaf_terminal[s] = first_slot[s] >= 0 ? done[first_slot[s]] : the leaf's
 *     stored terminal -> snac_uct_backup_paths (unchanged: an expanded row is written whole, priors zero) -> snac_uct_set_priors on the
 *     expanded slots' rows.  A root gets its priors when it is made (reset / re-rooting by an untried action).
 *   snac_uct_select_puct: one entry point for every paths >= 1 (K = 1: every P is 0).  Slots, scratch rows, fresh rows, first_slot, the
 *   in-flight counts and every output are those of snac_uct_select_paths; it differs only at a non-terminal node n that was not reached
 *   as a fresh row.  There, in float64, no contraction, in this order, for every action a in [0, num_actions):
 *         tried (child[a] >= 0):  Np = N_a + P_a;   q = (W_a - virtual_loss * (double)P_a) / (double)Np
 *         untried:                Np = 0;           q = first_play_value
 *         e = ((double)prior_n[a] * sqrt_table[N(n) + P(n)]) * inv_table[Np];    U = q + c * e
 *     (table indices clamped to [0, table_len - 1]; the caller computes sqrt_table[i] = sqrt(max(i, 1)), inv_table[i] = 1 / (1 + i)).
 *     best = the largest U, ties to the lowest a.  Then:
 *       - best untried and used[b] < cap: expand best (not the lowest untried action) into row b * cap + used[b], as
 *         snac_uct_select_paths expands;
 *       - best untried and the budget spent: best = the largest U over the tried children only (ties to the lowest a); none: stop, leaf = n;
 *       - best tried: descend, P += 1 as there; arriving at a fresh row stops the path as there.
 *   Checks before any HIP call: those of snac_uct_select_paths; first_play_value finite.
 *   snac_uct_set_priors: for i in [0, m), node rows[i] gets prior[a] = priors[i * num_actions + a] (a >= num_actions: 0); with
 *   only_unvisited != 0 a node whose visits != 0 is left alone; a rows[i] outside [0, stats_rows) is skipped (how a caller masks the
 *   slots that did not expand: the backup has already counted a visit on every leaf).  One 32-byte span per node; no other word
 *   changes.  Checks before any HIP call: num_actions 3, 5 or 8; stats non-null and 128-byte aligned; stats_rows >= 1; m >= 0; rows and
 *   priors non-null.  snac_uct_advance moves the priors of a kept node with it, bit for bit.
 * Self-play: moves sampled from the visit counts, new episodes in finished trees, value targets (snac_uct_pick_moves / snac_uct_restart /
 *   snac_uct_returns, k_uct_play.hip; snac_amd/selfplay.py: SelfPlay).  A move of every tree is
 *     iterations -> snac_observe_nodes* (the B roots) -> snac_uct_pick_moves -> snac_transition_nodes* (the B root edges) -> snac_uct_advance
 *                -> snac_reset of the finished trees' env rows -> snac_nodes*_pack into the scratch rows -> snac_uct_restart
 *   on one stream, with no host synchronisation.  All three check every argument before any HIP call.
 *   snac_uct_pick_moves: one move per tree from its root's statistics.  R = row b * cap, N_a = R.child_visits[a] for a < num_actions (zero
 *     where untried; a negative word reads as zero), total = the sum of the N_a as an unsigned 64-bit integer.  Outputs, each may be NULL:
 *       pi[b][a]  = total ? (float)((double)N_a / (double)total) : 0
 *       value[b]  = R.visits ? (float)(R.value_sum / (double)R.visits) : 0
 *       action[b] = 0 when total == 0;  the lowest a with the largest N_a when greedy is NULL or greedy[b] != 0;  otherwise proportional to
 *                   the visits, in integers only: w = word(seed, 3, env_id_base + b, t) of the counter RNG above (desc supplies seed and
 *                   env_id_base; t is the caller's move counter), u = ((uint64)w * total) >> 32 (in [0, total)), action = the lowest a
 *                   with N_0 + ... + N_a > u.  An action with N_a = 0 is never drawn; action a is drawn for floor or ceil of
 *                   2^32 * N_a / total of the 2^32 words.
 *     No floating point enters the choice.  The statistics are READ ONLY.  With action, pi and value all NULL nothing is launched.
 *     Checks: desc non-null; num_actions 3, 5 or 8; stats non-null and 128-byte aligned; B >= 1; cap >= 1; B * (cap + 1) within stats_rows
 *     and int32.
 *   snac_uct_restart: a new episode in the trees with mask[b] != 0.  The caller has just loaded each tree's new start state into its scratch
 *     record B * cap + b (the convention of snac_uct_advance for an untried action).  For a masked tree that record goes to row b * cap byte
 *     for byte; the root's statistics row is written whole (children -1, child visits and values 0, parent -1, action -1, terminal =
 *     terminal[b] != 0 (terminal NULL: 0), visits 0, W 0, reward 0, every zero[] word 0, the priors included); used[b] = 1.  A tree with
 *     mask[b] == 0 keeps every byte: statistics, records, used[b].  Rows [b * cap + 1, (b + 1) * cap) of a restarted tree hold unspecified
 *     contents, as after snac_uct_advance.  Checks: those of snac_uct_advance for stats, records, record_bytes and record_rows; mask and
 *     used non-null.
 *   snac_uct_returns: value targets from a ring of cap_moves slots of [B] rewards and dones, for the `count` slots from `first` (the
 *     oldest) on, modulo cap_moves.  Per tree, from the newest of them back to the oldest, in float64 with no contraction:
 *       g = (double)bootstrap[b] (bootstrap NULL: 0);  at each slot  g = (double)reward + (done ? 0.0 : gamma * g),  z = (float)g.
 *     Slots outside the count are not written.  Checks: B >= 1; cap_moves >= 1; B * cap_moves within int32; first in [0, cap_moves); count in
 *     [0, cap_moves]; gamma finite; reward, done and z non-null.  count == 0: nothing is launched.
 * Reanalyse: stored positions searched again, n-step value targets (snac_uct_save_roots / snac_uct_load_roots / snac_uct_store_targets /
 *   snac_uct_returns_nstep, k_uct_reanalyse.hip; UCTSearch.load_roots(), SelfPlay(keep_states=True).reanalyse() / targets(td_steps=n)).  A
 *   node record is a complete state (header with the plan row, episode counter, grid; the plan table stays in the env), so a ring that
 *   keeps each move's root record can be searched again after the env rows have moved on:
 *     play:      ... iterations -> snac_uct_save_roots (into the ring slot) -> snac_uct_pick_moves -> ... as "Self-play"
 *     reanalyse: snac_uct_load_roots (R trees of a second search <- R ring entries) -> iterations -> snac_uct_store_targets
 *   on one stream, with no host synchronisation.  All four check every argument before any HIP call and never wait for the device.
 *   snac_uct_save_roots: out[b] <- the record of row b * cap, byte for byte, for b in [0, B): B records of record_bytes, one run.  The
 *     records are READ ONLY.  Checks: B >= 1; cap >= 1; B * (cap + 1) within int32 and record_rows; records non-null and 128-byte aligned;
 *     record_bytes 128 or 896; out non-null and 128-byte aligned.
 *   snac_uct_load_roots: tree b starts over from a stored record.  s = index ? clamp(index[b], 0, src_rows - 1) : b.  Record src[s] goes,
 *     byte for byte, to row b * cap and to the tree's scratch row B * cap + b; the root's statistics row is written whole exactly as
 *     snac_uct_restart writes it, with terminal = (word 0 of the record >> 16) & SNAC_FLAG_NEED_RESET (the header's flags byte); used[b] = 1.
 *     Every tree is loaded; several trees may name one s.  Rows [b * cap + 1, (b + 1) * cap) hold unspecified contents afterwards, as
 *     after snac_uct_restart.  src is READ ONLY and must not overlap records: an overlap of [src, src + src_rows * record_bytes) with
 *     [records, records + record_rows * record_bytes) is rejected.  Checks: those of snac_uct_restart for num_actions, stats, B, cap,
 *     records, record_bytes, record_rows and used; src non-null and 128-byte aligned; src_rows >= 1; src_rows >= B when index is NULL.
 *   snac_uct_store_targets: tree b writes ring entry e = index[b]; an e outside [0, entries) is skipped.  With R = row b * cap:
 *       pi[e][a]  = policy ? policy[b * num_actions + a] : (total ? (float)((double)N_a / (double)total) : 0)     (snac_uct_pick_moves' pi)
 *       value[e]  = R.visits ? (float)(R.value_sum / (double)R.visits) : 0                                        (snac_uct_pick_moves' value)
 *       refreshed[e] += 1                                                                                        (int32)
 *     The statistics are READ ONLY.  The entries must be distinct: where two trees name one e, which of them wins, and whether refreshed
 *     counts one or both, is unspecified.  Checks: num_actions, stats, B, cap and rows as snac_uct_pick_moves; index non-null; entries >= 0;
 *     pi, value and refreshed non-null.  entries == 0: nothing is launched.
 *   snac_uct_returns_nstep: MuZero's n-step value target z_t = sum_{k<n} gamma^k r_{t+k} + gamma^n v_{t+n} over the ring of snac_uct_returns,
 *     for the `count` slots from `first` on (modulo cap_moves); slot i below is ring slot (first + i) % cap_moves, i = 0 the oldest.  Per
 *     tree b and slot i, in float64 with no contraction:
 *       e = min(i + n, count);   g = e < count ? (double)value[slot e][b] : (bootstrap ? (double)bootstrap[b] : 0.0)
 *       for j = e - 1 down to i:   g = (double)reward[slot j][b] + (done[slot j][b] ? 0.0 : gamma * g)
 *       z[slot i][b] = (float)g
 *     Hence n >= count gives snac_uct_returns bit for bit, and a window that crosses the end of an episode stops there.  Slots outside the
 *     count are not written; z must not alias value.  Checks: those of snac_uct_returns; n >= 1; value non-null.  count == 0: nothing is
 *     launched.
 * Exploration noise: self-play's root noise, Gumbel scores and move temperature from the counter RNG (snac_explore_root_dirichlet /
 *   snac_explore_gumbel_scores, k_explore.hip; snac_explore_pick_moves_temp, k_uct_play.hip; explore_rule.h states the rules once, for the kernels
 *   and for a host compiler; UCTSearch.add_dirichlet_noise() / gumbel_scores(t=) / pick_moves(temperature=), SelfPlay(dirichlet=,
 *   temperature=, counter_noise=)).  One launch each on the caller's stream, no host synchronisation, every draw keyed by env_id_base + b:
 *   a shard of the trees draws what the same trees draw in the whole batch.  All three check every argument before any HIP call.
 *   Everything is float64, every operation rounded on its own (no fused multiply-add), left to right as parenthesised.
 *     U(w)    = ((double)w + 0.5) * 2^-32                          (exact; in (0, 1))
 *     LOGP(s) = LOG's sequence of operations ("Acting from a policy") for every positive normal float64 s: frexp takes the exponent, the
 *               fold at sqrt 1/2 keeps |z| < 0.1716, so the truncated series leaves less than 2.3e-19 everywhere, and with its roundings the result is
 *               within 2.3e-19 + 17 * 2^-53 * (0.3466 + |log s|) of log s.  Here s runs from 2^-33 (U of word 0) to 2^31.
 *     Streams 6 (Dirichlet) and 7 (Gumbel scores) of the counter RNG; slot (b, a) draws with the env key (env_id_base + b) * 8 + a (the
 *     factor is 8 for every A; unsigned 64-bit wrap-around).  The temperature move keeps stream 3 and snac_uct_pick_moves' key.
 *   log of a Gamma(alpha, 1) draw of slot (b, a) at move t with at most R attempts:
 *     boost = alpha < 1;  a1 = boost ? alpha + 1.0 : alpha;  d = a1 - 1.0 / 3.0;  c = 1.0 / sqrt(9.0 * d)     (once per call, on the host)
 *     attempt j = 0 .. R - 1, until one is accepted; w_k = word(seed, 6, key, t * 128 + 4 * j + k) (the counter in 32-bit wrap-around):
 *       u1 = U(w_0), u2 = U(w_1), u3 = U(w_2);   x = (1.7156 * (u2 - 0.5)) / u1;   x2 = x * x         (the ratio-of-uniforms normal)
 *       s = 1.0 + c * x;   v = (s * s) * s;   lv = LOGP(v > 0 ? v : 1.0)
 *       accepted when  x2 <= -4.0 * LOGP(u1)  and  v > 0  and  LOGP(u3) < ((0.5 * x2 + d) - d * v) + d * lv      (Marsaglia and Tsang)
 *     lg = LOGP(d) + lv of the accepted attempt; with none accepted lg = LOGP(d).  An attempt is accepted with probability about 0.70.
 *     boost: lg = lg + LOGP(U(word(seed, 6, key, t * 128 + 3))) / alpha                                (word 3 of attempt 0)
 *   snac_explore_root_dirichlet: for every tree with mask[b] != 0 (mask NULL: every tree), R = row b * cap, p_a = R.prior[a] for a < num_actions:
 *     the row is bad when some p_a is a NaN, infinite or negative (-0.0 is a zero), or no p_a > 0: it keeps every byte and adds one to
 *     bad_rows[0] (int32 on the device, an atomic add; bad_rows may be NULL).  Otherwise, with the support {a : p_a > 0}:
 *       l_a   = (float)lg_a on the support, -inf elsewhere          (a Gamma draw per action of the support only)
 *       m, x_a = (double)l_a - (double)m, e_a = EXP(x_a), S = e_0 + ... + e_{A-1} from 0.0: the softmax of "Acting from a policy"
 *       eta_a = e_a / S;   p'_a = (float)(om * (double)p_a + eps * eta_a)  with  om = 1.0 - eps  (once per call): three rounded operations
 *     R.prior[a] = p'_a on the support; a prior outside it keeps its bits.  Only these A words of the root row may be written.
 *     Checks: desc non-null; those of snac_uct_pick_moves for num_actions, stats, B, cap and the rows; alpha in [2^-10, 2^10]; eps in
 *     [0, 1]; attempts in [1, 32].  With eps == 0 and bad_rows NULL there is nothing to write and nothing is launched.
 *   snac_explore_gumbel_scores: scores[b][a] for a < num_actions, float32 [B][num_actions], from the roots' priors, which are READ ONLY:
 *       p_a finite and > 0:  (float)(LOGP((double)p_a) + n),   n = noisy[b] != 0 (noisy NULL: everywhere) ?
 *                            -LOGP(-LOGP(U(word(seed, 7, key, t)))) : 0.0
 *       p_a == 0: -inf;   a NaN, a negative or an infinite p_a: NaN      (snac_uct_gumbel_candidates ranks a NaN as -inf)
 *     Checks: desc non-null; num_actions, stats, B, cap and the rows as above; scores non-null.
 *   snac_explore_pick_moves_temp: snac_uct_pick_moves with a temperature: pi and value are exactly its outputs, and so is action where total == 0
 *     or the tree is greedy by the mask.  Otherwise T = temperature ? (double)temperature[b] : temp, and with w the same stream-3 word:
 *       a NaN or T <= 0: the greedy rule;   T == 1: the integer rule of snac_uct_pick_moves, bit for bit;   else, with r = 1.0 / T and
 *       N_max the largest count:
 *         w_a   = N_a == N_max ? 2^28 : N_a > 0 ? (uint64)floor(EXP((LOGP((double)N_a) - LOGP((double)N_max)) * r) * 2^28) : 0
 *         total = w_0 + ... + w_{A-1}  (in [2^28, 2^31]);   u = ((uint64)w * total) >> 32;   action = the lowest a with w_0 + ... + w_a > u
 *       T = +inf draws uniformly over the visited actions (r = 0: every visited action weighs 2^28).
 *     Checks: those of snac_uct_pick_moves; temp >= 0, finite or +inf (a NaN is rejected).  With action, pi and value all NULL nothing is
 *     launched.
 * Prioritised replay: a 64-ary sum tree of integer weights in device memory, updated and sampled in O(log64 entries) per item with no
 *   host synchronisation (snac_prio_layout / snac_prio_init / snac_prio_update / snac_prio_fill / snac_prio_sample, k_prio.hip;
 *   snac_amd/priority.py PriorityTree, SelfPlay(prioritized=True), ReplayRing(prioritized=True)).
 *   Weights.  An entry's weight is a uint32; every sum is a uint64, hence exact and independent of the order of its terms.  A float
 *     priority p becomes a weight by quant(p, s), s = scale_log2 in 0 .. 31:
 *         p == 0 -> 0 (the entry cannot be drawn);   NaN or p < 0 -> 1;   otherwise min(max(rint((double)p * 2^s), 1), 2^32 - 1)
 *     (the multiply by a power of two is exact in float64; rint rounds half to even).
 *   The buffer: caller-owned, 128-byte aligned, snac_prio_layout's `bytes` long, uint64 words:
 *         head     128 bytes: word 0 = max_weight, the largest weight any snac_prio_update has stored (2^s, priority 1.0, after
 *                  snac_prio_init); word 1 = entries; word 2 = the number of sum levels; words 3 .. 15 = 0
 *         leaves   uint32[E64], E64 = entries rounded up to a multiple of 64               (level_offset[0] = 128)
 *         level 1  uint64[n_1 rounded up to a multiple of 64], n_1 = E64 / 64: value g = the sum of leaves 64 g .. 64 g + 63
 *         level l+1  uint64[n_{l+1} rounded up to a multiple of 64], n_{l+1} = ceil(n_l / 64): value g = the sum of level l's
 *                  values 64 g .. 64 g + 63;  the last level has n = 1: its value 0 is the total T
 *     Every level starts 128-byte aligned and all padding is zero.  entries is in [1, 2^31 - 64], so T < 2^63 and there are at most 6
 *     sum levels.  The entry points take `entries` (and scale_log2) by value and derive the layout from it: the head is for readers.
 *   snac_prio_layout (host only, no HIP call): bytes, levels (sum levels), level_offset[8] = bytes from the buffer's start of the
 *     leaves ([0]) and of sum level l ([l], l = 1 .. levels); the unused offsets are 0.
 *   snac_prio_init: writes the head and zeroes everything else (one launch).
 *   snac_prio_update: for j < n with i = index[j] in [0, entries) (any other index is skipped): leaf i <- quant(priority[j], s); where
 *     an index occurs more than once in a call the largest weight wins; max_weight <- max(max_weight, the weights stored).  Then every
 *     sum above a touched leaf is recomputed from its 64 children.  Launches, in stream order: the indexed leaves <- 0; atomic max of
 *     the weights into the leaves (and one atomic max per wavefront into max_weight); then one launch per sum level, one wavefront per
 *     parent (lane = child, a wave reduction, one lane stores): the parent of each index, or, where the level has no more values
 *     than n, all of them.  Duplicate parents do identical work.
 *   snac_prio_fill: entries [first, first + count) <- one weight: priority < 0: the head's max_weight as it stands on the device (new
 *     transitions get the largest priority seen); priority == 0: 0; otherwise quant(priority, s).  Then the sums above them, a
 *     contiguous range of each level, one launch per level; count = entries rebuilds the tree.  max_weight is not changed; the span does
 *     not wrap.
 *   snac_prio_sample: sample j < n draws with r as under "Counter RNG", stream 4.  With T the total, q = T / n and rem = T % n:
 *         stratified != 0 and q >= 1:  lo = j * q + min(j, rem);  len = q + (j < rem);  u = lo + mulhi64(r, len)
 *         otherwise:                   u = mulhi64(r, T)                        (mulhi64: the high 64 bits of the 128-bit product)
 *     index[j] = the lowest i with w_0 + ... + w_i > u, found from the top group down: at each level the lowest child whose inclusive
 *     prefix sum within its group of 64 exceeds u, then u less that child's exclusive prefix.  prob[j] = (float)((double)w_i / (double)T);
 *     weight[j] = w_i (weight may be NULL).  T == 0: index -1, prob 0, weight 0.  An entry of weight 0 is never drawn.  The tree is
 *     READ ONLY.  Sums that do not match their children (a buffer written by other means) give index -1, never an index out of range.
 *   Checks before any HIP call: tree non-null and 128-byte aligned; entries in [1, 2^31 - 64]; scale_log2 in 0 .. 31 (init, update,
 *     fill); n >= 0, index and priority non-null (update); first in [0, entries), count in [0, entries - first], priority not NaN
 *     (fill); draw in [0, 2^31), n >= 0, index and prob non-null (sample); the outputs non-null (layout).  n == 0 / count == 0: nothing
 *     is launched.
 * Normalised q: per-tree min-max bounds of the mean values, so that U does not depend on the reward scale (snac_uct_select_paths_norm /
 *   snac_uct_select_puct_norm / snac_uct_backup_paths_norm / snac_uct_bounds; UCTSearch(q_normalise=True)).
 *   The bounds array: caller-owned, 2 * B float64, 16-byte aligned; bounds[2 * b] = lo, bounds[2 * b + 1] = hi of tree b; the empty pair
 *     is (+inf, -inf).  The bounds are not part of snac_uct_node: snac_uct_advance / snac_uct_restart do not know them.
 *   Selection (snac_uct_select_paths_norm / snac_uct_select_puct_norm: the arguments of snac_uct_select_paths / snac_uct_select_puct and
 *     `bounds`, read only).  Tree b's pair is read once when the launch starts.  Everything is as in the unnormalised entry point, except
 *     that the q of a TRIED child, q = (W_a - virtual_loss * (double)P_a) / (double)Np as there, is normalised before it enters U, in
 *     float64, no contraction, in this order:
 *         if (hi > lo) q = (q - lo) / (hi - lo);      (hi - lo computed once per tree; otherwise q is unchanged)
 *     No clamp: with virtual loss q may leave [0, 1].  An untried action's first_play_value is used as given: it is in normalised
 *     units.  Ties, table clamping, expansion, fresh rows, in-flight counts and every output are unchanged; with the empty pair or
 *     hi == lo the outputs equal the unnormalised entry point's bit for bit.  There is no _norm form of the one-path snac_uct_select:
 *     snac_uct_select_paths_norm with paths = 1 is that search (every P = 0).
 *   Backup (snac_uct_backup_paths_norm: snac_uct_backup_paths and `bounds`, read and written).  The walks are those of
 *     snac_uct_backup_paths.  In addition, right after a node x with a parent (parent >= 0: not the root) has its new visits and
 *     value_sum, m = value_sum / (double)visits enters the tree's pair:
 *         lo = m < lo ? m : lo;   hi = m > hi ? m : hi;      (a NaN fails both comparisons and never enters)
 *     in slot order, then walk order; the pair is written back once per launch.  The root stays out because no selection compares its
 *     mean; the means below it are exactly the W_a / N_a that selection compares (the mirrors in the parents).
 *   Bounds from a tree as it stands (snac_uct_bounds; mask NULL: every tree).  For every tree with mask[b] != 0: lo / hi = the smallest /
 *     largest value_sum / (double)visits over rows b * cap + 1 .. b * cap + used[b] - 1 with visits > 0, by the comparisons above (used[b]
 *     clamped into [1, cap]); no such row: the empty pair.  Every other tree keeps its pair bit for bit.  After snac_uct_advance a
 *     kept subtree so gets the bounds of its own nodes, and a one-node tree (an untried action, snac_uct_restart) the empty pair.
 *   Checks before any HIP call: the _norm forms run the checks of the entry point they extend, then bounds non-null and 16-byte aligned.
 *     snac_uct_bounds: used non-null; stats non-null and 128-byte aligned; B >= 1; cap >= 1; B * (cap + 1) within stats_rows and int32;
 *     bounds non-null and 16-byte aligned.
 * Gumbel root: sequential halving over sampled root actions in place of PUCT at the root (Danihelka et al. 2022, Gumbel AlphaZero;
 *   snac_uct_select_gumbel, k_uct.hip; snac_uct_gumbel_candidates, k_uct_play.hip; UCTSearch(gumbel=m), SelfPlay(gumbel=True)).  A move is
 *     BEGIN -> per phase: [HALVE ->] iterations of (snac_uct_select_gumbel -> edges -> evaluator -> snac_uct_backup_paths_norm ->
 *     snac_uct_set_priors) -> PICK
 *   on one stream, with no host synchronisation.  The candidate array: caller-owned, B int32; bit a of cand[b] = root action a of tree b is
 *   a candidate; only bits below num_actions count.  It is not part of snac_uct_node: the caller zeroes it when a tree gets a new root.
 *   Selection (snac_uct_select_gumbel: the arguments of snac_uct_select_puct_norm, then `cand`, read only, and `offset`).  cand[b] is read
 *     once when the launch starts, beside the bounds pair; no level waits for that load.  cand[b] == 0 (below num_actions): tree b is
 *     selected exactly as by snac_uct_select_puct_norm, every output and statistics word bit for bit.  Otherwise let c_0 < ... < c_{M-1}
 *     be the candidates: path k of the launch takes the root action a = c[(offset + k) mod M] (integers only; no U is computed at the
 *     root).  A terminal root stops as before.  a tried: the path descends to it.  a untried and used < cap: a is expanded exactly as
 *     snac_uct_select_puct expands its best action.  a untried and the budget spent: the path stops at the root (leaf = src = the root,
 *     not expanded, first_slot = -1, r_leaf = the root's reward).  The root rule ignores the in-flight counts but counts them as before;
 *     slots, scratch rows, fresh rows, first_slot and every output are those of snac_uct_select_puct.  Below the root (depth >= 1) the
 *     rule is snac_uct_select_puct_norm's, unchanged.  Checks before any HIP call: those of snac_uct_select_puct_norm, then cand non-null,
 *     offset >= 0, offset + paths within int32.
 *   Candidates (snac_uct_gumbel_candidates): lane = tree, the statistics READ ONLY.  scores[b * A + a] (A = num_actions) is the caller's
 *     g(a) + logit(a) in float32; a NaN reads as -inf.  "The n largest of a set by x" below means: n times, take the member with the
 *     largest x among those not yet taken, by strict > scanning a upward (ties to the lowest a).
 *       mode 0, BEGIN:  cand[b] = 0 at a terminal root, else the min(m, A) largest of all actions by score.  Of the statistics only the
 *                       root's terminal word is read.
 *       mode 1, HALVE:  with M = popcount(cand[b]) (bits below A), cand[b] = the (M + 1) / 2 largest of the candidates by RANK.
 *       mode 2, PICK:   action[b] = the largest of the candidates by RANK; cand is not written.  cand[b] == 0: the lowest a with the
 *                       largest child_visits[a] (a negative word reads as zero), 0 when there are none -- the greedy snac_uct_pick_moves.
 *     RANK of action a at the root R, in float64, no contraction, in this order (lo, hi: the tree's pair of `bounds`):
 *         maxN = the largest max(R.child_visits[a'], 0) over a' < A with R.child[a'] >= 0 (none: 0)
 *         visited = R.child[a] >= 0 && R.child_visits[a] > 0
 *         q = visited ? R.child_value[a] / (double)R.child_visits[a] : first_play_value;   if (visited && hi > lo) q = (q - lo) / (hi - lo)
 *         s1 = c_visit + (double)maxN;  s2 = s1 * c_scale;  sig = s2 * q;  rank = (double)score + sig;  a NaN rank reads as -inf
 *     Checks before any HIP call: num_actions, stats, B, cap and rows as snac_uct_pick_moves; mode in 0 .. 2; m >= 1 for BEGIN; scores
 *     non-null; c_visit, c_scale and first_play_value finite; bounds non-null and 16-byte aligned for HALVE and PICK; cand non-null;
 *     action non-null for PICK.
 * Gumbel interior: the Gumbel rule below the root as well, and the improved policy with the full v_mix (Danihelka et al. 2022, Gumbel
 *   MuZero, section 5 and appendix D; snac_uct_set_priors_value / snac_uct_select_gumbel_interior / snac_uct_improved_policy, k_uct.hip;
 *   UCTSearch(gumbel=m, gumbel_interior=True)).  An iteration is that of "Gumbel root" with snac_uct_select_gumbel_interior in place of
 *   snac_uct_select_gumbel and snac_uct_set_priors_value in place of snac_uct_set_priors.
 *   The network value: words 56-57 of a node (net_value, float64) hold the value the evaluator gave for the node's state, 0 for a terminal
 *     node.  snac_uct_set_priors_value (the arguments of snac_uct_set_priors, and `value`, m float64, before only_unvisited) is
 *     snac_uct_set_priors and, for the same rows under the same skip rules, net_value <- value[i] (one 8-byte store; no other word
 *     changes).  snac_uct_advance moves the words with a kept node bit for bit; the backups and snac_uct_restart, which write an expanded
 *     or restarted row whole, zero them; no other entry point reads or writes them.  Checks before any HIP call: those of
 *     snac_uct_set_priors, then value non-null.
 *   The improved policy pi' of a non-terminal node n, in float64, no contraction, in this order (lo, hi: the tree's pair of `bounds`;
 *     P_a: the in-flight count of child[a], every P_a = 0 in snac_uct_improved_policy; v = n.net_value; p_a = (double)prior_n[a]):
 *         has_a = child[a] >= 0;  N_a = has_a ? max(child_visits[a], 0) : 0;  P_a = has_a ? in-flight : 0;  vis_a = has_a && N_a > 0
 *         sumN = sum N_a;  sumP = sum P_a;  maxN = max N_a        (int32, a ascending: the caller keeps sumN + sumP within int32)
 *         q_a  = W_a / (double)N_a                                  (vis_a only)
 *         sp = sum_{vis} p_a;  spq = sum_{vis} p_a * q_a;  sW = sum_{vis} W_a        (a ascending, from 0.0)
 *         vmix = sumN == 0 ? v : (v + (double)sumN * (sp > 0 ? spq / sp : sW / (double)sumN)) * inv_table[sumN]
 *         qh_a = vis_a ? q_a : vmix;      if (hi > lo) qh_a = (qh_a - lo) / (hi - lo)      (hi - lo computed once per tree)
 *         s1 = c_visit + (double)maxN;  s2 = s1 * c_scale;  sig_a = s2 * qh_a
 *         smax = -inf;  for a ascending: if (sig_a > smax) smax = sig_a                    (a NaN never wins)
 *         e_a = p_a * uct_exp(sig_a - smax);   Z = sum e_a (a ascending, from 0.0);   pi_a = Z > 0 ? e_a / Z : 0
 *     This is softmax(log p + sig) without a logarithm.  inv_table[i] = 1 / (1 + i) is PUCT's table, its index clamped as there;
 *     snac_uct_improved_policy takes no table and computes 1.0 / (1.0 + (double)sumN), the table's entry wherever sumN < table_len.
 *     uct_exp(x), made of float64 + - *, floor and ldexp alone so that a host restatement reproduces it bit for bit (within 1 ulp of exp
 *     on [-700, 0]): a NaN x or x < -700.0 gives 0.0; x > 0 reads as 0; k = floor(x * LOG2E + 0.5); r = (x - k * LN2_HI) - k * LN2_LO with
 *     LOG2E = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33; p = the Horner sum of r^i / i! from
 *     i = 13 down to 0 (p = 1.0 / 13!; p = p * r + 1.0 / i!, the coefficients the float64 quotients 1.0 / i!); the result is ldexp(p, k).
 *   Selection (snac_uct_select_gumbel_interior: the arguments of snac_uct_select_gumbel, then c_visit and c_scale).  A root with
 *     candidates (cand[b] != 0) takes its turn action; slots, scratch rows, fresh rows, first_slot, in-flight counts, every output, the
 *     stop at a terminal node and the stop on a fresh row are those of snac_uct_select_gumbel.  At every other non-terminal node -- every
 *     depth >= 1, and a root with cand[b] == 0 -- no U is computed (c, virtual_loss, first_play_value and sqrt_table are checked but not
 *     used): with pi' as above,
 *         score_a = pi_a - (double)(N_a + P_a) * inv_table[sumN + sumP]                    (index clamped)
 *     best = the largest score by strict >, ties to the lowest a, and the code continues as after PUCT's U: best untried and
 *     used[b] < cap: expand it; best untried and the budget spent: the best of the tried children by score, none: stop; best tried:
 *     descend, P += 1.  Checks before any HIP call: those of snac_uct_select_gumbel, then c_visit and c_scale finite.
 *   snac_uct_improved_policy: for i in [0, m), pi[i * A + a] = (float)pi_a of node rows[i], the bounds those of tree rows[i] / cap; a row
 *     outside [0, B * cap) or a terminal node gives zeros.  The statistics are READ ONLY.  Checks before any HIP call: num_actions 3, 5 or
 *     8; stats non-null and 128-byte aligned; B >= 1; cap >= 1; B * (cap + 1) within stats_rows and int32; m >= 0; rows non-null; c_visit
 *     and c_scale finite; bounds non-null and 16-byte aligned; pi non-null.  m == 0: nothing is launched. */
typedef struct snac_uct_node {  /* 256 bytes, 128-byte aligned: line 0 is all that selection compares, line 1 the node's own header */
    int32_t child[8];           /* row of the child through action a, -1 = untried (a >= num_actions: always -1) */
    int32_t child_visits[8];    /* N of child[a] */
    double child_value[8];      /* W of child[a] */
    int32_t parent;             /* -1 at a root */
    int32_t action;             /* the edge from the parent (-1 at a root) */
    int32_t terminal;           /* the edge's done (a root: its record's SNAC_FLAG_NEED_RESET) */
    int32_t visits;             /* N */
    double value_sum;           /* W */
    float reward;               /* the edge's transition reward, 0 at a root */
    int32_t zero[25];           /* zero[0 .. 8]: in-flight counts during a multi-path iteration (zero[1 + a]: of child[a]; zero[0]: a fresh
                                   row's expander slot), zero outside one.  zero[9 + a] (words 48-55 of the record, pieces 12 and 13): the
                                   PUCT prior of action a as a float32 bit pattern (snac_uct_set_priors; a >= num_actions: 0); the
                                   rollout search never writes these words: zero there.  zero[17 .. 18] (words 56-57, byte 224, the first
                                   half of piece 14): net_value, the float64 value the evaluator gave for this node's state, 0 for a
                                   terminal node (snac_uct_set_priors_value; zero in every search that does not call it).
                                   zero[19 .. 24]: zero */
} snac_uct_node;
#define SNAC_UCT_PRIOR_WORD 48  /* int32 word of prior[0] in a snac_uct_node: ((const float*)node)[SNAC_UCT_PRIOR_WORD + a] */
#define SNAC_UCT_NET_VALUE_WORD 56  /* int32 word of net_value in a snac_uct_node: *(const double*)((const int32_t*)node + 56) */
int snac_uct_select(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, double c, const double* log_table,
                    const double* rsqrt_table, int32_t table_len, int32_t* used, int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf,
                    uint8_t* expanded, float* r_leaf, void* stream);
int snac_uct_backup(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, double gamma, const int32_t* src,
                    const int8_t* action, const int32_t* leaf, const uint8_t* expanded, const float* reward, const uint8_t* done,
                    const double* est, void* stream);
int snac_uct_advance(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, void* records, int32_t record_bytes,
                     int32_t record_rows, const int8_t* actions, const float* edge_reward, const uint8_t* edge_done, int32_t* used,
                     int32_t* work, float* reward_out, uint8_t* done_out, void* stream);

int snac_uct_select_paths(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double c,
                          double virtual_loss, const double* log_table, const double* rsqrt_table, int32_t table_len, int32_t* used,
                          int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf, uint8_t* expanded, float* r_leaf, int32_t* first_slot,
                          void* stream);
int snac_uct_backup_paths(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double gamma,
                          const int32_t* src, const int8_t* action, const int32_t* leaf, const uint8_t* expanded, const float* reward,
                          const uint8_t* done, const double* est, void* stream);

int snac_uct_select_puct(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double c,
                         double virtual_loss, double first_play_value, const double* sqrt_table, const double* inv_table, int32_t table_len,
                         int32_t* used, int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf, uint8_t* expanded, float* r_leaf,
                         int32_t* first_slot, void* stream);
int snac_uct_set_priors(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t m, const int32_t* rows, const float* priors,
                        int32_t only_unvisited, void* stream);


int snac_uct_pick_moves(const snac_env_desc* desc, int32_t num_actions, const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap,
                        const uint8_t* greedy, uint32_t t, int8_t* action, float* pi, float* value, void* stream);
int snac_uct_restart(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, void* records, int32_t record_bytes,
                     int32_t record_rows, const uint8_t* mask, const uint8_t* terminal, int32_t* used, void* stream);
int snac_uct_returns(int32_t B, int32_t cap_moves, int32_t first, int32_t count, double gamma, const float* reward, const uint8_t* done,
                     const float* bootstrap, float* z, void* stream);

int snac_uct_save_roots(int32_t B, int32_t cap, const void* records, int32_t record_bytes, int32_t record_rows, void* out, void* stream);
int snac_uct_load_roots(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, void* records, int32_t record_bytes,
                        int32_t record_rows, const void* src, int32_t src_rows, const int32_t* index, int32_t* used, void* stream);
int snac_uct_store_targets(int32_t num_actions, const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, const int32_t* index,
                           int32_t entries, const float* policy, float* pi, float* value, int32_t* refreshed, void* stream);
int snac_uct_returns_nstep(int32_t B, int32_t cap_moves, int32_t first, int32_t count, int32_t n, double gamma, const float* reward,
                           const uint8_t* done, const float* value, const float* bootstrap, float* z, void* stream);
int snac_explore_root_dirichlet(const snac_env_desc* desc, int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap,
                                const uint8_t* mask, uint32_t t, double alpha, double eps, int32_t attempts, int32_t* bad_rows, void* stream);
int snac_explore_gumbel_scores(const snac_env_desc* desc, int32_t num_actions, const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap,
                               const uint8_t* noisy, uint32_t t, float* scores, void* stream);
int snac_explore_pick_moves_temp(const snac_env_desc* desc, int32_t num_actions, const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap,
                                 const uint8_t* greedy, uint32_t t, const float* temperature, double temp, int8_t* action, float* pi, float* value,
                                 void* stream);

int snac_prio_layout(int32_t entries, int64_t* bytes, int32_t* levels, int64_t* level_offset);
int snac_prio_init(void* tree, int32_t entries, int32_t scale_log2, void* stream);
int snac_prio_update(void* tree, int32_t entries, int32_t scale_log2, const int32_t* index, const float* priority, int32_t n, void* stream);
int snac_prio_fill(void* tree, int32_t entries, int32_t scale_log2, int32_t first, int32_t count, double priority, void* stream);
int snac_prio_sample(const void* tree, int32_t entries, uint64_t seed, int64_t sampler_id, int32_t draw, int32_t n, int32_t stratified,
                     int32_t* index, float* prob, uint32_t* weight, void* stream);

int snac_uct_select_paths_norm(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double c,
                               double virtual_loss, const double* log_table, const double* rsqrt_table, int32_t table_len, int32_t* used,
                               int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf, uint8_t* expanded, float* r_leaf,
                               int32_t* first_slot, const double* bounds, void* stream);
int snac_uct_select_puct_norm(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double c,
                              double virtual_loss, double first_play_value, const double* sqrt_table, const double* inv_table,
                              int32_t table_len, int32_t* used, int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf, uint8_t* expanded,
                              float* r_leaf, int32_t* first_slot, const double* bounds, void* stream);
int snac_uct_backup_paths_norm(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double gamma,
                               const int32_t* src, const int8_t* action, const int32_t* leaf, const uint8_t* expanded, const float* reward,
                               const uint8_t* done, const double* est, double* bounds, void* stream);
int snac_uct_bounds(const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, const int32_t* used, const uint8_t* mask,
                    double* bounds, void* stream);

int snac_uct_select_gumbel(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double c,
                           double virtual_loss, double first_play_value, const double* sqrt_table, const double* inv_table, int32_t table_len,
                           int32_t* used, int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf, uint8_t* expanded, float* r_leaf,
                           int32_t* first_slot, const double* bounds, const int32_t* cand, int32_t offset, void* stream);
int snac_uct_gumbel_candidates(int32_t num_actions, const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t mode, int32_t m,
                               const float* scores, double c_visit, double c_scale, double first_play_value, const double* bounds, int32_t* cand,
                               int8_t* action, void* stream);

int snac_uct_set_priors_value(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t m, const int32_t* rows, const float* priors,
                              const double* value, int32_t only_unvisited, void* stream);
int snac_uct_select_gumbel_interior(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double c,
                                    double virtual_loss, double first_play_value, const double* sqrt_table, const double* inv_table,
                                    int32_t table_len, int32_t* used, int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf,
                                    uint8_t* expanded, float* r_leaf, int32_t* first_slot, const double* bounds, const int32_t* cand,
                                    int32_t offset, double c_visit, double c_scale, void* stream);
int snac_uct_improved_policy(int32_t num_actions, const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t m,
                             const int32_t* rows, double c_visit, double c_scale, const double* bounds, float* pi, void* stream);

#ifdef __cplusplus
}
#endif
#endif
