// k_replay.hip -- the four kernels that build a minibatch out of the replay ring, with what they share stated once at the head of the file:
// snac_replay_gather / _tiled (the tuple of a step; include/snac_hip.h, "Minibatch assembly"), the walks along one env's column of the
// ring, snac_replay_gather_nstep (Rainbow's multi-step transition: s, the discounted sum of up to n rewards, the row to bootstrap from)
// and snac_replay_gather_windows (DRQN's Memory.get_batch: up to L consecutive tuples of one episode that end at the sample; the
// header's "n-step transitions and episode windows"), and snac_replay_gather_onpolicy (PPO's minibatch: s, the plan and five scalars of
// a sample; the header's "On-policy rollouts").
#include <cmath>
#include <cstddef>

#include "snac_units.h"

// All four kernels have one shape: 4 waves a block, S samples a wave, and rounds of loads that each go out for the whole group before
// anything waits on them -- the samples' indices (lane u = sample u), in the walks the flags along the walk (lane k = step k of the walk;
// one ballot turns them into the walk's length), then the rows -- and only then the stores.
namespace {

using namespace snac_detail;

constexpr int S = 4;                                                 // samples per wave
template <int KIND>
constexpr int PC = KIND == 1 ? 30 : 400;                             // float32 cells of an expanded plan row

// what the argument struct of every kernel begins with
struct GHead {
    int32_t n, cap, batch, num_plans;
    int32_t ld, frame_val;                                           // row length (K::D, + the position tail) and frame value of the ring's layout
    int32_t tiled;                                                   // obs is [ceil(n / 64)][cap][64][ld] instead of [cap][n][ld]
    const void* obs;
    const uint8_t* first;
    const int16_t* plan_idx;
    const int32_t* tick;
    const int32_t* env;
    const void* plans;
    float* s;
    float* plan_out;
};

// row (t, i) of the ring, in rows: obs[cap][n][ld], or tile-major obs[ceil(n / 64)][cap][64][ld]
__device__ __forceinline__ size_t ring_row(int tiled, int cap, int n, int t, int i) {
    return tiled ? ((size_t)(i >> 6) * cap + t) * 64 + (i & 63) : (size_t)t * n + i;
}

// lane u < ns holds sample b0 + u of the group: its slot t and env i, clamped into the ring, cur = [t][i] in the [cap][N] arrays, and of
// what stands there as much as the kernel asks for: the step's first flag, its action, and (when plans go out) its clamped plan row p
struct Pick {
    int t, i, first, act, p;
    size_t cur;
};
template <bool FIRST, bool ACT>
__device__ __forceinline__ Pick pick(const GHead& g, const int8_t* action, int b0, int ns, int lane) {
    Pick k = {0, 0, 0, 0, 0, 0};
    if (lane < ns) {
        k.t = min(max(g.tick[b0 + lane], 0), g.cap - 1);
        k.i = min(max(g.env[b0 + lane], 0), g.n - 1);
        k.cur = (size_t)k.t * g.n + k.i;
        if (FIRST) k.first = g.first[k.cur] != 0;
        if (ACT) k.act = action[k.cur];
        if (g.plan_out) k.p = min(max((int)g.plan_idx[k.cur], 0), g.num_plans - 1);
    }
    return k;
}

// value `lane` of the reset observation (the `s` of a step that opened an episode): the window at the start position over an empty
// grid, both scalar slots 0; lane >= D is the position tail: the start position
template <int KIND>
__device__ __forceinline__ float reset_obs(int lane, int frame_val) {
    constexpr int D = KIND == 1 ? 7 : 51, W = KIND == 1 ? 5 : 49;
    const int wi = lane / 7, wj = lane - 7 * wi;
    const bool frame = KIND == 1 ? lane < 2 : (wi < 3 || wj < 3);
    float sv = (lane < W && frame) ? (float)frame_val : 0.0f;
    if (lane >= D) sv = KIND == 1 ? 2.0f : 3.0f;
    return sv;
}

// value `lane` of a step's s: the reset observation where the step opened an episode, else the predecessor row's value
template <int KIND, typename OT>
__device__ __forceinline__ float s_value(int opened, int lane, int frame_val, OT vprev) {
    return opened ? reset_obs<KIND>(lane, frame_val) : (float)vprev;
}

// the plan of sample b0 + u (lane u holds its row p of the table) as float32 cells in plan_out, by one wave
template <int KIND>
__device__ __forceinline__ void expand_plan(const GHead& g, int p, int b0, int u, int lane) {
    const int pu = __builtin_amdgcn_readlane(p, u);
    float* const po = g.plan_out + (size_t)(b0 + u) * PC<KIND>;
    if (KIND == 1) {
        if (lane < PC<KIND>) po[lane] = (float)((const int16_t*)g.plans)[pu * 32 + lane];
    } else {
        // four consecutive cells per lane (a row of 20 holds five such groups): one 16-byte store each, 100 lanes a plan
        for (int q = lane; q < PC<KIND> / 4; q += 64) {
            const int c = q * 4;
            float4 v;
            if (KIND == 2) {
                const int row = c / 20, col = c - row * 20;
                const uint32_t w = ((const uint32_t*)g.plans)[pu * 20 + row] >> col;
                v = make_float4((float)(w & 1u), (float)((w >> 1) & 1u), (float)((w >> 2) & 1u), (float)((w >> 3) & 1u));
            } else {
                const short4 h = *(const short4*)((const int16_t*)g.plans + (size_t)pu * 400 + c);
                v = make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
            }
            *(float4*)(po + c) = v;
        }
    }
}

// the plan tail of a kernel: the plans of the group's ns samples, when plans go out
template <int KIND>
__device__ __forceinline__ void expand_plans(const GHead& g, int p, int b0, int ns, int lane) {
    if (!g.plan_out) return;
#pragma unroll
    for (int u = 0; u < S; ++u) {
        if (u >= ns) break;
        expand_plan<KIND>(g, p, b0, u, lane);
    }
}

// ------------------------------------------------------------------------------------------------
// replay sampling (the step after the env path: script/DQN/2d/DQN_2d_dynamic.py:122-124,145-166 keeps
// (s, a, r, s', plan) tuples in a python deque and re-assembles float32 minibatches on the host).  The rollout output
// ring obs[cap][N][D] already holds every s' -- and s is the previous tick's row, or the constant reset observation when
// the step opened an episode -- so sampling is a gather: float32 out, plan expanded from the table.
struct GArgs : GHead {
    float* s_next;
};

template <int KIND, typename OT>
__global__ __launch_bounds__(256) void k_gather(const GArgs g) {
    // S samples per wave: the index loads of all of them first (lane u = sample u), then every row load of the group in flight
    // before the first store -- one sample per wave was a chain of three dependent loads with a single row in flight.
    const int lane = threadIdx.x & 63;
    const int b0 = ((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * S;   // (alone among the four, not through readfirstlane)
    if (b0 >= g.batch) return;
    const int ns = min(S, g.batch - b0);
    const int LD = g.ld;                                         // D, or D + the position tail (1 / 2 values)
    const OT* o = (const OT*)g.obs;
    const Pick k = pick<true, false>(g, nullptr, b0, ns, lane);
    OT vcur[S], vprev[S];
    int fst[S];
#pragma unroll
    for (int u = 0; u < S; ++u) {
        const int tu = __builtin_amdgcn_readlane(k.t, u), iu = __builtin_amdgcn_readlane(k.i, u);
        fst[u] = __builtin_amdgcn_readlane(k.first, u);
        const int tp = tu == 0 ? g.cap - 1 : tu - 1;
        const size_t ocur = ring_row(g.tiled, g.cap, g.n, tu, iu), oprev = ring_row(g.tiled, g.cap, g.n, tp, iu);
        vcur[u] = (OT)0; vprev[u] = (OT)0;
        if (u < ns && lane < LD) {                                   // guarded loads, and no predecessor where the step opened an episode
            vcur[u] = o[ocur * LD + lane];
            if (!fst[u]) vprev[u] = o[oprev * LD + lane];
        }
    }
#pragma unroll
    for (int u = 0; u < S; ++u) {
        if (u < ns && lane < LD) {
            const size_t b = (size_t)(b0 + u);
            g.s_next[b * LD + lane] = (float)vcur[u];
            g.s[b * LD + lane] = s_value<KIND>(fst[u], lane, g.frame_val, vprev[u]);
        }
    }
    expand_plans<KIND>(g, k.p, b0, ns, lane);
}

// ------------------------------------------------------------------------------------------------
// the two walks (snac_replay_gather_nstep, snac_replay_gather_windows)
struct RArgs : GHead {
    int32_t end;                                                     // n-step: the newest slot; windows: the oldest addressable slot
    int32_t steps;                                                   // n, or L
    double gamma;
    const uint8_t* done;
    const float* reward;
    const int8_t* action;
    float* s_next;
    int64_t* action_out;
    float* reward_out;                                               // n-step: the return
    float* discount_out;
    uint8_t* done_out;
    uint8_t* mask_out;
    int32_t* steps_out;                                              // n-step: m; windows: len
};

template <int KIND, typename OT>
__global__ __launch_bounds__(256) void k_gather_nstep(const RArgs g) {
    const int lane = threadIdx.x & 63;
    const int b0 = ((int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * S;   // in scalar registers: the group's control flow is uniform
    if (b0 >= g.batch) return;
    const int ns = min(S, g.batch - b0);
    const int LD = g.ld;
    const OT* o = (const OT*)g.obs;
    const Pick k = pick<true, true>(g, g.action, b0, ns, lane);      // what step 0 gives: its first flag, action and plan row
    // lane k < n: step k of each sample's walk.  The loads of the whole group stand in one block, before anything reads them (a sample
    // past the batch's end walks from (0, 0): valid addresses, results unused)
    int tu[S], iu[S], sk[S], dnr[S], fnr[S];
    float rw[S];
#pragma unroll
    for (int u = 0; u < S; ++u) {
        tu[u] = __builtin_amdgcn_readlane(k.t, u); iu[u] = __builtin_amdgcn_readlane(k.i, u);
        sk[u] = (tu[u] + lane) % g.cap;
        dnr[u] = 0; fnr[u] = 0; rw[u] = 0.0f;
    }
    if (lane < g.steps) {
#pragma unroll
        for (int u = 0; u < S; ++u) {
            const size_t at = (size_t)sk[u] * g.n + iu[u];
            dnr[u] = g.done[at];
            rw[u] = g.reward[at];
        }
    }
    if (lane + 1 < g.steps) {                                        // step n - 1 stops whatever follows it: one scattered read less
#pragma unroll
        for (int u = 0; u < S; ++u) fnr[u] = g.first[(size_t)(sk[u] + 1 == g.cap ? 0 : sk[u] + 1) * g.n + iu[u]];
    }
    int dn[S], stop[S];
#pragma unroll
    for (int u = 0; u < S; ++u) {
        dn[u] = dnr[u] != 0;
        stop[u] = lane < g.steps && (dn[u] | (lane + 1 == g.steps) | (sk[u] == g.end) | (fnr[u] != 0));
    }
    // one ballot a sample gives m; then the two rows of every sample: the last step's own and step 0's predecessor.  All row loads are
    // unconditional and stand in one block, so that none waits for a branch: a lane past the row's end reads its last value again, and
    // the predecessor is read (not stored) also where step 0 opened an episode
    int m[S], fst[S];
    OT vcur[S], vprev[S];
    const int ll = min(lane, LD - 1);
#pragma unroll
    for (int u = 0; u < S; ++u) {
        m[u] = u < ns ? __ffsll((unsigned long long)__ballot(stop[u])) : 0;   // lane n - 1 stops: never 0 for a sample
        fst[u] = __builtin_amdgcn_readlane(k.first, u);
        const int tl = (tu[u] + max(m[u] - 1, 0)) % g.cap, tp = tu[u] == 0 ? g.cap - 1 : tu[u] - 1;
        vcur[u] = o[ring_row(g.tiled, g.cap, g.n, tl, iu[u]) * LD + ll];
        vprev[u] = o[ring_row(g.tiled, g.cap, g.n, tp, iu[u]) * LD + ll];
    }
    // the two recurrences, while the rows are on their way: every lane runs them on the same values (the rewards come by readlane), and
    // lane u keeps the scalars of sample u
    float ret = 0.0f, disc = 0.0f;
    int dlast = 0, taken = 0;
#pragma unroll
    for (int u = 0; u < S; ++u) {
        double sum = 0.0, d = 1.0;
        {
#pragma clang fp contract(off)                                      // no fma: product and sum each rounded, in the header's order
            for (int j = m[u] - 1; j >= 0; --j) {
                const double r = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(rw[u]), j));
                const double tt = g.gamma * sum;
                sum = r + tt;
            }
            for (int j = 0; j < m[u]; ++j) d = d * g.gamma;
        }
        const int dl = __builtin_amdgcn_readlane(dn[u], max(m[u] - 1, 0));
        if (lane == u) { ret = (float)sum; disc = dl ? 0.0f : (float)d; dlast = dl; taken = m[u]; }
    }
#pragma unroll
    for (int u = 0; u < S; ++u) {
        if (u < ns && lane < LD) {
            const size_t b = (size_t)(b0 + u);
            g.s_next[b * LD + lane] = (float)vcur[u];
            g.s[b * LD + lane] = s_value<KIND>(fst[u], lane, g.frame_val, vprev[u]);
        }
    }
    if (lane < ns) {
        g.action_out[b0 + lane] = (int64_t)k.act;
        g.reward_out[b0 + lane] = ret;
        g.discount_out[b0 + lane] = disc;
        g.done_out[b0 + lane] = (uint8_t)dlast;
        g.steps_out[b0 + lane] = taken;
    }
    expand_plans<KIND>(g, k.p, b0, ns, lane);
}

template <int KIND, typename OT>
__global__ __launch_bounds__(256) void k_gather_windows(const RArgs g) {
    constexpr int RU = 4;                                            // rows per sample and round
    const int lane = threadIdx.x & 63;
    const int b0 = ((int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * S;   // in scalar registers: the group's control flow is uniform
    if (b0 >= g.batch) return;
    const int ns = min(S, g.batch - b0);
    const int LD = g.ld, L = g.steps;
    const OT* o = (const OT*)g.obs;
    const Pick k = pick<false, false>(g, nullptr, b0, ns, lane);     // of (t, i) the plan row alone: flags and actions come along the walk
    // lane j < L: the step j before the window's end -- the window's earliest step when its length is j + 1.  The loads of the whole group
    // stand in one block, before anything reads them (a sample past the batch's end walks from (0, 0): valid addresses, results unused)
    int tu[S], iu[S], es[S], act[S], dnr[S], fr[S], dpr[S];
    float rw[S];
#pragma unroll
    for (int u = 0; u < S; ++u) {
        tu[u] = __builtin_amdgcn_readlane(k.t, u); iu[u] = __builtin_amdgcn_readlane(k.i, u);
        es[u] = ((tu[u] - lane) % g.cap + g.cap) % g.cap;
        act[u] = 0; dnr[u] = 0; fr[u] = 0; dpr[u] = 0; rw[u] = 0.0f;
    }
    if (lane < L) {
#pragma unroll
        for (int u = 0; u < S; ++u) {
            const size_t at = (size_t)es[u] * g.n + iu[u];
            fr[u] = g.first[at];
            dnr[u] = g.done[at];
            act[u] = g.action[at];
            rw[u] = g.reward[at];
            dpr[u] = g.done[(size_t)(es[u] == 0 ? g.cap - 1 : es[u] - 1) * g.n + iu[u]];
        }
    }
    int dn[S], f[S], stop[S];
#pragma unroll
    for (int u = 0; u < S; ++u) {
        dn[u] = dnr[u] != 0; f[u] = fr[u] != 0;
        stop[u] = lane < L && ((lane + 1 == L) | (es[u] == g.end) | f[u] | (dpr[u] != 0));
    }
    // one ballot a sample: its length.  Its len + 1 distinct rows are the rows of steps t - len .. t: row r is s of position r and s_next
    // of position r - 1; row 0 is the reset observation instead when the earliest step opened an episode
    int len[S], fst[S], start[S];
    int longest = 0;
#pragma unroll
    for (int u = 0; u < S; ++u) {
        len[u] = u < ns ? __ffsll((unsigned long long)__ballot(stop[u])) : 0;   // lane L - 1 stops: never 0 for a sample
        fst[u] = __builtin_amdgcn_readlane(f[u], max(len[u] - 1, 0));
        start[u] = ((tu[u] - len[u]) % g.cap + g.cap) % g.cap;
        longest = max(longest, len[u]);
    }
    // RU rows of each sample a round: S * RU row loads in flight before the round's first store
    for (int r0 = 0; r0 <= longest; r0 += RU) {
        // every load of the round unconditional, in one block: a row past the window's last is its last again and a lane past the row's end
        // its last value again (the same lines; nothing of them is stored), so that no load waits for a branch
        OT v[S][RU];
        const int ll = min(lane, LD - 1);
#pragma unroll
        for (int u = 0; u < S; ++u) {
#pragma unroll
            for (int x = 0; x < RU; ++x)
                v[u][x] = o[ring_row(g.tiled, g.cap, g.n, (start[u] + min(r0 + x, len[u])) % g.cap, iu[u]) * LD + ll];
        }
#pragma unroll
        for (int u = 0; u < S; ++u) {
#pragma unroll
            for (int x = 0; x < RU; ++x) {
                const int r = r0 + x;
                if (u < ns && r <= len[u] && lane < LD) {
                    const size_t b = (size_t)(b0 + u) * L;
                    const float val = s_value<KIND>(r == 0 && fst[u], lane, g.frame_val, v[u][x]);
                    if (r < len[u]) g.s[(b + r) * LD + lane] = val;
                    if (r >= 1) g.s_next[(b + r - 1) * LD + lane] = val;
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < S; ++u) {
        if (u >= ns) break;
        const size_t b = (size_t)(b0 + u) * L;
        // positions >= len: zero rows, as one run
        const size_t z0 = (b + len[u]) * LD;
        const int zn = (L - len[u]) * LD;
        for (int x = lane; x < zn; x += 64) { g.s[z0 + x] = 0.0f; g.s_next[z0 + x] = 0.0f; }
        if (lane < L) {                                              // lane j < len holds position len - 1 - j; lane j >= len zeroes position j
            const bool in = lane < len[u];
            const size_t at = b + (in ? len[u] - 1 - lane : lane);
            g.action_out[at] = in ? (int64_t)act[u] : 0;
            g.reward_out[at] = in ? rw[u] : 0.0f;
            g.done_out[at] = in ? (uint8_t)dn[u] : (uint8_t)0;
            g.mask_out[b + lane] = in ? 1 : 0;
        }
        if (lane == 0) g.steps_out[b0 + u] = len[u];
        if (g.plan_out) expand_plan<KIND>(g, k.p, b0, u, lane);      // the plan inside the per-sample loop, not as a tail
    }
}

// ------------------------------------------------------------------------------------------------
// snac_replay_gather_onpolicy (include/snac_hip.h, "On-policy rollouts"): the sample's s, its plan and five scalars of the [cap][N] rings.
struct PArgs : GHead {
    const int8_t* action;
    const float* value;
    const float* logp;
    const float* adv;
    const float* ret;
    const float* norm;                                               // {mean, rstd} or NULL
    int64_t* action_out;
    float* value_out;
    float* logp_out;
    float* adv_out;
    float* ret_out;
};

// k_gather's shape without the s_next row: the samples' indices, then their flags and scalars (lane u = sample u), then the predecessor
// row of every sample of the group, each round issued whole before anything waits on it; then the stores
template <int KIND, typename OT>
__global__ __launch_bounds__(256) void k_gather_onpolicy(const PArgs g) {
    const int lane = threadIdx.x & 63;
    const int b0 = ((int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * S;   // in scalar registers: the group's control flow is uniform
    if (b0 >= g.batch) return;
    const int ns = min(S, g.batch - b0);
    const int LD = g.ld;
    const OT* o = (const OT*)g.obs;
    const Pick k = pick<true, true>(g, g.action, b0, ns, lane);
    float val = 0.0f, lp = 0.0f, ad = 0.0f, rt = 0.0f, mean = 0.0f, rstd = 1.0f;
    if (lane < ns) {
        val = g.value[k.cur]; lp = g.logp[k.cur]; ad = g.adv[k.cur]; rt = g.ret[k.cur];
        if (g.norm) { mean = g.norm[0]; rstd = g.norm[1]; }
    }
    // the row loads unconditional, in one block: a lane past the row's end reads its last value again, a sample past the batch's end the
    // predecessor of (0, 0) (valid addresses, results unused), and the predecessor is read (not stored) also where the step opened an episode
    OT vprev[S];
    int fst[S];
    const int ll = min(lane, LD - 1);
#pragma unroll
    for (int u = 0; u < S; ++u) {
        const int tu = __builtin_amdgcn_readlane(k.t, u), iu = __builtin_amdgcn_readlane(k.i, u);
        fst[u] = __builtin_amdgcn_readlane(k.first, u);
        vprev[u] = o[ring_row(g.tiled, g.cap, g.n, tu == 0 ? g.cap - 1 : tu - 1, iu) * LD + ll];
    }
#pragma unroll
    for (int u = 0; u < S; ++u) {
        if (u < ns && lane < LD) g.s[(size_t)(b0 + u) * LD + lane] = s_value<KIND>(fst[u], lane, g.frame_val, vprev[u]);
    }
    if (lane < ns) {
        float an = ad;
        if (g.norm) {
#pragma clang fp contract(off)                                      // no fma: difference and product each rounded
            const float df = ad - mean;
            an = df * rstd;
        }
        g.action_out[b0 + lane] = (int64_t)k.act;
        g.value_out[b0 + lane] = val;
        g.logp_out[b0 + lane] = lp;
        g.adv_out[b0 + lane] = an;
        g.ret_out[b0 + lane] = rt;
    }
    expand_plans<KIND>(g, k.p, b0, ns, lane);
}

// ------------------------------------------------------------------------------------------------
// host side.  The checks every entry point shares, every one before any HIP call, in two halves: an entry point's own tests (the walks'
// steps and end, its null pointers) stand between them, so that each bad argument meets the check it always met first
int check_ring(const snac_env_desc* d, const snac_state* st, int32_t cap, int32_t batch) {
    if (int rc = check_common(d, st)) return rc;
    if (cap < 2 || batch < 0) return fail(SNAC_ERR_ARG, "cap must be >= 2 and batch >= 0");
    return SNAC_OK;
}

int check_plan_tail(const snac_env_desc* d, const int16_t* plan_idx_ring, const float* plan_out) {
    if (plan_out && !plan_idx_ring) return fail(SNAC_ERR_ARG, "plan_out needs plan_idx_ring");
    if (plan_out && d->kind != SNAC_ENV_1D && ((uintptr_t)plan_out & 15)) return fail(SNAC_ERR_ARG, "plan_out must be 16-byte aligned");
    if (d->obs_tail & ~SNAC_TAIL_POSITION) return fail(SNAC_ERR_UNSUPPORTED, "replay gather supports the position tail only");
    return SNAC_OK;
}

// the shared head of an argument struct, up to its two outputs
void fill_head(GHead& g, const snac_env_desc* d, const snac_state* st, int32_t cap, int32_t tiled, const void* obs_ring, const uint8_t* first_ring,
               const int16_t* plan_idx_ring, const int32_t* tick_idx, const int32_t* env_idx, int32_t batch) {
    g.n = d->num_envs; g.cap = cap; g.batch = batch; g.num_plans = d->num_plans;
    g.ld = base_obs_dim(d->kind) + tail_len(d->kind, d->obs_tail); g.frame_val = d->frame_value == 2 ? 2 : -1; g.tiled = tiled != 0;
    g.obs = obs_ring; g.first = first_ring; g.plan_idx = plan_idx_ring; g.tick = tick_idx; g.env = env_idx; g.plans = st->plans;
}

template <typename F>
void by_kind(const snac_env_desc* d, F f) {                          // the six (kind, row type) instantiations
    const bool f32 = d->obs_dtype == SNAC_OBS_F32;
    if (d->kind == SNAC_ENV_1D) { if (f32) f(std::integral_constant<int, 1>(), float()); else f(std::integral_constant<int, 1>(), double()); }
    else if (d->kind == SNAC_ENV_2D) { if (f32) f(std::integral_constant<int, 2>(), float()); else f(std::integral_constant<int, 2>(), double()); }
    else { if (f32) f(std::integral_constant<int, 3>(), float()); else f(std::integral_constant<int, 3>(), double()); }
}

dim3 groups(int32_t batch) { return dim3((unsigned)((batch + 4 * S - 1) / (4 * S))); }   // 4 waves x S samples a block (8 samples a wave were no faster)

// both layouts of the plain gather.  (snac_last_kernel() keeps naming the launch before, as it always has for this entry point)
int replay_gather(const snac_env_desc* d, const snac_state* st, int32_t cap, int32_t tiled, const void* obs_ring, const uint8_t* first_ring,
                  const int16_t* plan_idx_ring, const int32_t* tick_idx, const int32_t* env_idx, int32_t batch, float* s_out, float* s_next_out,
                  float* plan_out, void* stream) {
    if (int rc = check_ring(d, st, cap, batch)) return rc;
    if (!obs_ring || !first_ring || !tick_idx || !env_idx || !s_out || !s_next_out) return fail(SNAC_ERR_ARG, "null pointer");
    if (int rc = check_plan_tail(d, plan_idx_ring, plan_out)) return rc;
    if (batch == 0) return SNAC_OK;
    GArgs g{};
    fill_head(g, d, st, cap, tiled, obs_ring, first_ring, plan_idx_ring, tick_idx, env_idx, batch);
    g.s = s_out; g.s_next = s_next_out; g.plan_out = plan_out;
    // (round 4: a variant that takes whole groups of 16 samples with 16-byte stores -- lane = piece of the group's consecutive rows --
    // was built and measured: 0.0382 against 0.0352 ms per 65 536 samples for this kernel, which already runs at 5.3 TB/s = 0.66 of the
    // peak; what rounds 2 and 3 reported as "0.23-0.30" was the Python wrapper's own index kernels.  Not kept; tools/gather_time.py)
    by_kind(d, [&](auto kind, auto ot) {
        hipLaunchKernelGGL((k_gather<decltype(kind)::value, decltype(ot)>), groups(batch), dim3(256), 0, (hipStream_t)stream, g);
    });
    return launched("snac_replay_gather");
}

// the checks the two walks share; steps: n or L, end: newest or oldest
int walk_check(const snac_env_desc* d, const snac_state* st, int32_t cap, const void* obs_ring, const uint8_t* first_ring, const uint8_t* done_ring,
               const float* reward_ring, const int8_t* action_ring, const int16_t* plan_idx_ring, int32_t end, const char* end_msg,
               const int32_t* tick_idx, const int32_t* env_idx, int32_t batch, int32_t steps, const char* steps_msg, const float* plan_out) {
    if (int rc = check_ring(d, st, cap, batch)) return rc;
    if (steps < 1 || steps > 64) return fail(SNAC_ERR_ARG, steps_msg);
    if (end < 0 || end >= cap) return fail(SNAC_ERR_ARG, end_msg);
    if (!obs_ring || !first_ring || !done_ring || !reward_ring || !action_ring) return fail(SNAC_ERR_ARG, "null ring array");
    if (!tick_idx || !env_idx) return fail(SNAC_ERR_ARG, "null index array");
    return check_plan_tail(d, plan_idx_ring, plan_out);
}

RArgs walk_args(const snac_env_desc* d, const snac_state* st, int32_t cap, int32_t tiled, const void* obs_ring, const uint8_t* first_ring,
                const uint8_t* done_ring, const float* reward_ring, const int8_t* action_ring, const int16_t* plan_idx_ring, int32_t end,
                const int32_t* tick_idx, const int32_t* env_idx, int32_t batch, int32_t steps) {
    RArgs g{};
    fill_head(g, d, st, cap, tiled, obs_ring, first_ring, plan_idx_ring, tick_idx, env_idx, batch);
    g.end = end; g.steps = steps;
    g.done = done_ring; g.reward = reward_ring; g.action = action_ring;
    return g;
}

}  // namespace

extern "C" {

int snac_replay_gather(const snac_env_desc* d, const snac_state* st, int32_t cap, const void* obs_ring,
                       const uint8_t* first_ring, const int16_t* plan_idx_ring, const int32_t* tick_idx,
                       const int32_t* env_idx, int32_t batch, float* s_out, float* s_next_out, float* plan_out,
                       void* stream) {
    return replay_gather(d, st, cap, 0, obs_ring, first_ring, plan_idx_ring, tick_idx, env_idx, batch, s_out, s_next_out, plan_out, stream);
}

int snac_replay_gather_tiled(const snac_env_desc* d, const snac_state* st, int32_t cap, const void* obs_ring,
                             const uint8_t* first_ring, const int16_t* plan_idx_ring, const int32_t* tick_idx,
                             const int32_t* env_idx, int32_t batch, float* s_out, float* s_next_out, float* plan_out,
                             void* stream) {
    return replay_gather(d, st, cap, 1, obs_ring, first_ring, plan_idx_ring, tick_idx, env_idx, batch, s_out, s_next_out, plan_out, stream);
}

int snac_replay_gather_nstep(const snac_env_desc* d, const snac_state* st, int32_t cap, int32_t tiled, const void* obs_ring,
                             const uint8_t* first_ring, const uint8_t* done_ring, const float* reward_ring, const int8_t* action_ring,
                             const int16_t* plan_idx_ring, int32_t newest, const int32_t* tick_idx, const int32_t* env_idx, int32_t batch,
                             int32_t n, double gamma, float* s_out, float* s_next_out, float* plan_out, int64_t* action_out,
                             float* return_out, float* discount_out, uint8_t* done_out, int32_t* steps_out, void* stream) {
    if (int rc = walk_check(d, st, cap, obs_ring, first_ring, done_ring, reward_ring, action_ring, plan_idx_ring, newest,
                            "newest must be in [0, cap)", tick_idx, env_idx, batch, n, "n must be in [1, 64]", plan_out))
        return rc;
    if (!std::isfinite(gamma)) return fail(SNAC_ERR_ARG, "gamma must be finite");
    if (!s_out || !s_next_out || !action_out || !return_out || !discount_out || !done_out || !steps_out) return fail(SNAC_ERR_ARG, "null output");
    if (batch == 0) return SNAC_OK;                                  // no sample: no launch
    RArgs g = walk_args(d, st, cap, tiled, obs_ring, first_ring, done_ring, reward_ring, action_ring, plan_idx_ring, newest, tick_idx, env_idx, batch, n);
    g.gamma = gamma;
    g.s = s_out; g.s_next = s_next_out; g.plan_out = plan_out; g.action_out = action_out; g.reward_out = return_out;
    g.discount_out = discount_out; g.done_out = done_out; g.steps_out = steps_out;
    g_kernel = "k_gather_nstep";
    by_kind(d, [&](auto kind, auto ot) {
        hipLaunchKernelGGL((k_gather_nstep<decltype(kind)::value, decltype(ot)>), groups(batch), dim3(256), 0, (hipStream_t)stream, g);
    });
    return launched("snac_replay_gather_nstep");
}

int snac_replay_gather_windows(const snac_env_desc* d, const snac_state* st, int32_t cap, int32_t tiled, const void* obs_ring,
                               const uint8_t* first_ring, const uint8_t* done_ring, const float* reward_ring, const int8_t* action_ring,
                               const int16_t* plan_idx_ring, int32_t oldest, const int32_t* tick_idx, const int32_t* env_idx, int32_t batch,
                               int32_t L, float* s_out, float* s_next_out, float* plan_out, int64_t* action_out, float* reward_out,
                               uint8_t* done_out, uint8_t* mask_out, int32_t* length_out, void* stream) {
    if (int rc = walk_check(d, st, cap, obs_ring, first_ring, done_ring, reward_ring, action_ring, plan_idx_ring, oldest,
                            "oldest must be in [0, cap)", tick_idx, env_idx, batch, L, "L must be in [1, 64]", plan_out))
        return rc;
    if (!s_out || !s_next_out || !action_out || !reward_out || !done_out || !mask_out || !length_out) return fail(SNAC_ERR_ARG, "null output");
    if (batch == 0) return SNAC_OK;                                  // no window: no launch
    RArgs g = walk_args(d, st, cap, tiled, obs_ring, first_ring, done_ring, reward_ring, action_ring, plan_idx_ring, oldest, tick_idx, env_idx, batch, L);
    g.s = s_out; g.s_next = s_next_out; g.plan_out = plan_out; g.action_out = action_out; g.reward_out = reward_out;
    g.done_out = done_out; g.mask_out = mask_out; g.steps_out = length_out;
    g_kernel = "k_gather_windows";
    by_kind(d, [&](auto kind, auto ot) {
        hipLaunchKernelGGL((k_gather_windows<decltype(kind)::value, decltype(ot)>), groups(batch), dim3(256), 0, (hipStream_t)stream, g);
    });
    return launched("snac_replay_gather_windows");
}

int snac_replay_gather_onpolicy(const snac_env_desc* d, const snac_state* st, int32_t cap, int32_t tiled, const void* obs_ring,
                                const uint8_t* first_ring, const int16_t* plan_idx_ring, const int8_t* action_ring, const float* value_ring,
                                const float* logp_ring, const float* adv_ring, const float* ret_ring, const float* norm,
                                const int32_t* tick_idx, const int32_t* env_idx, int32_t batch, float* s_out, float* plan_out,
                                int64_t* action_out, float* value_out, float* logp_out, float* adv_out, float* ret_out, void* stream) {
    if (int rc = check_ring(d, st, cap, batch)) return rc;
    if (!obs_ring || !first_ring || !action_ring || !value_ring || !logp_ring || !adv_ring || !ret_ring) return fail(SNAC_ERR_ARG, "null ring array");
    if (!tick_idx || !env_idx) return fail(SNAC_ERR_ARG, "null index array");
    if (int rc = check_plan_tail(d, plan_idx_ring, plan_out)) return rc;
    if (!s_out || !action_out || !value_out || !logp_out || !adv_out || !ret_out) return fail(SNAC_ERR_ARG, "null output");
    if (batch == 0) return SNAC_OK;                                  // no sample: no launch
    PArgs g{};
    fill_head(g, d, st, cap, tiled, obs_ring, first_ring, plan_idx_ring, tick_idx, env_idx, batch);
    g.action = action_ring; g.value = value_ring; g.logp = logp_ring; g.adv = adv_ring; g.ret = ret_ring; g.norm = norm;
    g.s = s_out; g.plan_out = plan_out; g.action_out = action_out; g.value_out = value_out; g.logp_out = logp_out; g.adv_out = adv_out;
    g.ret_out = ret_out;
    g_kernel = "k_gather_onpolicy";
    by_kind(d, [&](auto kind, auto ot) {
        hipLaunchKernelGGL((k_gather_onpolicy<decltype(kind)::value, decltype(ot)>), groups(batch), dim3(256), 0, (hipStream_t)stream, g);
    });
    return launched("snac_replay_gather_onpolicy");
}

}  // extern "C"
