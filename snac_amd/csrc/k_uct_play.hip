// k_uct_play.hip -- self-play on the UCT trees of k_uct.hip: snac_uct_pick_moves (a move per tree from the root's visit counts, with the
// visit distribution and the root value), snac_uct_restart (a new episode in some trees, the others untouched), snac_uct_returns
// (value targets from a ring of rewards) and snac_uct_gumbel_candidates (the candidate sets and the move of the Gumbel root search);
// snac_explore_pick_moves_temp, the move drawn from the counts' power 1 / T, is k_uct_pick with a temperature.
// include/snac_hip.h, "Self-play", "Gumbel root" and "Exploration noise", has the semantics.
#include <cmath>
#include <cstddef>

#include "snac_units.h"
#include "explore_rule.h"
#include "uct_dev.h"

// Three small, latency-bound kernels beside k_uct_advance.  pick and returns are lane = tree: a root is one 128-byte line (two when the
// value is asked for) and a ring slot is one coalesced span over b.  restart is wave = tree: the record (8 or 56 pieces of 16 bytes) and
// the statistics row (16 pieces) of a restarted tree leave as one piece per lane.
namespace {

constexpr uint32_t PICK_STREAM = 3;                                  // the counter RNG's stream of the sampled moves

struct UctPick {
    const uint4* stats;
    int32_t B, cap;
    uint32_t key, t;
    int64_t env_id_base;
    const uint8_t* greedy;
    int8_t* action;
    float* pi;
    float* value;
};

struct UctPickTemp : UctPick {                                       // snac_explore_pick_moves_temp: T per tree, or one T
    const float* temperature;
    double temp;
};

// the move's rules are explore_rule.h's: the greedy one and the integer draw for both entry points, the weights of a T for the second
template <int A, bool TEMP>
__global__ __launch_bounds__(64) void k_uct_pick(const std::conditional_t<TEMP, UctPickTemp, UctPick> v) {
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= v.B) return;
    const uint4* const rec = v.stats + (size_t)b * v.cap * PIECES;
    const uint4 n0 = rec[P_VISITS], n1 = rec[P_VISITS + 1];
    uint4 hdr = make_uint4(0u, 0u, 0u, 0u), own = hdr;
    if (v.value) { hdr = rec[P_HDR]; own = rec[P_OWN]; }             // line 1 only when the value is asked for
    const uint32_t raw[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
    uint32_t n[A];
    uint64_t total = 0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        n[a] = (uint32_t)max((int)raw[a], 0);                        // a count is never negative in a tree the search built
        total += n[a];
    }
    if (v.pi) {
#pragma unroll
        for (int a = 0; a < A; ++a) v.pi[(size_t)b * A + a] = total ? (float)((double)n[a] / (double)total) : 0.f;
    }
    if (v.value) {
        const int visits = (int)hdr.w;
        v.value[b] = visits ? (float)(__hiloint2double((int)own.y, (int)own.x) / (double)visits) : 0.f;
    }
    if (!v.action) return;
    int act = 0;
    if (total != 0) {
        const bool greedy = !v.greedy || v.greedy[b] != 0;
        uint32_t w = 0;
        if (!greedy) w = rng_word(env_keys(v.key, (uint64_t)(v.env_id_base + b)), v.t);
        if constexpr (TEMP) {
            const double T = v.temperature ? (double)v.temperature[b] : v.temp;
            act = snac_spec::temp_move<A>(n, total, greedy, T, w);
        } else {
            act = greedy ? snac_spec::pick_greedy<A>(n) : snac_spec::pick_weighted<A>(n, total, w);      // no floating point enters the choice
        }
    }
    v.action[b] = (int8_t)act;
}

struct UctRestart {
    uint4* stats;
    uint4* records;
    int32_t B, cap;
    const uint8_t* mask;
    const uint8_t* terminal;
    int32_t* used;
};

constexpr int RESTART_WAVES = 4;                                     // trees per workgroup

template <int RP>                                                    // 16-byte pieces of a node record (8: 1D / 2D, 56: 3D)
__global__ __launch_bounds__(64 * RESTART_WAVES) void k_uct_restart(const UctRestart v) {
    static_assert(RP <= 64, "a record is at most one piece per lane");
    const int lane = (int)threadIdx.x & 63;
    const int b = (int)blockIdx.x * RESTART_WAVES + ((int)threadIdx.x >> 6);
    if (b >= v.B) return;
    if (v.mask[b] == 0) return;                                      // the tree keeps every byte
    const size_t root = (size_t)b * v.cap, scratch = (size_t)v.B * v.cap + b;
    const bool term = v.terminal && v.terminal[b] != 0;
    if (lane < RP) v.records[root * RP + lane] = v.records[scratch * RP + lane];
    if (lane < PIECES) {
        const uint4 none = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu), zero = make_uint4(0u, 0u, 0u, 0u);
        v.stats[root * PIECES + lane] =
            lane < P_VISITS ? none : lane == P_HDR ? make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, term ? 1u : 0u, 0u) : zero;
    }
    if (lane == 0) v.used[b] = 1;
}

struct UctReturns {
    int32_t B, cap_moves, first, count;
    double gamma;
    const float* reward;
    const uint8_t* done;
    const float* bootstrap;
    float* z;
};

__global__ __launch_bounds__(64) void k_uct_returns(const UctReturns v) {
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= v.B) return;
    double g = v.bootstrap ? (double)v.bootstrap[b] : 0.0;
    int slot = (int)(((long long)v.first + v.count - 1) % v.cap_moves);
    for (int i = 0; i < v.count; ++i) {                              // the newest slot back to the oldest
        const size_t at = (size_t)slot * v.B + b;
        const double r = (double)v.reward[at];
        const bool d = v.done[at] != 0;
        {
#pragma clang fp contract(off)                                      // no fma: product and sum each rounded, as a host restatement computes them
            const double t = v.gamma * g;
            g = r + (d ? 0.0 : t);
        }
        v.z[at] = (float)g;
        slot = slot == 0 ? v.cap_moves - 1 : slot - 1;
    }
}

// ---- Gumbel root: candidate sets and the final move --------------------------------------------------------------------------------------
// lane = tree, as k_uct_pick: the root's line 0 (children, child visits, child values), its header's terminal word, the tree's A scores
// and its bounds pair are all issued before the first is used; the choice is A rounds of "the largest remaining by strict >, scanning a
// upward" over at most 8 ranks held in registers.
constexpr int GUMBEL_BEGIN = 0, GUMBEL_HALVE = 1, GUMBEL_PICK = 2;

struct UctGumbel {
    const uint4* stats;
    int32_t B, cap, mode, m;
    const float* scores;
    double c_visit, c_scale, fpv;
    const double* bounds;
    int32_t* cand;
    int8_t* action;
};

// the `keep` members of `from` (a mask over a < A) with the largest rank: one at a time, the largest remaining by strict >, a upward
template <int A>
__device__ __forceinline__ int top_ranks(const double (&rank)[A], int from, int keep) {
    int out = 0;
#pragma unroll
    for (int i = 0; i < A; ++i) {
        if (i >= keep) break;
        int best = -1;
        double br = 0.0;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const bool open = (from >> a & 1) != 0 && (out >> a & 1) == 0;
            if (open && (best < 0 || rank[a] > br)) { best = a; br = rank[a]; }
        }
        if (best >= 0) out |= 1 << best;
    }
    return out;
}

template <int A>
__global__ __launch_bounds__(64) void k_uct_gumbel(const UctGumbel v) {
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= v.B) return;
    const uint4* const rec = v.stats + (size_t)b * v.cap * PIECES;
    const bool begin = v.mode == GUMBEL_BEGIN;
    const uint4 hdr = rec[P_HDR];
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    uint4 c0 = zero4, c1 = zero4, n0 = zero4, n1 = zero4, w[4] = {zero4, zero4, zero4, zero4};
    double2 pair = make_double2(0.0, 0.0);
    int from = (1 << A) - 1;
    if (!begin) {                                                    // BEGIN reads no statistics but the root's terminal word
        c0 = rec[P_CHILD]; c1 = rec[P_CHILD + 1];
        n0 = rec[P_VISITS]; n1 = rec[P_VISITS + 1];
#pragma unroll
        for (int q = 0; q < (A + 1) / 2; ++q) w[q] = rec[P_VALUE + q];
        pair = reinterpret_cast<const double2*>(v.bounds)[b];
        from &= v.cand[b];
    }
    float score[A];
#pragma unroll
    for (int a = 0; a < A; ++a) score[a] = v.scores[(size_t)b * A + a];
    const uint32_t ch[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w}, nn[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
    int maxn = 0;
#pragma unroll
    for (int a = 0; a < A; ++a)
        if ((int)ch[a] >= 0) maxn = max(maxn, max((int)nn[a], 0));
    double rank[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
#pragma clang fp contract(off)                                      // no fma: the rank rounded step by step, as a host restatement computes it
        double x = (double)score[a];
        if (!begin) {
            const uint4 w2 = w[a / 2];
            const double wa = (a % 2 == 0) ? __hiloint2double((int)w2.y, (int)w2.x) : __hiloint2double((int)w2.w, (int)w2.z);
            const bool visited = (int)ch[a] >= 0 && (int)nn[a] > 0;
            double q = visited ? wa / (double)(int)nn[a] : v.fpv;
            if (visited && pair.y > pair.x) {
                const double d = q - pair.x, span = pair.y - pair.x;
                q = d / span;
            }
            const double s1 = v.c_visit + (double)maxn;
            const double s2 = s1 * v.c_scale;
            const double sig = s2 * q;
            x = x + sig;
        }
        rank[a] = x != x ? -INFINITY : x;
    }
    if (begin) {
        v.cand[b] = hdr.z != 0u ? 0 : top_ranks<A>(rank, from, min(v.m, A));
    } else if (v.mode == GUMBEL_HALVE) {
        v.cand[b] = top_ranks<A>(rank, from, (__popc((unsigned)from) + 1) / 2);
    } else {
        int act = 0;
        if (from != 0) {
            const int one = top_ranks<A>(rank, from, 1);
            act = __ffs(one) - 1;
        } else {                                                     // no candidates: the lowest a with the most child visits
            int best = max((int)nn[0], 0);
#pragma unroll
            for (int a = 1; a < A; ++a)
                if (max((int)nn[a], 0) > best) { best = max((int)nn[a], 0); act = a; }
        }
        v.action[b] = (int8_t)act;
    }
}

}  // namespace

namespace snac_detail {
// declared in snac_units.h: k_uct_reanalyse.hip runs the same checks
int play_check(int A, const void* stats, int32_t rows, int32_t B, int32_t cap) {
    if (A != 3 && A != 5 && A != 8) return fail(SNAC_ERR_ARG, "num_actions must be 3, 5 or 8");
    if (!stats) return fail(SNAC_ERR_ARG, "null stats");
    if (B < 1) return fail(SNAC_ERR_ARG, "B must be >= 1");
    if (cap < 1) return fail(SNAC_ERR_ARG, "cap must be >= 1");
    const long long need = (long long)B * ((long long)cap + 1);
    if (need > 0x7FFFFFFFll) return fail(SNAC_ERR_ARG, "B * (cap + 1) rows exceed int32");
    if (need > rows) return fail(SNAC_ERR_ARG, "B * (cap + 1) rows exceed stats_rows");
    if (((uintptr_t)stats & 127) != 0) return fail(SNAC_ERR_ARG, "stats must be 128-byte aligned (records of whole lines)");
    return SNAC_OK;
}
}  // namespace snac_detail

extern "C" {

int snac_uct_pick_moves(const snac_env_desc* desc, int32_t num_actions, const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap,
                        const uint8_t* greedy, uint32_t t, int8_t* action, float* pi, float* value, void* stream) {
    using namespace snac_detail;
    if (!desc) return fail(SNAC_ERR_ARG, "null desc");
    if (int rc = play_check(num_actions, stats, stats_rows, B, cap)) return rc;
    if (!action && !pi && !value) return SNAC_OK;                    // nothing asked for
    const UctPick v{(const uint4*)stats, B, cap, stream_key(desc->seed, PICK_STREAM), t, desc->env_id_base, greedy, action, pi, value};
    g_kernel = "k_uct_pick";
    if (num_actions == 3) hipLaunchKernelGGL((k_uct_pick<3, false>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, v);
    else if (num_actions == 5) hipLaunchKernelGGL((k_uct_pick<5, false>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, v);
    else hipLaunchKernelGGL((k_uct_pick<8, false>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, v);
    return launched("snac_uct_pick_moves");
}

int snac_explore_pick_moves_temp(const snac_env_desc* desc, int32_t num_actions, const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap,
                                 const uint8_t* greedy, uint32_t t, const float* temperature, double temp, int8_t* action, float* pi, float* value,
                                 void* stream) {
    using namespace snac_detail;
    if (!desc) return fail(SNAC_ERR_ARG, "null desc");
    if (int rc = play_check(num_actions, stats, stats_rows, B, cap)) return rc;
    if (!(temp >= 0.0)) return fail(SNAC_ERR_ARG, "temp must be >= 0 (finite or +inf; 0: greedy)");
    if (!action && !pi && !value) return SNAC_OK;                    // nothing asked for
    UctPickTemp v;
    static_cast<UctPick&>(v) = UctPick{(const uint4*)stats, B, cap, stream_key(desc->seed, PICK_STREAM), t, desc->env_id_base, greedy, action, pi, value};
    v.temperature = temperature;
    v.temp = temp;
    g_kernel = "k_uct_pick_temp";
    const dim3 grid((unsigned)((B + 63) / 64));
    if (num_actions == 3) hipLaunchKernelGGL((k_uct_pick<3, true>), grid, dim3(64), 0, (hipStream_t)stream, v);
    else if (num_actions == 5) hipLaunchKernelGGL((k_uct_pick<5, true>), grid, dim3(64), 0, (hipStream_t)stream, v);
    else hipLaunchKernelGGL((k_uct_pick<8, true>), grid, dim3(64), 0, (hipStream_t)stream, v);
    return launched("snac_explore_pick_moves_temp");
}

int snac_uct_restart(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, void* records, int32_t record_bytes,
                     int32_t record_rows, const uint8_t* mask, const uint8_t* terminal, int32_t* used, void* stream) {
    using namespace snac_detail;
    if (int rc = play_check(num_actions, stats, stats_rows, B, cap)) return rc;
    if (!records) return fail(SNAC_ERR_ARG, "null records");
    if (((uintptr_t)records & 127) != 0) return fail(SNAC_ERR_ARG, "records must be 128-byte aligned");
    if (record_bytes != 128 && record_bytes != 896) return fail(SNAC_ERR_ARG, "record_bytes must be 128 or 896");
    if ((long long)B * ((long long)cap + 1) > record_rows) return fail(SNAC_ERR_ARG, "B * (cap + 1) rows exceed record_rows");
    if (!mask) return fail(SNAC_ERR_ARG, "null mask");
    if (!used) return fail(SNAC_ERR_ARG, "null used");
    const UctRestart v{(uint4*)stats, (uint4*)records, B, cap, mask, terminal, used};
    const dim3 grid((unsigned)((B + RESTART_WAVES - 1) / RESTART_WAVES)), block(64 * RESTART_WAVES);
    g_kernel = "k_uct_restart";
    if (record_bytes == 128) hipLaunchKernelGGL((k_uct_restart<8>), grid, block, 0, (hipStream_t)stream, v);
    else hipLaunchKernelGGL((k_uct_restart<56>), grid, block, 0, (hipStream_t)stream, v);
    return launched("snac_uct_restart");
}

int snac_uct_returns(int32_t B, int32_t cap_moves, int32_t first, int32_t count, double gamma, const float* reward, const uint8_t* done,
                     const float* bootstrap, float* z, void* stream) {
    using namespace snac_detail;
    if (B < 1) return fail(SNAC_ERR_ARG, "B must be >= 1");
    if (cap_moves < 1) return fail(SNAC_ERR_ARG, "cap_moves must be >= 1");
    if ((long long)B * (long long)cap_moves > 0x7FFFFFFFll) return fail(SNAC_ERR_ARG, "B * cap_moves entries exceed int32");
    if (first < 0 || first >= cap_moves) return fail(SNAC_ERR_ARG, "first must be in [0, cap_moves)");
    if (count < 0 || count > cap_moves) return fail(SNAC_ERR_ARG, "count must be in [0, cap_moves]");
    if (!std::isfinite(gamma)) return fail(SNAC_ERR_ARG, "gamma must be finite");
    if (!reward || !done || !z) return fail(SNAC_ERR_ARG, "null ring array (reward / done / z)");
    if (count == 0) return SNAC_OK;                                  // no slot to fill
    const UctReturns v{B, cap_moves, first, count, gamma, reward, done, bootstrap, z};
    g_kernel = "k_uct_returns";
    hipLaunchKernelGGL(k_uct_returns, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, v);
    return launched("snac_uct_returns");
}

int snac_uct_gumbel_candidates(int32_t num_actions, const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t mode, int32_t m,
                               const float* scores, double c_visit, double c_scale, double first_play_value, const double* bounds, int32_t* cand,
                               int8_t* action, void* stream) {
    using namespace snac_detail;
    if (int rc = play_check(num_actions, stats, stats_rows, B, cap)) return rc;
    if (mode < GUMBEL_BEGIN || mode > GUMBEL_PICK) return fail(SNAC_ERR_ARG, "mode must be 0 (begin), 1 (halve) or 2 (pick)");
    if (mode == GUMBEL_BEGIN && m < 1) return fail(SNAC_ERR_ARG, "m must be >= 1");
    if (!scores) return fail(SNAC_ERR_ARG, "null scores");
    if (!std::isfinite(c_visit) || !std::isfinite(c_scale)) return fail(SNAC_ERR_ARG, "c_visit and c_scale must be finite");
    if (!std::isfinite(first_play_value)) return fail(SNAC_ERR_ARG, "first_play_value must be finite");
    if (mode != GUMBEL_BEGIN) {
        if (!bounds) return fail(SNAC_ERR_ARG, "null bounds");
        if (((uintptr_t)bounds & 15) != 0) return fail(SNAC_ERR_ARG, "bounds must be 16-byte aligned (a tree's pair is one piece)");
    }
    if (!cand) return fail(SNAC_ERR_ARG, "null cand");
    if (mode == GUMBEL_PICK && !action) return fail(SNAC_ERR_ARG, "null action");
    const UctGumbel v{(const uint4*)stats, B, cap, mode, m, scores, c_visit, c_scale, first_play_value, bounds, cand, action};
    const dim3 grid((unsigned)((B + 63) / 64));
    g_kernel = "k_uct_gumbel";
    if (num_actions == 3) hipLaunchKernelGGL((k_uct_gumbel<3>), grid, dim3(64), 0, (hipStream_t)stream, v);
    else if (num_actions == 5) hipLaunchKernelGGL((k_uct_gumbel<5>), grid, dim3(64), 0, (hipStream_t)stream, v);
    else hipLaunchKernelGGL((k_uct_gumbel<8>), grid, dim3(64), 0, (hipStream_t)stream, v);
    return launched("snac_uct_gumbel_candidates");
}

}  // extern "C"
