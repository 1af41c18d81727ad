// k_onpolicy.hip -- snac_gae: generalised advantage estimation over a span of the ring's [cap][N] arrays (PPO's advantages and returns).
// include/snac_hip.h, "On-policy rollouts", has the rule.  The minibatch gather of the same section is k_gather_onpolicy in k_replay.hip.
#include <cmath>
#include <cstddef>

#include "snac_units.h"

// lane = env, as k_uct_returns: every load and store of a wave is one coalesced span of a slot's row.  k_uct_returns walks its slots with
// one dependent load trip per slot; here the reward / value / done loads of a chunk of K slots all go out before the first dependent
// multiply of that chunk, and the next chunk's go out before this chunk's chain runs.  The serial chain is then the float64 operations of
// a slot, not a memory round trip per slot.  At small N the grid does not fill the device: the chain's length sets the time there, not
// occupancy (a time-parallel scan would fill it, and would not reproduce the rule bit for bit).
namespace {

using namespace snac_detail;

constexpr int K = SNAC_GAE_CHUNK;                                    // slots per chunk

struct GaeArgs {
    int32_t n, cap, first, count;
    double gamma, c;                                                 // c = gamma * lambda, rounded once on the host
    const float* reward;
    const uint8_t* done;
    const float* value;
    const float* bootstrap;
    float* adv;
    float* ret;
};

struct Chunk {
    float r[K], v[K];
    int d[K];
};

// entry j of the chunk is the slot j before `slot`, across the wrap; `left` >= 1 slots of the span remain from `slot` on, and an entry past
// them reads the last of them again (a valid address, the same lines; the value is not used), so that no load waits for a branch
__device__ __forceinline__ void load_chunk(const GaeArgs& g, int slot, int left, int i, Chunk& q) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
        int s = slot - min(j, left - 1);
        s = s < 0 ? s + g.cap : s;
        const size_t at = (size_t)s * g.n + i;
        q.r[j] = g.reward[at];
        q.v[j] = g.value[at];
        q.d[j] = g.done[at];
    }
}

// the chain over the chunk's first min(K, left) entries, newest first; nv and a carry over from chunk to chunk
__device__ __forceinline__ void run_chunk(const GaeArgs& g, int slot, int left, int i, const Chunk& q, double& nv, double& a) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < left) {                                              // `left` is uniform: a scalar branch
            int s = slot - j;
            s = s < 0 ? s + g.cap : s;
            const size_t at = (size_t)s * g.n + i;
            const double r = (double)q.r[j], v = (double)q.v[j];
            const bool d = q.d[j] != 0;
            double out;
            {
#pragma clang fp contract(off)                                      // no fma: every product, sum and difference rounded, in the header's order
                const double gn = g.gamma * nv;
                const double tgt = r + (d ? 0.0 : gn);
                const double delta = tgt - v;
                const double ca = g.c * a;
                a = delta + (d ? 0.0 : ca);
                out = a + v;
            }
            g.adv[at] = (float)a;
            g.ret[at] = (float)out;
            nv = v;
        }
    }
}

__device__ __forceinline__ int chunk_before(const GaeArgs& g, int slot) {   // the next chunk's newest slot (used only when more than K slots remain, so cap > K)
    const int s = slot - K;
    return s < 0 ? s + g.cap : s;
}

__global__ __launch_bounds__(64) void k_gae(const GaeArgs g) {
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= g.n) return;
    double nv = g.bootstrap ? (double)g.bootstrap[i] : 0.0, a = 0.0;
    int slot = (int)(((long long)g.first + g.count - 1) % g.cap);    // the newest slot
    int left = g.count;
    Chunk p, q;                                                      // two chunks in turn: one runs its chain while the other's loads are on their way
    load_chunk(g, slot, left, i, p);
    while (true) {
        int ns = chunk_before(g, slot);
        if (left > K) load_chunk(g, ns, left - K, i, q);
        run_chunk(g, slot, left, i, p, nv, a);
        left -= K; slot = ns;
        if (left <= 0) break;
        ns = chunk_before(g, slot);
        if (left > K) load_chunk(g, ns, left - K, i, p);
        run_chunk(g, slot, left, i, q, nv, a);
        left -= K; slot = ns;
        if (left <= 0) break;
    }
}

}  // namespace

extern "C" int snac_gae(int32_t N, int32_t cap, int32_t first, int32_t count, double gamma, double lambda, const float* reward,
                        const uint8_t* done, const float* value, const float* bootstrap, float* adv, float* ret, void* stream) {
    using namespace snac_detail;
    if (N < 1) return fail(SNAC_ERR_ARG, "N must be >= 1");
    if (cap < 1) return fail(SNAC_ERR_ARG, "cap must be >= 1");
    if (first < 0 || first >= cap) return fail(SNAC_ERR_ARG, "first must be in [0, cap)");
    if (count < 0 || count > cap) return fail(SNAC_ERR_ARG, "count must be in [0, cap]");
    if (!std::isfinite(gamma) || !std::isfinite(lambda)) return fail(SNAC_ERR_ARG, "gamma and lambda must be finite");
    if (!reward || !done || !value || !adv || !ret) return fail(SNAC_ERR_ARG, "null ring array (reward / done / value / adv / ret)");
    if (count == 0) return SNAC_OK;                                  // no slot to fill
    double c;
    {
#pragma clang fp contract(off)
        c = gamma * lambda;
    }
    const GaeArgs g{N, cap, first, count, gamma, c, reward, done, value, bootstrap, adv, ret};
    g_kernel = "k_gae";
    hipLaunchKernelGGL(k_gae, dim3((unsigned)(((long long)N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, g);
    return launched("snac_gae");
}
