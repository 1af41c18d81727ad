// batch_sum.h -- the two stages of the batch statistics of include/snac_hip.h ("PPO loss", "Q-learning losses", "Search loss"), device
// side, for k_ppo.hip, k_qloss.hip and k_search.hip: eight float64 sums over a minibatch in a fixed order, without atomics on floats.  Stage 1 is wave_sum in
// the loss kernel, a wave per 64 consecutive samples, whose lane 0 writes the wave's row of partials; stage 2 is reduce_partials, the
// body of a kernel of one wave.  COUNTS: bit k set where column k is a count, which is not divided by B.
#pragma once
#include <cstdint>

namespace snac_detail {

constexpr int BATCH_STATS = 8;                                       // SNAC_PPO_STATS, SNAC_Q_STATS, SNAC_SEARCH_STATS

// the xor butterfly of the header: u_j = u_j + u_{j ^ off}, off = 32 .. 1; every lane holds the same sum afterwards, since a + b == b + a
// bit for bit
__device__ __forceinline__ double wave_sum(double u) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) u = u + __shfl_xor(u, off, 64);
    return u;
}

// One wave.  Lane j adds rows j, j + 64, ... of the partials in increasing order from 0.0, then the same butterfly, the divisions by B,
// and lane 0 writes stats and mean_loss (stats[0] as a float; may be NULL).
template <unsigned COUNTS>
__device__ __forceinline__ void reduce_partials(const double* partials, long long W, int32_t B, double* stats, float* mean_loss) {
#pragma clang fp contract(off)
    double s[BATCH_STATS];
#pragma unroll
    for (int k = 0; k < BATCH_STATS; ++k) s[k] = 0.0;
    for (long long w = threadIdx.x; w < W; w += 64) {
#pragma unroll
        for (int k = 0; k < BATCH_STATS; ++k) s[k] = s[k] + partials[w * BATCH_STATS + k];      // the eight columns together
    }
#pragma unroll
    for (int k = 0; k < BATCH_STATS; ++k) s[k] = wave_sum(s[k]);
    if (threadIdx.x != 0) return;
    const double n = (double)B;
#pragma unroll
    for (int k = 0; k < BATCH_STATS; ++k) {
        const double v = (COUNTS >> k & 1u) ? s[k] : s[k] / n;
        stats[k] = v;
        if (k == 0 && mean_loss) mean_loss[0] = (float)v;
    }
}

}  // namespace snac_detail
