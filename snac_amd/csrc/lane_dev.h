// lane_dev.h -- the lane helpers of the units whose lane is an atom of a categorical distribution (k_dist.hip, k_qloss.hip's k_c51_loss):
// a wave-uniform lane read of a double, the DPP move inside rows of 16 lanes, and TREE of include/snac_hip.h ("Distributional targets"),
// the shuffle-down tree over the 64 lanes of a wave.  Device code only.
#pragma once
#include <cstdint>

namespace snac_detail {

// lane `lane` (wave-uniform) of v, in every lane
__device__ __forceinline__ double lane_read(double v, int lane) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// lane j's copy of lane j + S of v for S < 16, inside rows of 16 lanes (0.0 where j + S leaves the row): a DPP move, no trip through LDS
template <int S>
__device__ __forceinline__ double row_down(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, 0x100 + S, 0xf, 0xf, true);      // row_shl:S
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), 0x100 + S, 0xf, 0xf, true);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// TREE: x_j = x_j + x_{j+s} for s = 32, 16, 8, 4, 2, 1, and x_0 in every lane (x: lane j's term, 0.0 in the lanes past the row's end).
// At step s only lanes j < s are read later, and their source j + s lies in the same row of 16 for s <= 8; the other lanes hold sums
// nobody reads
__device__ __forceinline__ double tree_sum(double x) {
#pragma clang fp contract(off)
    x = x + __shfl_down(x, 32, 64);
    x = x + __shfl_down(x, 16, 64);
    x = x + row_down<8>(x);
    x = x + row_down<4>(x);
    x = x + row_down<2>(x);
    x = x + row_down<1>(x);
    return lane_read(x, 0);
}

}  // namespace snac_detail
