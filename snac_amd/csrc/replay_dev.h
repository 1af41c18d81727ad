// replay_dev.h -- what the replay gathers share (k_gather in k_misc.hip; k_gather_nstep, k_gather_windows and k_gather_onpolicy in k_replay.hip): where a
// ring row lies in either layout, the reset observation, and the expansion of a plan row into float32 cells.  include/snac_hip.h,
// "Minibatch assembly", has the semantics.
#pragma once
#include "snac_units.h"

namespace snac_detail {

// row (t, i) of the ring, in rows: obs[cap][n][ld], or tile-major obs[ceil(n / 64)][cap][64][ld]
__device__ __forceinline__ size_t ring_row(int tiled, int cap, int n, int t, int i) {
    return tiled ? ((size_t)(i >> 6) * cap + t) * 64 + (i & 63) : (size_t)t * n + i;
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

// plan row pu of the table as float32 cells at po (30 for 1D, else 400), by one wave
template <int KIND>
__device__ __forceinline__ void expand_plan(const void* plans, int pu, float* po, int lane) {
    constexpr int PC = KIND == 1 ? 30 : 400;
    if (KIND == 1) {
        if (lane < PC) po[lane] = (float)((const int16_t*)plans)[pu * 32 + lane];
    } else {
        // four consecutive cells per lane (a row of 20 holds five such groups): one 16-byte store each, 100 lanes a plan
        for (int q = lane; q < PC / 4; q += 64) {
            const int c = q * 4;
            float4 v;
            if (KIND == 2) {
                const int row = c / 20, col = c - row * 20;
                const uint32_t w = ((const uint32_t*)plans)[pu * 20 + row] >> col;
                v = make_float4((float)(w & 1u), (float)((w >> 1) & 1u), (float)((w >> 2) & 1u), (float)((w >> 3) & 1u));
            } else {
                const short4 h = *(const short4*)((const int16_t*)plans + (size_t)pu * 400 + c);
                v = make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
            }
            *(float4*)(po + c) = v;
        }
    }
}

}  // namespace snac_detail
