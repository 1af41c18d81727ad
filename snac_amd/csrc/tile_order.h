// tile_order.h -- which block of envs a workgroup of k_rollout2d takes (SNAC_2D_STAGE_XCD).  Plain host / device arithmetic without any
// HIP type, so that tests/native/tile_order_test.cpp checks it on the CPU.
//
// Workgroups are dealt round-robin over the 8 XCDs (blockIdx.x & 7 labels the workgroups that share one).  In launch order, XCD x
// therefore owns blocks x, x + 8, x + 16, ...: every 8th block of 256 envs.  The XCD-contiguous order gives it a contiguous eighth of
// the env range instead, as k_rollout3d does: the grid is padded to a multiple of 8, workgroup b takes block
// (b & 7) * (grid / 8) + (b >> 3), and a workgroup whose block lies past the last one leaves.  A bijection of [0, grid) onto itself.
// The knob: 0 launch order, 1 the XCD-contiguous order always, 2 (default) only where the number of blocks is a multiple of 8 already --
// padding puts whole blocks behind the first round of workgroups (launch_roll2d_w, profiles/pass_ends.txt).
#pragma once

#if defined(__HIPCC__)
#define SNAC_TILE_HD __host__ __device__
#else
#define SNAC_TILE_HD
#endif

namespace snac_detail {

// the grid for `blocks` blocks of envs: as many workgroups (launch order), or the next multiple of 8 (XCD-contiguous order)
SNAC_TILE_HD constexpr int tile_order_grid(int blocks, bool xcd) { return xcd ? (blocks + 7) & ~7 : blocks; }

// the block of envs that workgroup `wg` of a grid of `grid` workgroups takes; with xcd, grid is a multiple of 8
SNAC_TILE_HD constexpr int tile_order_block(int wg, int grid, bool xcd) { return xcd ? (wg & 7) * (grid >> 3) + (wg >> 3) : wg; }

}  // namespace snac_detail
