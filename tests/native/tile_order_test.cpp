// tile_order_test.cpp -- snac_amd/csrc/tile_order.h on the CPU: which tile of 64 envs each wave of a k_rollout2d grid takes.
// For every tile count 1 .. 600, in both orders (launch order; XCD-contiguous with the grid padded to a multiple of 8): every tile
// below the count is produced exactly once by the waves of the grid, and every other wave's tile lies past the end (that wave leaves).
// Plain host code with its own main; tests/test_tile_order.py builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <vector>

#include "tile_order.h"

using snac_detail::tile_order_block;
using snac_detail::tile_order_grid;

static_assert(tile_order_grid(10, true) == 16 && tile_order_grid(10, false) == 10 && tile_order_grid(16, true) == 16, "padding");
static_assert(tile_order_block(9, 16, true) == 3 && tile_order_block(9, 16, false) == 9, "the map is constexpr");

int main() {
    constexpr int WPB = 4;                                           // waves (tiles) per workgroup of k_rollout2d
    long checked = 0;
    for (int xcd = 0; xcd < 2; ++xcd) {
        for (int tiles = 1; tiles <= 600; ++tiles) {
            const int blocks = (tiles + WPB - 1) / WPB, grid = tile_order_grid(blocks, xcd != 0);
            if (grid < blocks || (xcd && (grid & 7)) || grid >= blocks + 8) { std::printf("grid %d for %d blocks (xcd %d)\n", grid, blocks, xcd); return 1; }
            std::vector<int> seen((size_t)tiles, 0);
            int past = 0;
            for (int wg = 0; wg < grid; ++wg) {
                const int blk = tile_order_block(wg, grid, xcd != 0);
                if (blk < 0 || blk >= grid) { std::printf("workgroup %d of %d -> block %d (xcd %d)\n", wg, grid, blk, xcd); return 1; }
                if (xcd && (blk / (grid >> 3)) != (wg & 7)) { std::printf("workgroup %d: block %d is not in the eighth of its XCD label\n", wg, blk); return 1; }
                for (int wv = 0; wv < WPB; ++wv) {
                    const int tile = blk * WPB + wv;
                    if (tile < tiles) seen[(size_t)tile] += 1; else past += 1;
                    ++checked;
                }
            }
            for (int t = 0; t < tiles; ++t)
                if (seen[(size_t)t] != 1) { std::printf("tiles %d xcd %d: tile %d taken %d times\n", tiles, xcd, t, seen[(size_t)t]); return 1; }
            if (past != grid * WPB - tiles) { std::printf("tiles %d xcd %d: %d waves past the end, expected %d\n", tiles, xcd, past, grid * WPB - tiles); return 1; }
        }
    }
    std::printf("TILE ORDER OK %ld\n", checked);
    return 0;
}
