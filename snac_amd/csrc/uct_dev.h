// uct_dev.h -- what the UCT units share (k_uct.hip: selection, backup, re-rooting; k_uct_play.hip: self-play; k_uct_reanalyse.hip): the
// map of a statistics row (snac_uct_node) in pieces and words, the loads of a node's pieces, and the steps of the K-paths selections
// that do not depend on the rule.  The rules (UCB1, PUCT, the Gumbel forms) are not here: each stays in its kernel.  Internal.
//
// Every helper here was kept only where the gfx950 listing of each kernel that uses it is the parent's, instruction for instruction
// (tools/uct_isa_compare.sh OLD.o NEW.o '' all).  That is why some kernels still spell a step out that another takes from here:
// HISTORY.md has the list.
#pragma once
#include <cstddef>

#include "snac_units.h"

// ------------------------------------------------------------------------------------------------
// The row's map, in 16-byte pieces (include/snac_hip.h has the struct): line 0 is all that selection compares, line 1 the node's own.
//     0-1 child[8] | 2-3 child_visits[8] | 4-7 child_value[8] || 8 parent, action, terminal, visits | 9 value_sum, reward, zero[0]: the
//     expander's slot | 10-11 zero[1 + a]: the in-flight counts | 12-13 the priors | 14 net_value, zero | 15 zero
static_assert(sizeof(snac_uct_node) == 256, "snac_uct_node is two lines");
static_assert(offsetof(snac_uct_node, child_visits) == 32 && offsetof(snac_uct_node, child_value) == 64 && offsetof(snac_uct_node, parent) == 128 &&
                  offsetof(snac_uct_node, visits) == 140 && offsetof(snac_uct_node, value_sum) == 144 && offsetof(snac_uct_node, reward) == 152 &&
                  offsetof(snac_uct_node, zero) == 156,
              "the piece map below");

namespace {

constexpr int PIECES = 16;                                           // 16-byte pieces per row
constexpr int P_CHILD = 0, P_VISITS = 2, P_VALUE = 4, P_HDR = 8, P_OWN = 9, P_FLY = 10, P_PRIOR = 12, P_NETV = 14;
// the 4-byte words that are read or stored one at a time
constexpr int W_CHILD_VISITS = 4 * P_VISITS, W_CHILD_VALUE = 4 * P_VALUE;   // the mirrors of child a's N (+ a) and W (+ 2 a) in its parent
constexpr int W_PARENT = 4 * P_HDR, W_VISITS = W_PARENT + 3, W_VALUE_SUM = 4 * P_OWN;
constexpr int W_SLOT = W_VALUE_SUM + 3;                              // zero[0]: the slot that expanded a row not yet written whole
constexpr int W_FLY = 4 * P_FLY;                                     // zero[1 + a]: paths in flight through child a

static_assert(4 * W_VISITS == offsetof(snac_uct_node, visits) && 4 * W_SLOT == offsetof(snac_uct_node, zero) &&
                  4 * W_FLY == offsetof(snac_uct_node, zero) + 4,
              "the words above");
static_assert(4 * SNAC_UCT_PRIOR_WORD == 16 * P_PRIOR && offsetof(snac_uct_node, zero) + 9 * 4 == 16 * P_PRIOR, "the priors' pieces");
static_assert(4 * SNAC_UCT_NET_VALUE_WORD == 16 * P_NETV && offsetof(snac_uct_node, zero) + 17 * 4 == 16 * P_NETV, "net_value's piece");

__device__ __forceinline__ double f64(uint32_t lo, uint32_t hi) { return __hiloint2double((int)hi, (int)lo); }

__device__ __forceinline__ int clamp_row(int r, int base, int cap) { return min(max(r, base), base + cap - 1); }

// word j (a constant after unrolling) of a piece
__device__ __forceinline__ uint32_t word_of(const uint4& p, int j) { return j == 0 ? p.x : j == 1 ? p.y : j == 2 ? p.z : p.w; }

// ------------------------------------------------------------------------------------------------
// A node's pieces in registers, as the UCB1 selections read them: children, child visits, child values, the header and the node's own
// piece, and with FLY the in-flight counts.  load() issues every load, before the first use; a piece that is not named is not loaded.
template <int A, bool FLY>
struct NodePieces {
    static constexpr int CI = (A + 3) / 4, CW = (A + 1) / 2;         // pieces of child / child_visits / in-flight, of child_value
    uint4 pc[CI], pn[CI], pf[CI], pw[CW], hdr, own;

    __device__ __forceinline__ void load(const uint4* rec) {
#pragma unroll
        for (int q = 0; q < CI; ++q) {
            pc[q] = rec[P_CHILD + q];
            pn[q] = rec[P_VISITS + q];
            if constexpr (FLY) pf[q] = rec[P_FLY + q];
        }
#pragma unroll
        for (int q = 0; q < CW; ++q) pw[q] = rec[P_VALUE + q];
        hdr = rec[P_HDR];
        own = rec[P_OWN];
    }
};

// ------------------------------------------------------------------------------------------------
// The steps of the K-paths selections (k_uct_select_paths, k_uct_select_puct) that do not depend on the rule.
// Action a of the node whose words are `words`, untried, becomes the tree's next row: the child word, one path in flight through it,
// and slot s in the new row's W_SLOT until the backup writes the row whole.  The new row.
__device__ __forceinline__ int expand_path(int32_t* words, uint4* stats, int a, int base, int& used, int s) {
    const int row = base + used;
    used += 1;
    words[a] = row;
    words[W_FLY + a] = 1;
    reinterpret_cast<int32_t*>(stats + (size_t)row * PIECES)[W_SLOT] = s;
    return row;
}

// Row n was made by an earlier path of this launch and is not written whole yet: the slot that expanded it.
__device__ __forceinline__ int fresh_row_slot(const uint4* stats, int n) { return reinterpret_cast<const int32_t*>(stats + (size_t)n * PIECES)[W_SLOT]; }

}  // namespace
