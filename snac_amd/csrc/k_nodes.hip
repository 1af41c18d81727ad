// k_nodes.hip -- tree-search node pools with ONE record per node: snac_nodes{1,2,3}d_pack / _unpack, snac_transition_nodes{1,2,3}d
#include "nodes_dev.h"
#include "rows1d.h"

// A tree edge (Env/1D/DMP_Env_1D_dynamic_MCTS.py:82-139, Env/2D/DMP_ENV_2D_dynamic_MCTS.py:117-175,
// Env/3D/DMP_simulator_3d_dynamic_triangle_MCTS.py:195-277: transition(state, action), one call per edge in
// script/MCTS/utils/mcts_Qvalue_dynamic.py:88,118) reads its parent at a RANDOM row, and the memory side of the L2 reads whole 128-byte
// lines (profiles/r06_rd_gran.txt: a lone 16-byte load costs the time of 128 bytes, whatever the stride from 128 B up).  In the batch
// layout of snac_state a parent lies in three arrays -- header 16 B, episode counter 4 B, grid -- so a 2D parent is 1 + 1 + 1.6 lines = 460
// bytes fetched for 100 (k_edges2d, round 5, runs at 0.55 of the peak by the algorithmic count because of it), a 1D parent three lines for
// 84 bytes and a 3D parent nine (800 bytes of heights at offset r * 800 span seven lines).  A node record (nodes_dev.h has the map) holds
// the three in whole 128-byte aligned lines -- one for 1D / 2D, seven for 3D -- so an edge reads its lines once and writes them once.
// Semantics are k_edges1d's / k_edges2d's / k_edges3d's on batch rows (rules1d / rules2d / rules3d + reward_check3d, snac_dev.h), the
// canonical layout, no auto-reset and no episodic sums.  1D / 3D pad words are written as zero whatever the source holds.

namespace snac_detail {

// the argument checks every node-pool entry point of the 1D / 3D records, snac_observe_nodes{1,2,3}d and snac_evaluate_nodes{1,2,3}d share
// (snac_dev.h; the 2D pack / unpack / transition have nodes2d_check below)
int nodes_check(int kind, const snac_env_desc* d, const snac_state* st, const void* nodes, int32_t pool_rows, int32_t m) {
    if (!d || !st || !nodes) return fail(SNAC_ERR_ARG, "null desc / state / nodes");
    if (d->kind != kind)
        return fail(SNAC_ERR_UNSUPPORTED, kind == SNAC_ENV_1D   ? "snac_node1d records are for the 1D kinds"
                                          : kind == SNAC_ENV_2D ? "snac_node2d records are for the 2D kinds (1D / 3D: snac_node1d / snac_node3d)"
                                                                : "snac_node3d records are for the 3D kinds");
    if (int rc = check_common(d, st)) return rc;
    if (pool_rows < 1) return fail(SNAC_ERR_ARG, "pool_rows must be >= 1");
    if (m < 0) return fail(SNAC_ERR_ARG, "m must be >= 0");
    if (((uintptr_t)nodes & 127) != 0) return fail(SNAC_ERR_ARG, "the node pool must be 128-byte aligned (records of whole lines)");
    if (make_args(d, st).variant) return fail(SNAC_ERR_UNSUPPORTED, "node pools write the canonical observation rows (layout variants: snac_transition)");
    return SNAC_OK;
}

}  // namespace snac_detail

namespace {

// the piece a 1D record leaves with: pad words zero (piece 1: the counter's three, piece 5: the two pad cells, the pad pieces)
__device__ __forceinline__ uint4 clean_piece1d(uint4 v, int part) {
    if (part == 1) v.y = v.z = v.w = 0u;
    if (part == 5) v.w = 0u;
    return part < 6 ? v : make_uint4(0u, 0u, 0u, 0u);
}

// 2D tree edges on node records.  A wave takes 64 edges; the records lie in LDS (LineRecs, nodes_dev.h) for the transition and the window
// and leave for their destination records the same way, header and episode counter included; the rows go out through emit_tile.  The step
// is K2D::step's on the agent's row word (DMP_Env_2D_dynamic_usedata_plan.py:85-147).  VEC = false: rows written value by value (a wave of
// m % 4 != 0 edges, an unaligned obs).
template <bool DYN, typename OT, int WPB, bool VEC, bool NT>
__global__ __launch_bounds__(WPB * 64) void k_edges2dp(const KArgs a) {
    using K = K2D<DYN, 64>;
    constexpr int E = 64, GE = K::GE;
    static_assert(E * LINE_WORDS * 4 <= TILE_STG_BYTES, "the records of a wave's edges fit its staging tile");
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[WPB * (TILE_STG_BYTES / 4)];
    const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
    const int edge0 = __builtin_amdgcn_readfirstlane(((int)blockIdx.x * WPB + wv) * E);
    if (edge0 >= a.n) return;
    const int nedge = min(E, a.n - edge0);
    const bool active = lane < nedge;
    const int edge = edge0 + (active ? lane : 0);
    LineRecs n(lds_all + wv * (TILE_STG_BYTES / 4), lane);
    uint4* const nodes = (uint4*)a.grid;                             // snac_node2d[pool]
    const int srow = (int)row_of(a.src_index, a.pool, edge), drow = (int)row_of(a.dst_index, a.pool, edge);
    // the action and step size first: their loads fly with the records' (after the gather they would wait behind its LDS stores)
    const uint64_t gid = (uint64_t)(a.env_id_base + edge);
    const uint32_t w = rng_word(env_keys(a.key_step, gid), a.t0);
    int act = draw_action<K::A>(w, a), k = 1 + (int)(((w & 0xffffu) * 3u) >> 16);
    if (a.use_scalar) { act = a.act_scalar; k = a.k_scalar; }
    if (a.actions) act = (int)a.actions[edge];
    if (a.step_size) k = (int)a.step_size[edge];
    k = min(max(k, 1), 3);
    n.gather<FETCH_ALL>(nodes, srow, nedge);
    Lane s = n.header();
    const uint32_t* const prow = (const uint32_t*)a.plans + (size_t)s.pidx * GE;
    const int q0 = min(max(s.r - 3, 0), GE - 1), bit = min(max(s.c - 3, 0), 19);
    const uint32_t pword = prow[q0];                                 // the one dependent load: the plan row under the agent (L2)
    // ---- the 2D step (rules2d, snac_dev.h) on the agent's row word
    const uint32_t row0 = n.word(REC_GRID + q0);
    const bool was = ((row0 >> bit) & 1u) != 0u, planned = ((pword >> bit) & 1u) != 0u;
    const Rule2D u = rules2d(s, act, k, was, planned, a.ts_done, a.brick_gt);   // the rules: snac_dev.h
    if (active && u.drop) n.word_at(REC_GRID + q0) = row0 | (1u << bit);
    const bool done = active && u.done;
    const int reward = u.reward;
    s.ep_ret = clamp16(s.ep_ret + reward);
    s.flags = done ? SNAC_FLAG_NEED_RESET : 0;
    if (active) {
        if (a.reward) a.reward[edge] = (float)reward;
        if (a.done) a.done[edge] = done ? 1 : 0;
        n.set_header(s);
    }
    // ---- the window round the new position -- read before the records leave (the staging tile takes their place).  (`bit` above is
    // clamped because the source header may be hand-made; the window's first column is not: this position comes out of rules2d)
    const Window2D cell(n, s.r, s.c - 3, GE);
    n.scatter(nodes, drow, nedge, [](uint4 v, int) { return v; });
    if (!a.obs) return;
    const Slots v = scalar_slots<DYN>(s, a.total_step);
    if constexpr (VEC) {
        asm volatile("" ::: "memory");                               // (every read of the records above, every write of the rows below)
        emit_tile<OT, NT>((char*)n.rec, (char*)a.obs + (size_t)edge0 * K::D * sizeof(OT), lane, nedge, cell, v.v0, v.v1);
    } else if (active) {
        write_row<K::W>((OT*)a.obs + (size_t)edge * K::D, cell, v);
    }
}

// 1D tree edges on node records: k_edges2dp's record movement (the two pad pieces are not read) with k_edges1d's step and the 5-cell
// window; the whole line leaves for the destination record.  VEC: the rows as one run per wave (Rows1D, m % 4 == 0 and an aligned obs;
// the staging run reuses the records' LDS once they have left); otherwise value by value.
template <bool DYN, typename OT, int WPB, bool VEC, bool NT>
__global__ __launch_bounds__(WPB * 64) void k_edges1dp(const KArgs a) {
    using K = K1D<DYN, 64>;
    constexpr int E = 64;
    static_assert(E * LINE_WORDS * 4 >= Rows1D<OT>::NF * 1024, "the rows' staging run fits the wave's records");
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[WPB * E * LINE_WORDS];
    const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
    const int edge0 = __builtin_amdgcn_readfirstlane(((int)blockIdx.x * WPB + wv) * E);
    if (edge0 >= a.n) return;
    const int nedge = min(E, a.n - edge0);
    const bool active = lane < nedge;
    const int edge = edge0 + (active ? lane : 0);
    LineRecs n(lds_all + wv * E * LINE_WORDS, lane);
    uint4* const nodes = (uint4*)a.grid;                             // snac_node1d[pool]
    const int srow = (int)row_of(a.src_index, a.pool, edge), drow = (int)row_of(a.dst_index, a.pool, edge);
    n.gather<fetch_but(6, 7)>(nodes, srow, nedge);
    const uint64_t gid = (uint64_t)(a.env_id_base + edge);
    const uint32_t w = rng_word(env_keys(a.key_step, gid), a.t0);
    int act = draw_action<K::A>(w, a), k = 1 + (int)(((w & 0xffffu) * 3u) >> 16);
    if (a.use_scalar) { act = a.act_scalar; k = a.k_scalar; }
    if (a.actions) act = (int)a.actions[edge];
    if (a.step_size) k = (int)a.step_size[edge];
    k = min(max(k, 1), 3);
    Lane s = n.header();
    const int episode = (int)n.word(REC_EPISODE);
    const int16_t* const prow = (const int16_t*)a.plans + (size_t)s.pidx * K::GE;
    const int r_in = min(max(s.r, 2), 31);                            // (a hand-made header: stay inside the row)
    const int pl = (int)prow[r_in - 2];                               // the one dependent load: the plan's height under the agent (L2)
    // ---- the 1D step (rules1d, snac_dev.h) on the cell under the agent (bordered position r = interior cell r - 2)
    s.r = r_in;
    const int c_old = s.r - 2;
    const Rule1D u = rules1d(s, act, k, cell1d(n, c_old), pl, a.ts_done, a.brick_gt);
    if (active && u.drop) {
        uint32_t& v = n.word_at(REC_GRID + (c_old >> 1));
        const int sh = (c_old & 1) * 16;
        v = (v & ~(0xffffu << sh)) | (((uint32_t)u.hnew & 0xffffu) << sh);
    }
    const bool done = active && u.done;
    const int reward = u.reward;
    s.ep_ret = clamp16(s.ep_ret + reward);
    s.flags = done ? SNAC_FLAG_NEED_RESET : 0;
    if (active) {
        if (a.reward) a.reward[edge] = (float)reward;
        if (a.done) a.done[edge] = done ? 1 : 0;
        n.set_header(s);
        n.word_at(REC_EPISODE) = (uint32_t)episode;
    }
    // ---- the window round the new position -- read before the records leave (the staging run takes their place)
    int win[5];
    window1d(n, s.r, win);
    n.scatter(nodes, drow, nedge, clean_piece1d);
    if (!a.obs) return;
    const Slots v = scalar_slots<DYN>(s, a.total_step);
    if constexpr (VEC) {
        Rows1D<OT> rows;
        rows.stage((char*)n.rec, lane, win, v.v0, v.v1);
        rows.template flush<NT>((char*)a.obs + (size_t)edge0 * K::D * sizeof(OT), lane, nedge);
    } else if (active) {
        write_row<5>((OT*)a.obs + (size_t)edge * K::D, [&](int i) { return win[i]; }, v);
    }
}

// 3D tree edges on node records: k_edges3d's shape (32 edges per wave, the heights through LDS -- Heights3D, nodes_dev.h -- lane = edge
// for the step and the window, rows through emit_tile) with the node record's addresses.  Header and episode counter never pass through
// LDS, so a wave's LDS is k_edges3d's 25 600 bytes (three blocks of two waves per CU).  Out: an edge onto another record writes all 56
// pieces -- header (lanes 0-31), counter (lanes 32-63), heights, the four zero pieces -- so every line it touches is whole; an edge in
// place writes its header and counter pieces and its one changed cell.
template <bool DYN, typename OT, int WPB, bool VEC>
__global__ __launch_bounds__(WPB * 64) void k_edges3dp(const KArgs a) {
    using K = K3D<DYN, 8>;
    using H3 = Heights3D;
    constexpr int E = H3::E, GE = K::GE, HP = H3::HP;
    static_assert(GE * 2 == H3::RECB && K::W == 49, "the 3D kinds' map and window");
    __shared__ __attribute__((aligned(16))) char lds_all[WPB * H3::WAVE_BYTES];
    const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
    const int edge0 = __builtin_amdgcn_readfirstlane(((int)blockIdx.x * WPB + wv) * E);
    if (edge0 >= a.n) return;
    const int nedge = min(E, a.n - edge0);
    const bool active = lane < nedge;
    const int edge = edge0 + (active ? lane : 0);
    const H3 hm(lds_all + wv * H3::WAVE_BYTES, lane);
    uint4* const nodes = (uint4*)a.grid;                             // snac_node3d[pool]
    const int srow = (int)row_of(a.src_index, a.pool, edge), drow = (int)row_of(a.dst_index, a.pool, edge);
    const int me = lane & (E - 1);                                   // (lanes 32..63 shadow 0..31: they store the counter pieces only)
    const int sme = __shfl(srow, me), dme = __shfl(drow, me);
    const bool mine_ok = me < nedge;
    Lane s;
    int episode = 0;
    {
        const uint4 h = nodes[(size_t)sme * REC3_PIECES];
        s.unpack(make_int4((int)h.x, (int)h.y, (int)h.z, (int)h.w));
        episode = ((const int32_t*)(nodes + (size_t)sme * REC3_PIECES))[REC_EPISODE];
    }
    hm.gather(nodes, srow, nedge);
    const uint64_t gid = (uint64_t)(a.env_id_base + edge);
    const uint32_t w = rng_word(env_keys(a.key_step, gid), a.t0);
    int act = draw_action<K::A>(w, a), k = 1 + (int)(((w & 0xffffu) * 3u) >> 16);
    if (a.use_scalar) { act = a.act_scalar; k = a.k_scalar; }
    if (a.actions) act = (int)a.actions[edge];
    if (a.step_size) k = (int)a.step_size[edge];
    k = min(max(k, 1), 3);
    const int d = act & 3;
    const int dr = d == 2 ? 1 : (d == 3 ? -1 : 0), dc = d == 0 ? -1 : (d == 1 ? 1 : 0);
    const int tr = s.r + dr - 3, tc = s.c + dc - 3;
    const bool inside = (unsigned)tr < 20u && (unsigned)tc < 20u;
    const int tcell = inside ? tr * 20 + tc : 0;
    const int pl = ((const int16_t*)a.plans)[(size_t)s.pidx * GE + tcell];
    const int n0 = hm.cell(s.r, s.c - 1), n1 = hm.cell(s.r, s.c + 1), n2 = hm.cell(s.r + 1, s.c), n3 = hm.cell(s.r - 1, s.c);
    const int c2 = hm.cell(s.r + 2 * dr, s.c + 2 * dc), c3 = hm.cell(s.r + 3 * dr, s.c + 3 * dc);
    const Rule3D u = rules3d<DYN>(s, act, k, n0, n1, n2, n3, c2, c3, active, a.ts_done, a.brick_gt);   // the rules: snac_dev.h
    const bool built = u.built;
    const int newh = u.newh;
    s.cross += (built && newh <= pl) ? 1 : 0;
    const bool done = u.done && active;
    const int reward = u.sel ? reward_check3d(newh, pl) : u.reward0;
    s.ep_ret = clamp16(s.ep_ret + reward);
    s.flags = done ? SNAC_FLAG_NEED_RESET : 0;
    if (built) hm.mine[tcell] = (int16_t)newh;                       // the record and the window show the built cell
    if (active) {
        if (a.reward) a.reward[edge] = (float)reward;
        if (a.done) a.done[edge] = done ? 1 : 0;
        const int4 h = s.pack();
        nodes[(size_t)drow * REC3_PIECES] = make_uint4((uint32_t)h.x, (uint32_t)h.y, (uint32_t)h.z, (uint32_t)h.w);
    }
    if (lane >= E && mine_ok) nodes[(size_t)dme * REC3_PIECES + 1] = make_uint4((uint32_t)episode, 0u, 0u, 0u);
    int cellv[K::W];
    hm.window(s.r, s.c, cellv);
    // ---- the heights leave: 16-byte pieces again, then the four zero pieces; an edge in place writes its one changed cell instead
    const bool copy = drow != srow;
    if (active && !copy && built) ((int16_t*)(nodes + (size_t)drow * REC3_PIECES + REC_GRID_PIECE))[tcell] = (int16_t)newh;
    {
        uint4 pv[HP / 2];
#pragma unroll
        for (int p = 0; p < HP / 2; ++p) pv[p] = *(const uint4*)(hm.rec + (p * 64 + lane) * 16);
#pragma unroll
        for (int p = 0; p < HP / 2; ++p) {
            const int q = p * 64 + lane, e = q / HP, l = q - HP * e;
            const int de = __shfl(drow, e);
            const bool cp = __shfl((int)copy, e) != 0;
            if (e < nedge && cp) nodes[(size_t)de * REC3_PIECES + REC_GRID_PIECE + l] = pv[p];
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int q = p * 64 + lane, e = q >> 2;
            const int de = __shfl(drow, e);
            const bool cp = __shfl((int)copy, e) != 0;
            if (e < nedge && cp) nodes[(size_t)de * REC3_PIECES + REC_GRID_PIECE + HP + (q & 3)] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    if (!a.obs) return;
    const Slots v = scalar_slots<DYN>(s, a.total_step);
    auto cell = [&](int el) { return cellv[el]; };
    if constexpr (VEC) {
        emit_tile<OT, ROWS_NT_EDGES>(hm.rec, (char*)a.obs + (size_t)edge0 * K::D * sizeof(OT), lane, nedge, cell, v.v0, v.v1);
    } else if (active) {
        write_row<K::W>((OT*)a.obs + (size_t)edge * K::D, cell, v);
    }
}

// batch rows -> node records (PACK) and back: one lane per 16-byte piece; NP pieces per record, GP pieces of grid from piece REC_GRID_PIECE
template <bool PACK, int NP, int GP>
__global__ __launch_bounds__(256) void k_nodes_copy(int4* hdr, int32_t* episode, uint4* grid, int nrows, uint4* nodes, int pool, const int32_t* rows,
                                                    const int32_t* node_rows, int m) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)m * NP) return;
    const int i = (int)(g / NP), part = (int)(g - (long long)i * NP);
    const size_t r = row_of(rows, nrows, i), nr = row_of(node_rows, pool, i);
    if (PACK) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (part == 0) { const int4 h = hdr[r]; v = make_uint4((uint32_t)h.x, (uint32_t)h.y, (uint32_t)h.z, (uint32_t)h.w); }
        else if (part == 1) v.x = (uint32_t)episode[r];
        else if (part < REC_GRID_PIECE + GP) v = grid[r * GP + (part - REC_GRID_PIECE)];
        nodes[nr * NP + part] = v;
    } else {
        const uint4 v = nodes[nr * NP + part];
        if (part == 0) hdr[r] = make_int4((int)v.x, (int)v.y, (int)v.z, (int)v.w);
        else if (part == 1) episode[r] = (int32_t)v.x;
        else if (part < REC_GRID_PIECE + GP) grid[r * GP + (part - REC_GRID_PIECE)] = v;
    }
}

template <bool DYN, typename OT>
void launch_edges2dp_part(const KArgs& a, bool vec, hipStream_t s) {
    const dim3 grid((unsigned)(((a.n + 63) / 64 + 3) / 4)), block(256);
    if (!vec) hipLaunchKernelGGL((k_edges2dp<DYN, OT, 4, false, false>), grid, block, 0, s, a);
    else if (snac_detail::tune(snac_detail::TN_NODES2D_NT) != 0) hipLaunchKernelGGL((k_edges2dp<DYN, OT, 4, true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_edges2dp<DYN, OT, 4, true, false>), grid, block, 0, s, a);
}

template <bool DYN, typename OT>
void launch_edges2dp(const KArgs& a, hipStream_t s) {
    launch_split<51, OT>(a, [s](const KArgs& b, bool vec) { launch_edges2dp_part<DYN, OT>(b, vec, s); });
}

template <bool DYN, typename OT>
void launch_edges1dp(const KArgs& a, hipStream_t s) {
    launch_split<7, OT>(a, [s](const KArgs& b, bool vec) {
        const dim3 grid((unsigned)(((b.n + 63) / 64 + 3) / 4)), block(256);
        if (vec) hipLaunchKernelGGL((k_edges1dp<DYN, OT, 4, true, ROWS_NT_EDGES>), grid, block, 0, s, b);
        else hipLaunchKernelGGL((k_edges1dp<DYN, OT, 4, false, false>), grid, block, 0, s, b);
    });
}

template <bool DYN, typename OT>
void launch_edges3dp(const KArgs& a, hipStream_t s) {
    launch_split<51, OT>(a, [s](const KArgs& b, bool vec) {
        const dim3 grid((unsigned)(((b.n + 31) / 32 + 1) / 2)), block(128);   // two waves per block: 51 KB of LDS, three blocks per CU
        if (vec) hipLaunchKernelGGL((k_edges3dp<DYN, OT, 2, true>), grid, block, 0, s, b);
        else hipLaunchKernelGGL((k_edges3dp<DYN, OT, 2, false>), grid, block, 0, s, b);
    });
}

// The 2D entry points keep a check of their own, on purpose: pack / unpack accept descriptors with a layout variant (they move state, no
// rows), the transition runs check_layout and has its own text for a variant, and the alignment text differs (tests pin it).
int nodes2d_check(const snac_env_desc* d, const snac_state* st, const void* nodes, int32_t pool_rows, int32_t m) {
    using namespace snac_detail;
    if (!d || !st || !nodes) return fail(SNAC_ERR_ARG, "null desc / state / nodes");
    if (d->kind != SNAC_ENV_2D) return fail(SNAC_ERR_UNSUPPORTED, "snac_node2d records are for the 2D kinds (1D / 3D: snac_node1d / snac_node3d)");
    if (int rc = check_common(d, st)) return rc;
    if (pool_rows < 1) return fail(SNAC_ERR_ARG, "pool_rows must be >= 1");
    if (m < 0) return fail(SNAC_ERR_ARG, "m must be >= 0");
    if (((uintptr_t)nodes & 127) != 0) return fail(SNAC_ERR_ARG, "the node pool must be 128-byte aligned (one record = one line)");
    return SNAC_OK;
}

template <bool PACK, int NP, int GP>
int nodes_copy(int kind, const char* name, const snac_env_desc* d, snac_state* st, void* nodes, int32_t pool_rows, const int32_t* rows,
               const int32_t* node_rows, int32_t m, void* stream) {
    using namespace snac_detail;
    if (int rc = kind == SNAC_ENV_2D ? nodes2d_check(d, st, nodes, pool_rows, m) : nodes_check(kind, d, st, nodes, pool_rows, m)) return rc;
    if ((!rows && m > d->num_envs) || (!node_rows && m > pool_rows)) return fail(SNAC_ERR_ARG, "m exceeds the batch / the pool");
    if (m == 0) return SNAC_OK;
    g_kernel = "k_nodes_copy";
    hipLaunchKernelGGL((k_nodes_copy<PACK, NP, GP>), dim3((unsigned)(((long long)m * NP + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int4*)st->hdr,
                       st->episode, (uint4*)st->grid, d->num_envs, (uint4*)nodes, pool_rows, rows, node_rows, m);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SNAC_OK : fail_hip(e, name);
}

int transition_nodes(int kind, const char* name, const snac_env_desc* d, const snac_state* st, void* nodes, int32_t pool_rows, int32_t m,
                     const int32_t* src_index, const int32_t* dst_index, uint32_t t, const int8_t* actions, const int8_t* step_size, void* obs,
                     float* reward, uint8_t* done, void* stream) {
    using namespace snac_detail;
    if (kind == SNAC_ENV_2D) {
        if (int rc = nodes2d_check(d, st, nodes, pool_rows, m)) return rc;
        if (int rc = check_layout(d)) return rc;
    } else if (int rc = nodes_check(kind, d, st, nodes, pool_rows, m)) return rc;
    if ((!src_index || !dst_index) && m > pool_rows) return fail(SNAC_ERR_ARG, "m exceeds the pool");
    if (m == 0) return SNAC_OK;
    KArgs a = make_args(d, st);
    if (kind == SNAC_ENV_2D && a.variant) return fail(SNAC_ERR_UNSUPPORTED, "snac_transition_nodes2d writes the canonical rows (layout variants: snac_transition)");
    a.pool = pool_rows; a.n = m; a.src_index = src_index; a.dst_index = dst_index; a.grid = nodes; a.hdr = nullptr; a.episode = nullptr;
    a.T = 1; a.t0 = t; a.actions = actions; a.step_size = step_size; a.obs = obs; a.reward = reward; a.done = done;
    a.auto_reset = 0; a.stats_on = 0;
    const bool dyn = d->dynamic != 0, f32 = d->obs_dtype == SNAC_OBS_F32;
    hipStream_t s = (hipStream_t)stream;
    if (kind == SNAC_ENV_1D) {
        g_kernel = "k_edges1dp";
        if (dyn) f32 ? launch_edges1dp<true, float>(a, s) : launch_edges1dp<true, double>(a, s);
        else f32 ? launch_edges1dp<false, float>(a, s) : launch_edges1dp<false, double>(a, s);
    } else if (kind == SNAC_ENV_2D) {
        g_kernel = "k_edges2dp";
        if (dyn) f32 ? launch_edges2dp<true, float>(a, s) : launch_edges2dp<true, double>(a, s);
        else f32 ? launch_edges2dp<false, float>(a, s) : launch_edges2dp<false, double>(a, s);
    } else {
        g_kernel = "k_edges3dp";
        if (dyn) f32 ? launch_edges3dp<true, float>(a, s) : launch_edges3dp<true, double>(a, s);
        else f32 ? launch_edges3dp<false, float>(a, s) : launch_edges3dp<false, double>(a, s);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SNAC_OK : fail_hip(e, name);
}

}  // namespace

extern "C" {

int snac_nodes1d_pack(const snac_env_desc* d, const snac_state* st, const int32_t* rows, int32_t m, snac_node1d* nodes, int32_t pool_rows,
                      const int32_t* node_rows, void* stream) {
    return nodes_copy<true, LINE_PIECES, GRID_PIECES_1D>(SNAC_ENV_1D, "snac_nodes1d_pack", d, (snac_state*)st, nodes, pool_rows, rows, node_rows, m, stream);
}

int snac_nodes1d_unpack(const snac_env_desc* d, const snac_node1d* nodes, int32_t pool_rows, const int32_t* node_rows, int32_t m, snac_state* st,
                        const int32_t* rows, void* stream) {
    return nodes_copy<false, LINE_PIECES, GRID_PIECES_1D>(SNAC_ENV_1D, "snac_nodes1d_unpack", d, st, (void*)nodes, pool_rows, rows, node_rows, m, stream);
}

int snac_transition_nodes1d(const snac_env_desc* d, const snac_state* st, snac_node1d* nodes, int32_t pool_rows, int32_t m, const int32_t* src_index,
                            const int32_t* dst_index, uint32_t t, const int8_t* actions, const int8_t* step_size, void* obs, float* reward, uint8_t* done,
                            void* stream) {
    return transition_nodes(SNAC_ENV_1D, "snac_transition_nodes1d", d, st, nodes, pool_rows, m, src_index, dst_index, t, actions, step_size, obs, reward,
                            done, stream);
}

int snac_nodes2d_pack(const snac_env_desc* d, const snac_state* st, const int32_t* rows, int32_t m, snac_node2d* nodes, int32_t pool_rows,
                      const int32_t* node_rows, void* stream) {
    return nodes_copy<true, LINE_PIECES, GRID_PIECES_2D>(SNAC_ENV_2D, "snac_nodes2d_pack", d, (snac_state*)st, nodes, pool_rows, rows, node_rows, m, stream);
}

int snac_nodes2d_unpack(const snac_env_desc* d, const snac_node2d* nodes, int32_t pool_rows, const int32_t* node_rows, int32_t m, snac_state* st,
                        const int32_t* rows, void* stream) {
    return nodes_copy<false, LINE_PIECES, GRID_PIECES_2D>(SNAC_ENV_2D, "snac_nodes2d_unpack", d, st, (void*)nodes, pool_rows, rows, node_rows, m, stream);
}

int snac_transition_nodes2d(const snac_env_desc* d, const snac_state* st, snac_node2d* nodes, int32_t pool_rows, int32_t m, const int32_t* src_index,
                            const int32_t* dst_index, uint32_t t, const int8_t* actions, const int8_t* step_size, void* obs, float* reward, uint8_t* done,
                            void* stream) {
    return transition_nodes(SNAC_ENV_2D, "snac_transition_nodes2d", d, st, nodes, pool_rows, m, src_index, dst_index, t, actions, step_size, obs, reward,
                            done, stream);
}

int snac_nodes3d_pack(const snac_env_desc* d, const snac_state* st, const int32_t* rows, int32_t m, snac_node3d* nodes, int32_t pool_rows,
                      const int32_t* node_rows, void* stream) {
    return nodes_copy<true, REC3_PIECES, GRID_PIECES_3D>(SNAC_ENV_3D, "snac_nodes3d_pack", d, (snac_state*)st, nodes, pool_rows, rows, node_rows, m, stream);
}

int snac_nodes3d_unpack(const snac_env_desc* d, const snac_node3d* nodes, int32_t pool_rows, const int32_t* node_rows, int32_t m, snac_state* st,
                        const int32_t* rows, void* stream) {
    return nodes_copy<false, REC3_PIECES, GRID_PIECES_3D>(SNAC_ENV_3D, "snac_nodes3d_unpack", d, st, (void*)nodes, pool_rows, rows, node_rows, m, stream);
}

int snac_transition_nodes3d(const snac_env_desc* d, const snac_state* st, snac_node3d* nodes, int32_t pool_rows, int32_t m, const int32_t* src_index,
                            const int32_t* dst_index, uint32_t t, const int8_t* actions, const int8_t* step_size, void* obs, float* reward, uint8_t* done,
                            void* stream) {
    return transition_nodes(SNAC_ENV_3D, "snac_transition_nodes3d", d, st, nodes, pool_rows, m, src_index, dst_index, t, actions, step_size, obs, reward,
                            done, stream);
}

}  // extern "C"
