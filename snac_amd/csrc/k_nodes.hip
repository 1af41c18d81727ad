// k_nodes.hip -- 1D and 3D tree-search node pools with ONE record per node: snac_nodes{1,3}d_pack / _unpack, snac_transition_nodes{1,3}d
#include <cstddef>

#include "snac_dev.h"
#include "rows1d.h"

// The 2D pools' idea (k_nodes2d.hip) for the other two kinds.  A tree edge (Env/1D/DMP_Env_1D_dynamic_MCTS.py:82-139,
// Env/3D/DMP_simulator_3d_dynamic_triangle_MCTS.py:195-277: transition(state, action), one call per edge in
// script/MCTS/utils/mcts_Qvalue_dynamic.py:88,118) reads its parent at a RANDOM row, and the memory side reads whole 128-byte lines
// (profiles/r06_rd_gran.txt).  On batch rows a 1D parent is three lines for 84 bytes and a 3D parent nine (800 bytes of heights at offset
// r * 800 span seven lines, plus the header's and the episode counter's).  The records, in 16-byte pieces:
//     snac_node1d   0 header | 1 episode counter, 3 zero words | 2-5 the 32 cells (30 interior + 2 pad) | 6-7 zero      = ONE line
//     snac_node3d   0 header | 1 episode counter, 3 zero words | 2-51 the 400 heights | 52-55 zero                       = seven lines
// Semantics are k_edges1d's / k_edges3d's on batch rows (rules1d / rules3d + reward_check3d, snac_dev.h), the canonical layout, no
// auto-reset and no episodic sums (the entry points switch both off).  Pad words are written as zero whatever the source holds.
static_assert(sizeof(snac_node1d) == 128 && offsetof(snac_node1d, episode) == 16 && offsetof(snac_node1d, cells) == 32 &&
              offsetof(snac_node1d, zero1) == 96, "snac_node1d: one line");
static_assert(sizeof(snac_node3d) == 896 && offsetof(snac_node3d, episode) == 16 && offsetof(snac_node3d, heights) == 32 &&
              offsetof(snac_node3d, zero1) == 832, "snac_node3d: seven lines");

namespace snac_detail {

// the argument checks every node-pool entry point of the 1D / 3D records and snac_evaluate_nodes{1,2,3}d share (snac_dev.h)
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

constexpr int N1_PIECES = 8, N1_WORDS = 32, N1_CELLS = 8;           // 1D: 16-byte pieces / 4-byte words per record; the cells' first word
constexpr int N3_PIECES = 56;                                       // 3D: pieces per record

// the piece a record leaves with: pad words zero (piece 1: the counter's three, 1D piece 5: the two pad cells, the pad pieces)
__device__ __forceinline__ uint4 clean_piece1d(uint4 v, int part) {
    if (part == 1) v.y = v.z = v.w = 0u;
    if (part == 5) v.w = 0u;
    return part < 6 ? v : make_uint4(0u, 0u, 0u, 0u);
}

// 1D tree edges on node records: k_edges2dp's record movement with k_edges1d's step.  A wave takes 64 edges; a record's eight pieces are
// fetched by eight neighbouring lanes (the two pad pieces are not read), lie in LDS for the step and the 5-cell window -- piece p of edge e
// at slot p ^ (e & 7), as in k_edges2dp -- and the whole line leaves for the destination record.  VEC: the rows as one run per wave (Rows1D,
// m % 4 == 0 and an aligned obs; the staging run reuses the records' LDS once they have left); otherwise value by value.
template <bool DYN, typename OT, int WPB, bool VEC, bool NT>
__global__ __launch_bounds__(WPB * 64) void k_edges1dp(const KArgs a) {
    using K = K1D<DYN, 64>;
    constexpr int E = 64;
    static_assert(E * N1_WORDS * 4 >= Rows1D<OT>::NF * 1024, "the rows' staging run fits the wave's records");
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[WPB * E * N1_WORDS];
    const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
    const int edge0 = __builtin_amdgcn_readfirstlane(((int)blockIdx.x * WPB + wv) * E);
    if (edge0 >= a.n) return;
    const int nedge = min(E, a.n - edge0);
    const bool active = lane < nedge;
    const int edge = edge0 + (active ? lane : 0);
    uint32_t* const rec = lds_all + wv * E * N1_WORDS;
    uint4* const nodes = (uint4*)a.grid;                             // snac_node1d[pool]
    const int srow = (int)row_of(a.src_index, a.pool, edge), drow = (int)row_of(a.dst_index, a.pool, edge);
    // ---- the source records (plain loads: children share their parents)
    uint4 rv[N1_PIECES];
#pragma unroll
    for (int i = 0; i < N1_PIECES; ++i) {
        const int g = i * 64 + lane, e = g >> 3, part = g & 7;
        const int se = __builtin_amdgcn_ds_bpermute(e << 2, srow);
        rv[i] = make_uint4(0u, 0u, 0u, 0u);
        if (g < nedge * N1_PIECES && part < 6) rv[i] = nodes[(size_t)se * N1_PIECES + part];
    }
    const uint64_t gid = (uint64_t)(a.env_id_base + edge);
    const uint32_t w = rng_word(env_keys(a.key_step, gid), a.t0);
    int act = draw_action<K::A>(w, a), k = 1 + (int)(((w & 0xffffu) * 3u) >> 16);
    if (a.use_scalar) { act = a.act_scalar; k = a.k_scalar; }
    if (a.actions) act = (int)a.actions[edge];
    if (a.step_size) k = (int)a.step_size[edge];
    k = min(max(k, 1), 3);
#pragma unroll
    for (int i = 0; i < N1_PIECES; ++i) {
        const int g = i * 64 + lane, e = g >> 3, part = g & 7;
        ((uint4*)rec)[e * N1_PIECES + (part ^ (e & 7))] = rv[i];
    }
    uint32_t* const mine = rec + lane * N1_WORDS;
    const int sw = lane & 7;
    auto word = [&](int wd) -> uint32_t& { return mine[(((wd >> 2) ^ sw) << 2) + (wd & 3)]; };   // logical word wd of this lane's record
    auto cell = [&](int j) -> int {                                  // interior cell j, or the frame (-1) for j outside 0..29
        const bool in = (unsigned)j < 30u;
        const int jj = in ? j : 0;
        const uint32_t v = word(N1_CELLS + (jj >> 1));
        return in ? (int)(int16_t)((jj & 1) ? (v >> 16) : (v & 0xffffu)) : -1;
    };
    Lane s;
    {
        const uint4 h = *(const uint4*)&mine[(0 ^ sw) << 2];
        s.unpack(make_int4((int)h.x, (int)h.y, (int)h.z, (int)h.w));
    }
    const int episode = (int)word(4);
    const int16_t* const prow = (const int16_t*)a.plans + (size_t)s.pidx * K::GE;
    const int r_in = min(max(s.r, 2), 31);                            // (a hand-made header: stay inside the row)
    const int pl = (int)prow[r_in - 2];                               // the one dependent load: the plan's height under the agent (L2)
    // ---- the 1D step (rules1d, snac_dev.h) on the cell under the agent (bordered position r = interior cell r - 2)
    s.r = r_in;
    const int c_old = s.r - 2;
    const Rule1D u = rules1d(s, act, k, cell(c_old), pl, a.ts_done, a.brick_gt);
    if (active && u.drop) {
        uint32_t& v = word(N1_CELLS + (c_old >> 1));
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
        const int4 h = s.pack();
        *(uint4*)&mine[(0 ^ sw) << 2] = make_uint4((uint32_t)h.x, (uint32_t)h.y, (uint32_t)h.z, (uint32_t)h.w);
        word(4) = (uint32_t)episode;
    }
    // ---- the window round the new position -- read before the records leave (the staging run takes their place)
    int win[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) win[i] = cell(s.r - 4 + i);
    // ---- the (updated) records leave for their destination rows, whole lines, eight neighbouring lanes per record
#pragma unroll
    for (int i = 0; i < N1_PIECES; ++i) {
        const int g = i * 64 + lane, e = g >> 3, part = g & 7;
        const int de = __builtin_amdgcn_ds_bpermute(e << 2, drow);
        if (g < nedge * N1_PIECES) nodes[(size_t)de * N1_PIECES + part] = clean_piece1d(((const uint4*)rec)[e * N1_PIECES + (part ^ (e & 7))], part);
    }
    if (!a.obs) return;
    const double c0 = (double)s.cb, c1 = (double)s.cs;
    const double v0 = DYN ? c0 / (double)s.tb : c0, v1 = DYN ? c1 / (double)a.total_step : c1;
    if constexpr (VEC) {
        Rows1D<OT> rows;
        rows.stage((char*)rec, lane, win, v0, v1);
        rows.template flush<NT>((char*)a.obs + (size_t)edge0 * K::D * sizeof(OT), lane, nedge);
    } else if (active) {
        OT* const o = (OT*)a.obs + (size_t)edge * K::D;
#pragma unroll
        for (int i = 0; i < 5; ++i) o[i] = (OT)win[i];
        o[5] = (OT)v0; o[6] = (OT)v1;
    }
}

// 3D tree edges on node records: k_edges3d's shape (32 edges per wave, the heights through LDS as REC[edge][400 cells], lane = edge for the
// step and the window, rows through emit_tile) with the node record's addresses.  Lane l (and its shadow l + 32) loads the header and
// episode counter of edge l & 31 itself -- they never pass through LDS, so a wave's LDS is k_edges3d's 25 600 bytes (three blocks of two
// waves per CU) -- and piece q of the wave's 32 x 50 height pieces (edge q / 50) arrives at piece 2 + q % 50 of its record.  Out: an edge
// onto another record writes all 56 pieces -- header (lanes 0-31), counter (lanes 32-63), heights, the four zero pieces -- so every
// line it touches is whole; an edge in place writes its header and counter pieces and its one changed cell.
template <bool DYN, typename OT, int WPB, bool VEC>
__global__ __launch_bounds__(WPB * 64) void k_edges3dp(const KArgs a) {
    using K = K3D<DYN, 8>;
    constexpr int E = 32, GE = K::GE, RECB = GE * 2, HP = GE * 2 / 16;   // 800 bytes = 50 pieces of heights per record
    constexpr int WAVE_BYTES = E * RECB > TILE_STG_BYTES ? E * RECB : TILE_STG_BYTES;
    __shared__ __attribute__((aligned(16))) char lds_all[WPB * WAVE_BYTES];
    const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
    const int edge0 = __builtin_amdgcn_readfirstlane(((int)blockIdx.x * WPB + wv) * E);
    if (edge0 >= a.n) return;
    const int nedge = min(E, a.n - edge0);
    const bool active = lane < nedge;
    const int edge = edge0 + (active ? lane : 0);
    char* const rec = lds_all + wv * WAVE_BYTES;
    uint4* const nodes = (uint4*)a.grid;                             // snac_node3d[pool]
    const int srow = (int)row_of(a.src_index, a.pool, edge), drow = (int)row_of(a.dst_index, a.pool, edge);
    const int me = lane & (E - 1);                                   // (lanes 32..63 shadow 0..31: they store the counter pieces only)
    const int sme = __shfl(srow, me), dme = __shfl(drow, me);
    const bool mine_ok = me < nedge;
    Lane s;
    int episode = 0;
    {
        const uint4 h = nodes[(size_t)sme * N3_PIECES];
        s.unpack(make_int4((int)h.x, (int)h.y, (int)h.z, (int)h.w));
        episode = ((const int32_t*)(nodes + (size_t)sme * N3_PIECES + 1))[0];
    }
    {
        uint4 pv[HP / 2];                                            // 25 loads in flight
#pragma unroll
        for (int p = 0; p < HP / 2; ++p) {
            const int q = p * 64 + lane, e = q / HP, l = q - HP * e;
            const int se = __shfl(srow, e);
            pv[p] = e < nedge ? nodes[(size_t)se * N3_PIECES + 2 + l] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int p = 0; p < HP / 2; ++p) *(uint4*)(rec + (p * 64 + lane) * 16) = pv[p];
    }
    const uint64_t gid = (uint64_t)(a.env_id_base + edge);
    const uint32_t w = rng_word(env_keys(a.key_step, gid), a.t0);
    int act = draw_action<K::A>(w, a), k = 1 + (int)(((w & 0xffffu) * 3u) >> 16);
    if (a.use_scalar) { act = a.act_scalar; k = a.k_scalar; }
    if (a.actions) act = (int)a.actions[edge];
    if (a.step_size) k = (int)a.step_size[edge];
    k = min(max(k, 1), 3);
    int16_t* const mine = (int16_t*)(rec + me * RECB);
    auto cell = [&](int R, int C) -> int {                           // a cell of the edge's map in bordered coordinates: the frame is -1
        const bool in = (unsigned)(R - 3) < 20u && (unsigned)(C - 3) < 20u;
        const int v = (int)mine[in ? (R - 3) * 20 + (C - 3) : 0];
        return in ? v : -1;
    };
    const int d = act & 3;
    const int dr = d == 2 ? 1 : (d == 3 ? -1 : 0), dc = d == 0 ? -1 : (d == 1 ? 1 : 0);
    const int tr = s.r + dr - 3, tc = s.c + dc - 3;
    const bool inside = (unsigned)tr < 20u && (unsigned)tc < 20u;
    const int tcell = inside ? tr * 20 + tc : 0;
    const int pl = ((const int16_t*)a.plans)[(size_t)s.pidx * GE + tcell];
    const int n0 = cell(s.r, s.c - 1), n1 = cell(s.r, s.c + 1), n2 = cell(s.r + 1, s.c), n3 = cell(s.r - 1, s.c);
    const int c2 = cell(s.r + 2 * dr, s.c + 2 * dc), c3 = cell(s.r + 3 * dr, s.c + 3 * dc);
    const Rule3D u = rules3d<DYN>(s, act, k, n0, n1, n2, n3, c2, c3, active, a.ts_done, a.brick_gt);   // the rules: snac_dev.h
    const bool built = u.built;
    const int newh = u.newh;
    s.cross += (built && newh <= pl) ? 1 : 0;
    const bool done = u.done && active;
    const int reward = u.sel ? reward_check3d(newh, pl) : u.reward0;
    s.ep_ret = clamp16(s.ep_ret + reward);
    s.flags = done ? SNAC_FLAG_NEED_RESET : 0;
    if (built) mine[tcell] = (int16_t)newh;                          // the record and the window show the built cell
    if (active) {
        if (a.reward) a.reward[edge] = (float)reward;
        if (a.done) a.done[edge] = done ? 1 : 0;
        const int4 h = s.pack();
        nodes[(size_t)drow * N3_PIECES] = make_uint4((uint32_t)h.x, (uint32_t)h.y, (uint32_t)h.z, (uint32_t)h.w);
    }
    if (lane >= E && mine_ok) nodes[(size_t)dme * N3_PIECES + 1] = make_uint4((uint32_t)episode, 0u, 0u, 0u);
    int cellv[K::W];
#pragma unroll
    for (int el = 0; el < K::W; ++el) { const int i = el / 7, j = el - 7 * i; cellv[el] = cell(s.r - 3 + i, s.c - 3 + j); }
    // ---- the heights leave: 16-byte pieces again, then the four zero pieces; an edge in place writes its one changed cell instead
    const bool copy = drow != srow;
    if (active && !copy && built) ((int16_t*)(nodes + (size_t)drow * N3_PIECES + 2))[tcell] = (int16_t)newh;
    {
        uint4 pv[HP / 2];
#pragma unroll
        for (int p = 0; p < HP / 2; ++p) pv[p] = *(const uint4*)(rec + (p * 64 + lane) * 16);
#pragma unroll
        for (int p = 0; p < HP / 2; ++p) {
            const int q = p * 64 + lane, e = q / HP, l = q - HP * e;
            const int de = __shfl(drow, e);
            const bool cp = __shfl((int)copy, e) != 0;
            if (e < nedge && cp) nodes[(size_t)de * N3_PIECES + 2 + l] = pv[p];
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int q = p * 64 + lane, e = q >> 2;
            const int de = __shfl(drow, e);
            const bool cp = __shfl((int)copy, e) != 0;
            if (e < nedge && cp) nodes[(size_t)de * N3_PIECES + 2 + HP + (q & 3)] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    if (!a.obs) return;
    const double c0 = (double)s.cb, c1 = (double)s.cs;
    const double v0 = DYN ? c0 / (double)s.tb : c0, v1 = DYN ? c1 / (double)a.total_step : c1;
    if constexpr (VEC) {
        emit_tile<OT, ROWS_NT_EDGES>(rec, (char*)a.obs + (size_t)edge0 * K::D * sizeof(OT), lane, nedge, [&](int el) { return cellv[el]; }, v0, v1);
    } else if (active) {
        OT* const o = (OT*)a.obs + (size_t)edge * K::D;
#pragma unroll
        for (int el = 0; el < K::W; ++el) o[el] = (OT)cellv[el];
        o[K::W] = (OT)v0; o[K::W + 1] = (OT)v1;
    }
}

// batch rows -> node records (PACK) and back: one lane per 16-byte piece; NP pieces per record, GP pieces of grid record from piece 2
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
        else if (part < 2 + GP) v = grid[r * GP + (part - 2)];
        nodes[nr * NP + part] = v;
    } else {
        const uint4 v = nodes[nr * NP + part];
        if (part == 0) hdr[r] = make_int4((int)v.x, (int)v.y, (int)v.z, (int)v.w);
        else if (part == 1) episode[r] = (int32_t)v.x;
        else if (part < 2 + GP) grid[r * GP + (part - 2)] = v;
    }
}

// whole 16-byte pieces of rows (m % 4 = 0, an aligned obs) through the wave's run; otherwise the first m & ~3 edges that way and the last
// one to three as a launch of their own when both index arrays are given (launch_edges2dp), else every row value by value
template <int D, typename OT, class Part>
void launch_split(const KArgs& a, Part part) {
    const bool aligned = !a.obs || ((uintptr_t)a.obs & 15) == 0;
    const int head = a.n & ~3;
    if (aligned && head == a.n) { part(a, true); return; }
    if (!aligned || head == 0 || !a.src_index || !a.dst_index) { part(a, false); return; }
    KArgs h = a, t = a;
    h.n = head;
    t.n = a.n - head;
    t.src_index += head; t.dst_index += head;
    if (t.actions) t.actions += head;
    if (t.step_size) t.step_size += head;
    if (t.reward) t.reward += head;
    if (t.done) t.done += head;
    if (t.obs) t.obs = (char*)t.obs + (size_t)head * D * sizeof(OT);
    t.env_id_base += head;                                           // the counter RNG is keyed by the edge's index in the call
    part(h, true);
    part(t, false);
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

template <bool PACK, int NP, int GP>
int nodes_copy(int kind, const char* name, const snac_env_desc* d, snac_state* st, void* nodes, int32_t pool_rows, const int32_t* rows,
               const int32_t* node_rows, int32_t m, void* stream) {
    using namespace snac_detail;
    if (int rc = nodes_check(kind, d, st, nodes, pool_rows, m)) return rc;
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
    if (int rc = nodes_check(kind, d, st, nodes, pool_rows, m)) return rc;
    if ((!src_index || !dst_index) && m > pool_rows) return fail(SNAC_ERR_ARG, "m exceeds the pool");
    if (m == 0) return SNAC_OK;
    KArgs a = make_args(d, st);
    a.pool = pool_rows; a.n = m; a.src_index = src_index; a.dst_index = dst_index; a.grid = nodes; a.hdr = nullptr; a.episode = nullptr;
    a.T = 1; a.t0 = t; a.actions = actions; a.step_size = step_size; a.obs = obs; a.reward = reward; a.done = done;
    a.auto_reset = 0; a.stats_on = 0;
    const bool dyn = d->dynamic != 0, f32 = d->obs_dtype == SNAC_OBS_F32;
    hipStream_t s = (hipStream_t)stream;
    if (kind == SNAC_ENV_1D) {
        g_kernel = "k_edges1dp";
        if (dyn) f32 ? launch_edges1dp<true, float>(a, s) : launch_edges1dp<true, double>(a, s);
        else f32 ? launch_edges1dp<false, float>(a, s) : launch_edges1dp<false, double>(a, s);
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
    return nodes_copy<true, N1_PIECES, 4>(SNAC_ENV_1D, "snac_nodes1d_pack", d, (snac_state*)st, nodes, pool_rows, rows, node_rows, m, stream);
}

int snac_nodes1d_unpack(const snac_env_desc* d, const snac_node1d* nodes, int32_t pool_rows, const int32_t* node_rows, int32_t m, snac_state* st,
                        const int32_t* rows, void* stream) {
    return nodes_copy<false, N1_PIECES, 4>(SNAC_ENV_1D, "snac_nodes1d_unpack", d, st, (void*)nodes, pool_rows, rows, node_rows, m, stream);
}

int snac_transition_nodes1d(const snac_env_desc* d, const snac_state* st, snac_node1d* nodes, int32_t pool_rows, int32_t m, const int32_t* src_index,
                            const int32_t* dst_index, uint32_t t, const int8_t* actions, const int8_t* step_size, void* obs, float* reward, uint8_t* done,
                            void* stream) {
    return transition_nodes(SNAC_ENV_1D, "snac_transition_nodes1d", d, st, nodes, pool_rows, m, src_index, dst_index, t, actions, step_size, obs, reward,
                            done, stream);
}

int snac_nodes3d_pack(const snac_env_desc* d, const snac_state* st, const int32_t* rows, int32_t m, snac_node3d* nodes, int32_t pool_rows,
                      const int32_t* node_rows, void* stream) {
    return nodes_copy<true, N3_PIECES, 50>(SNAC_ENV_3D, "snac_nodes3d_pack", d, (snac_state*)st, nodes, pool_rows, rows, node_rows, m, stream);
}

int snac_nodes3d_unpack(const snac_env_desc* d, const snac_node3d* nodes, int32_t pool_rows, const int32_t* node_rows, int32_t m, snac_state* st,
                        const int32_t* rows, void* stream) {
    return nodes_copy<false, N3_PIECES, 50>(SNAC_ENV_3D, "snac_nodes3d_unpack", d, st, (void*)nodes, pool_rows, rows, node_rows, m, stream);
}

int snac_transition_nodes3d(const snac_env_desc* d, const snac_state* st, snac_node3d* nodes, int32_t pool_rows, int32_t m, const int32_t* src_index,
                            const int32_t* dst_index, uint32_t t, const int8_t* actions, const int8_t* step_size, void* obs, float* reward, uint8_t* done,
                            void* stream) {
    return transition_nodes(SNAC_ENV_3D, "snac_transition_nodes3d", d, st, nodes, pool_rows, m, src_index, dst_index, t, actions, step_size, obs, reward,
                            done, stream);
}

}  // extern "C"
