// k_nodes_obs.hip -- the observation rows of node records: snac_observe_nodes1d / 2d / 3d (what a policy / value network reads of the leaves
// of a tree search: snac_amd/uct.py, evaluator=)
#include "snac_dev.h"
#include "rows1d.h"

// obs[i] = the canonical row of record node_rows[i]: the window round the record's position and the two scalar slots, as snac_observe
// writes them for a batch row holding that state (the flags do not enter: a record with SNAC_FLAG_NEED_RESET shows its last state).  A leaf
// batch names RANDOM records, and the memory side reads whole 128-byte lines (profiles/r06_rd_gran.txt), so the records are fetched as the
// tree-edge kernels fetch theirs -- k_edges2dp / k_edges1dp: a wave takes 64 records, eight neighbouring lanes the eight 16-byte pieces of
// one, through LDS at piece slot p ^ (e & 7); k_edges3dp: 32 records per wave, the 50 height pieces of each through LDS, header per lane --
// and the rows leave as the wave's one run of 16-byte stores (emit_tile, Rows1D).  Nothing is stepped and nothing is written but the rows.
// VEC = false: rows value by value (the last m % 4 rows of a call, an unaligned obs).  Plain stores: the evaluator reads the rows next.
namespace {

struct ObsArgs {
    const uint4* nodes;
    int32_t pool, m, row0;     // row0: the record of index 0 when node_rows is NULL (the tail launch of a split call)
    const int32_t* node_rows;
    void* obs;
    int32_t total_step;
};

__device__ __forceinline__ int obs_row(const ObsArgs& a, int i) {
    return a.node_rows ? (int)row_of(a.node_rows, a.pool, i) : min(a.row0 + i, a.pool - 1);
}

constexpr int ON_WORDS = 32, ON_PIECES = 8, ON_GRID = 8;            // a 1D / 2D record in words / pieces; the grid's first word

template <bool DYN, typename OT, int WPB, bool VEC>
__global__ __launch_bounds__(WPB * 64) void k_observe2dp(const ObsArgs a) {
    using K = K2D<DYN, 64>;
    constexpr int E = 64, GE = K::GE;
    static_assert(E * ON_WORDS * 4 <= TILE_STG_BYTES, "the records of a wave fit its staging tile");
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[WPB * (TILE_STG_BYTES / 4)];
    const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
    const int i0 = __builtin_amdgcn_readfirstlane(((int)blockIdx.x * WPB + wv) * E);
    if (i0 >= a.m) return;
    const int nrec = min(E, a.m - i0);
    const bool active = lane < nrec;
    const int i = i0 + (active ? lane : 0);
    uint32_t* const rec = lds_all + wv * (TILE_STG_BYTES / 4);
    const int srow = obs_row(a, i);
    uint4 rv[ON_PIECES];
#pragma unroll
    for (int p = 0; p < ON_PIECES; ++p) {                            // header and board: pieces 0 and 2 .. 6 of the line
        const int g = p * 64 + lane, e = g >> 3, part = g & 7;
        const int se = __builtin_amdgcn_ds_bpermute(e << 2, srow);
        rv[p] = make_uint4(0u, 0u, 0u, 0u);
        if (g < nrec * ON_PIECES && part != 1 && part != 7) rv[p] = a.nodes[(size_t)se * ON_PIECES + part];
    }
#pragma unroll
    for (int p = 0; p < ON_PIECES; ++p) {
        const int g = p * 64 + lane, e = g >> 3, part = g & 7;
        ((uint4*)rec)[e * ON_PIECES + (part ^ (e & 7))] = rv[p];
    }
    const uint32_t* const mine = rec + lane * ON_WORDS;
    const int sw = lane & 7;
    auto word = [&](int wd) -> uint32_t { return mine[(((wd >> 2) ^ sw) << 2) + (wd & 3)]; };   // logical word wd of this lane's record
    Lane s;
    {
        const uint4 h = *(const uint4*)&mine[(0 ^ sw) << 2];
        s.unpack(make_int4((int)h.x, (int)h.y, (int)h.z, (int)h.w));
    }
    // the window round the position as two-bit codes (00 empty / 01 brick / 11 frame), 14 bits per row: k_edges2dp's
    uint32_t wr[7];
    {
        const int sh = min(max(s.c - 3, 0), 19);                     // first window column, bordered
        constexpr uint32_t FRAME26 = 0x3800007u;
        const uint32_t frm = spread16((FRAME26 >> sh) & 0x7Fu) * 3u;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int q = s.r - 6 + j;
            const bool in = (unsigned)q < (unsigned)GE;
            const uint32_t g = word(ON_GRID + (in ? q : 0));
            wr[j] = in ? (spread16(((g << 3) >> sh) & 0x7Fu) | frm) : 0x3FFFu;
        }
    }
    const double c0 = (double)s.cb, c1 = (double)s.cs;
    const double v0 = DYN ? c0 / (double)s.tb : c0, v1 = DYN ? c1 / (double)a.total_step : c1;
    auto cell = [&](int el) { const int r = el / 7, j = el - 7 * r; return ((int)(wr[r] << (30 - 2 * j))) >> 30; };
    if constexpr (VEC) {
        asm volatile("" ::: "memory");                               // (every read of the records above, every write of the rows below)
        emit_tile<OT, false>((char*)rec, (char*)a.obs + (size_t)i0 * K::D * sizeof(OT), lane, nrec, cell, v0, v1);
    } else if (active) {
        OT* const o = (OT*)a.obs + (size_t)i * K::D;
#pragma unroll
        for (int el = 0; el < K::W; ++el) o[el] = (OT)cell(el);
        o[K::W] = (OT)v0; o[K::W + 1] = (OT)v1;
    }
}

template <bool DYN, typename OT, int WPB, bool VEC>
__global__ __launch_bounds__(WPB * 64) void k_observe1dp(const ObsArgs a) {
    using K = K1D<DYN, 64>;
    constexpr int E = 64;
    static_assert(E * ON_WORDS * 4 >= Rows1D<OT>::NF * 1024, "the rows' staging run fits the wave's records");
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[WPB * E * ON_WORDS];
    const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
    const int i0 = __builtin_amdgcn_readfirstlane(((int)blockIdx.x * WPB + wv) * E);
    if (i0 >= a.m) return;
    const int nrec = min(E, a.m - i0);
    const bool active = lane < nrec;
    const int i = i0 + (active ? lane : 0);
    uint32_t* const rec = lds_all + wv * E * ON_WORDS;
    const int srow = obs_row(a, i);
    uint4 rv[ON_PIECES];
#pragma unroll
    for (int p = 0; p < ON_PIECES; ++p) {                            // header and cells: pieces 0 and 2 .. 5 of the line
        const int g = p * 64 + lane, e = g >> 3, part = g & 7;
        const int se = __builtin_amdgcn_ds_bpermute(e << 2, srow);
        rv[p] = make_uint4(0u, 0u, 0u, 0u);
        if (g < nrec * ON_PIECES && part != 1 && part < 6) rv[p] = a.nodes[(size_t)se * ON_PIECES + part];
    }
#pragma unroll
    for (int p = 0; p < ON_PIECES; ++p) {
        const int g = p * 64 + lane, e = g >> 3, part = g & 7;
        ((uint4*)rec)[e * ON_PIECES + (part ^ (e & 7))] = rv[p];
    }
    const uint32_t* const mine = rec + lane * ON_WORDS;
    const int sw = lane & 7;
    auto word = [&](int wd) -> uint32_t { return mine[(((wd >> 2) ^ sw) << 2) + (wd & 3)]; };
    auto cell = [&](int j) -> int {                                  // interior cell j, or the frame (-1) for j outside 0..29
        const bool in = (unsigned)j < 30u;
        const int jj = in ? j : 0;
        const uint32_t v = word(ON_GRID + (jj >> 1));
        return in ? (int)(int16_t)((jj & 1) ? (v >> 16) : (v & 0xffffu)) : -1;
    };
    Lane s;
    {
        const uint4 h = *(const uint4*)&mine[(0 ^ sw) << 2];
        s.unpack(make_int4((int)h.x, (int)h.y, (int)h.z, (int)h.w));
    }
    int win[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) win[j] = cell(s.r - 4 + j);          // bordered position r = interior cell r - 2
    const double c0 = (double)s.cb, c1 = (double)s.cs;
    const double v0 = DYN ? c0 / (double)s.tb : c0, v1 = DYN ? c1 / (double)a.total_step : c1;
    if constexpr (VEC) {
        asm volatile("" ::: "memory");                               // (the records are read, the staging run takes their place)
        Rows1D<OT> rows;
        rows.stage((char*)rec, lane, win, v0, v1);
        rows.template flush<false>((char*)a.obs + (size_t)i0 * K::D * sizeof(OT), lane, nrec);
    } else if (active) {
        OT* const o = (OT*)a.obs + (size_t)i * K::D;
#pragma unroll
        for (int j = 0; j < 5; ++j) o[j] = (OT)win[j];
        o[5] = (OT)v0; o[6] = (OT)v1;
    }
}

constexpr int ON3_PIECES = 56;

template <bool DYN, typename OT, int WPB, bool VEC>
__global__ __launch_bounds__(WPB * 64) void k_observe3dp(const ObsArgs a) {
    using K = K3D<DYN, 8>;
    constexpr int E = 32, GE = K::GE, RECB = GE * 2, HP = GE * 2 / 16;   // 800 bytes = 50 pieces of heights per record
    constexpr int WAVE_BYTES = E * RECB > TILE_STG_BYTES ? E * RECB : TILE_STG_BYTES;
    __shared__ __attribute__((aligned(16))) char lds_all[WPB * WAVE_BYTES];
    const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
    const int i0 = __builtin_amdgcn_readfirstlane(((int)blockIdx.x * WPB + wv) * E);
    if (i0 >= a.m) return;
    const int nrec = min(E, a.m - i0);
    const bool active = lane < nrec;
    const int i = i0 + (active ? lane : 0);
    char* const rec = lds_all + wv * WAVE_BYTES;
    const int srow = obs_row(a, i);
    const int me = lane & (E - 1);                                   // (lanes 32..63 shadow 0..31)
    const int sme = __shfl(srow, me);
    Lane s;
    {
        const uint4 h = a.nodes[(size_t)sme * ON3_PIECES];
        s.unpack(make_int4((int)h.x, (int)h.y, (int)h.z, (int)h.w));
    }
    {
        uint4 pv[HP / 2];                                            // 25 loads in flight
#pragma unroll
        for (int p = 0; p < HP / 2; ++p) {
            const int q = p * 64 + lane, e = q / HP, l = q - HP * e;
            const int se = __shfl(srow, e);
            pv[p] = e < nrec ? a.nodes[(size_t)se * ON3_PIECES + 2 + l] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int p = 0; p < HP / 2; ++p) *(uint4*)(rec + (p * 64 + lane) * 16) = pv[p];
    }
    const int16_t* const mine = (const int16_t*)(rec + me * RECB);
    auto cell = [&](int R, int C) -> int {                           // bordered coordinates: the frame is -1
        const bool in = (unsigned)(R - 3) < 20u && (unsigned)(C - 3) < 20u;
        const int v = (int)mine[in ? (R - 3) * 20 + (C - 3) : 0];
        return in ? v : -1;
    };
    int cellv[K::W];
#pragma unroll
    for (int el = 0; el < K::W; ++el) { const int r = el / 7, j = el - 7 * r; cellv[el] = cell(s.r - 3 + r, s.c - 3 + j); }
    const double c0 = (double)s.cb, c1 = (double)s.cs;
    const double v0 = DYN ? c0 / (double)s.tb : c0, v1 = DYN ? c1 / (double)a.total_step : c1;
    if constexpr (VEC) {
        asm volatile("" ::: "memory");
        emit_tile<OT, false>(rec, (char*)a.obs + (size_t)i0 * K::D * sizeof(OT), lane, nrec, [&](int el) { return cellv[el]; }, v0, v1);
    } else if (active) {
        OT* const o = (OT*)a.obs + (size_t)i * K::D;
#pragma unroll
        for (int el = 0; el < K::W; ++el) o[el] = (OT)cellv[el];
        o[K::W] = (OT)v0; o[K::W + 1] = (OT)v1;
    }
}

// whole 16-byte pieces of rows for the first m & ~3 records (an aligned obs), the last one to three value by value in a launch of their own
template <int D, typename OT, class Part>
void observe_split(const ObsArgs& a, Part part) {
    const bool aligned = ((uintptr_t)a.obs & 15) == 0;
    const int head = aligned ? a.m & ~3 : 0;
    if (head) {
        ObsArgs h = a;
        h.m = head;
        part(h, true);
    }
    if (head < a.m) {
        ObsArgs t = a;
        t.m = a.m - head;
        if (t.node_rows) t.node_rows += head; else t.row0 += head;
        t.obs = (char*)a.obs + (size_t)head * D * sizeof(OT);
        part(t, false);
    }
}

template <int KIND, bool DYN, typename OT>
void launch_observe(const ObsArgs& a, hipStream_t s) {
    if constexpr (KIND == SNAC_ENV_3D) {
        observe_split<51, OT>(a, [s](const ObsArgs& b, bool vec) {
            const dim3 grid((unsigned)(((b.m + 31) / 32 + 1) / 2)), block(128);   // two waves per block, as k_edges3dp
            if (vec) hipLaunchKernelGGL((k_observe3dp<DYN, OT, 2, true>), grid, block, 0, s, b);
            else hipLaunchKernelGGL((k_observe3dp<DYN, OT, 2, false>), grid, block, 0, s, b);
        });
    } else {
        observe_split<KIND == SNAC_ENV_1D ? 7 : 51, OT>(a, [s](const ObsArgs& b, bool vec) {
            const dim3 grid((unsigned)(((b.m + 63) / 64 + 3) / 4)), block(256);
            if constexpr (KIND == SNAC_ENV_1D) {
                if (vec) hipLaunchKernelGGL((k_observe1dp<DYN, OT, 4, true>), grid, block, 0, s, b);
                else hipLaunchKernelGGL((k_observe1dp<DYN, OT, 4, false>), grid, block, 0, s, b);
            } else {
                if (vec) hipLaunchKernelGGL((k_observe2dp<DYN, OT, 4, true>), grid, block, 0, s, b);
                else hipLaunchKernelGGL((k_observe2dp<DYN, OT, 4, false>), grid, block, 0, s, b);
            }
        });
    }
}

template <int KIND>
int observe_nodes(const char* name, const char* kernel, const snac_env_desc* d, const snac_state* st, const void* nodes, int32_t pool_rows, int32_t m,
                  const int32_t* node_rows, void* obs, void* stream) {
    using namespace snac_detail;
    if (int rc = nodes_check(KIND, d, st, nodes, pool_rows, m)) return rc;
    if (!obs) return fail(SNAC_ERR_ARG, "null obs");
    if (!node_rows && m > pool_rows) return fail(SNAC_ERR_ARG, "m exceeds the pool");
    if (m == 0) return SNAC_OK;
    const KArgs k = make_args(d, st);
    const ObsArgs a{(const uint4*)nodes, pool_rows, m, 0, node_rows, obs, k.total_step};
    g_kernel = kernel;
    const bool dyn = d->dynamic != 0, f32 = d->obs_dtype == SNAC_OBS_F32;
    hipStream_t s = (hipStream_t)stream;
    if (dyn) f32 ? launch_observe<KIND, true, float>(a, s) : launch_observe<KIND, true, double>(a, s);
    else f32 ? launch_observe<KIND, false, float>(a, s) : launch_observe<KIND, false, double>(a, s);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SNAC_OK : fail_hip(e, name);
}

}  // namespace

extern "C" {

int snac_observe_nodes1d(const snac_env_desc* d, const snac_state* st, const snac_node1d* nodes, int32_t pool_rows, int32_t m, const int32_t* node_rows,
                         void* obs, void* stream) {
    return observe_nodes<SNAC_ENV_1D>("snac_observe_nodes1d", "k_observe1dp", d, st, nodes, pool_rows, m, node_rows, obs, stream);
}

int snac_observe_nodes2d(const snac_env_desc* d, const snac_state* st, const snac_node2d* nodes, int32_t pool_rows, int32_t m, const int32_t* node_rows,
                         void* obs, void* stream) {
    return observe_nodes<SNAC_ENV_2D>("snac_observe_nodes2d", "k_observe2dp", d, st, nodes, pool_rows, m, node_rows, obs, stream);
}

int snac_observe_nodes3d(const snac_env_desc* d, const snac_state* st, const snac_node3d* nodes, int32_t pool_rows, int32_t m, const int32_t* node_rows,
                         void* obs, void* stream) {
    return observe_nodes<SNAC_ENV_3D>("snac_observe_nodes3d", "k_observe3dp", d, st, nodes, pool_rows, m, node_rows, obs, stream);
}

}  // extern "C"
