// k_nodes_obs.hip -- the observation rows of node records: snac_observe_nodes1d / 2d / 3d (what a policy / value network reads of the leaves
// of a tree search: snac_amd/uct.py, evaluator=)
#include "nodes_dev.h"
#include "rows1d.h"

// obs[i] = the canonical row of record node_rows[i]: the window round the record's position and the two scalar slots, as snac_observe
// writes them for a batch row holding that state (the flags do not enter: a record with SNAC_FLAG_NEED_RESET shows its last state).  A leaf
// batch names RANDOM records, and the memory side reads whole 128-byte lines (profiles/r06_rd_gran.txt), so the records are fetched as the
// tree-edge kernels fetch theirs (nodes_dev.h: LineRecs for 1D / 2D, 64 records per wave; Heights3D, 32 records per wave, header per lane)
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

template <bool DYN, typename OT, int WPB, bool VEC>
__global__ __launch_bounds__(WPB * 64) void k_observe2dp(const ObsArgs a) {
    using K = K2D<DYN, 64>;
    constexpr int E = 64;
    static_assert(E * LINE_WORDS * 4 <= TILE_STG_BYTES, "the records of a wave fit its staging tile");
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[WPB * (TILE_STG_BYTES / 4)];
    const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
    const int i0 = __builtin_amdgcn_readfirstlane(((int)blockIdx.x * WPB + wv) * E);
    if (i0 >= a.m) return;
    const int nrec = min(E, a.m - i0);
    const bool active = lane < nrec;
    const int i = i0 + (active ? lane : 0);
    LineRecs n(lds_all + wv * (TILE_STG_BYTES / 4), lane);
    n.gather<fetch_but(1, 7)>(a.nodes, obs_row(a, i), nrec);         // header and board
    const Lane s = n.header();
    const Window2D cell(n, s.r, min(max(s.c - 3, 0), 19), K::GE);    // (a hand-made record: the first window column is clamped)
    const Slots v = scalar_slots<DYN>(s, a.total_step);
    if constexpr (VEC) {
        asm volatile("" ::: "memory");                               // (every read of the records above, every write of the rows below)
        emit_tile<OT, false>((char*)n.rec, (char*)a.obs + (size_t)i0 * K::D * sizeof(OT), lane, nrec, cell, v.v0, v.v1);
    } else if (active) {
        write_row<K::W>((OT*)a.obs + (size_t)i * K::D, cell, v);
    }
}

template <bool DYN, typename OT, int WPB, bool VEC>
__global__ __launch_bounds__(WPB * 64) void k_observe1dp(const ObsArgs a) {
    using K = K1D<DYN, 64>;
    constexpr int E = 64;
    static_assert(E * LINE_WORDS * 4 >= Rows1D<OT>::NF * 1024, "the rows' staging run fits the wave's records");
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[WPB * E * LINE_WORDS];
    const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
    const int i0 = __builtin_amdgcn_readfirstlane(((int)blockIdx.x * WPB + wv) * E);
    if (i0 >= a.m) return;
    const int nrec = min(E, a.m - i0);
    const bool active = lane < nrec;
    const int i = i0 + (active ? lane : 0);
    uint32_t* const rec = lds_all + wv * E * LINE_WORDS;
    const int srow = obs_row(a, i);
    // LineRecs::gather with the pieces 0 and 2 .. 5 (header and cells), written out: through the shared helper this kernel, alone of
    // the six, takes two to four more registers
    uint4 rv[LINE_PIECES];
#pragma unroll
    for (int p = 0; p < LINE_PIECES; ++p) {
        const int g = p * 64 + lane, e = g >> 3, part = g & 7;
        const int se = __builtin_amdgcn_ds_bpermute(e << 2, srow);
        rv[p] = make_uint4(0u, 0u, 0u, 0u);
        if (g < nrec * LINE_PIECES && part != 1 && part < 6) rv[p] = a.nodes[(size_t)se * LINE_PIECES + part];
    }
#pragma unroll
    for (int p = 0; p < LINE_PIECES; ++p) {
        const int g = p * 64 + lane, e = g >> 3, part = g & 7;
        ((uint4*)rec)[line_slot(e, part)] = rv[p];
    }
    const LineRecs n(rec, lane);
    const Lane s = n.header();
    int win[5];
    window1d(n, s.r, win);
    const Slots v = scalar_slots<DYN>(s, a.total_step);
    if constexpr (VEC) {
        asm volatile("" ::: "memory");                               // (the records are read, the staging run takes their place)
        Rows1D<OT> rows;
        rows.stage((char*)rec, lane, win, v.v0, v.v1);
        rows.template flush<false>((char*)a.obs + (size_t)i0 * K::D * sizeof(OT), lane, nrec);
    } else if (active) {
        write_row<5>((OT*)a.obs + (size_t)i * K::D, [&](int j) { return win[j]; }, v);
    }
}

template <bool DYN, typename OT, int WPB, bool VEC>
__global__ __launch_bounds__(WPB * 64) void k_observe3dp(const ObsArgs a) {
    using K = K3D<DYN, 8>;
    using H3 = Heights3D;
    constexpr int E = H3::E;
    static_assert(K::GE * 2 == H3::RECB && K::W == 49, "the 3D kinds' map and window");
    __shared__ __attribute__((aligned(16))) char lds_all[WPB * H3::WAVE_BYTES];
    const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
    const int i0 = __builtin_amdgcn_readfirstlane(((int)blockIdx.x * WPB + wv) * E);
    if (i0 >= a.m) return;
    const int nrec = min(E, a.m - i0);
    const bool active = lane < nrec;
    const int i = i0 + (active ? lane : 0);
    const H3 hm(lds_all + wv * H3::WAVE_BYTES, lane);
    const int srow = obs_row(a, i);
    const int sme = __shfl(srow, lane & (E - 1));                    // (lanes 32..63 shadow 0..31)
    Lane s;
    {
        const uint4 h = a.nodes[(size_t)sme * REC3_PIECES];
        s.unpack(make_int4((int)h.x, (int)h.y, (int)h.z, (int)h.w));
    }
    hm.gather(a.nodes, srow, nrec);
    int cellv[K::W];
    hm.window(s.r, s.c, cellv);
    const Slots v = scalar_slots<DYN>(s, a.total_step);
    auto cell = [&](int el) { return cellv[el]; };
    if constexpr (VEC) {
        asm volatile("" ::: "memory");
        emit_tile<OT, false>(hm.rec, (char*)a.obs + (size_t)i0 * K::D * sizeof(OT), lane, nrec, cell, v.v0, v.v1);
    } else if (active) {
        write_row<K::W>((OT*)a.obs + (size_t)i * K::D, cell, v);
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
