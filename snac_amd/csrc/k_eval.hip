// k_eval.hip -- default-policy evaluation of tree leaves IN PLACE on node pools: snac_evaluate_nodes{1,2,3}d
#include "nodes_dev.h"

// The "Evaluation" block of the vanilla MCTS procedure (script/MCTS/utils/mcts.py:100-110): from every new leaf, uniformly random steps
// until `done` or the horizon, `estimate += reward * gamma**t`.  On batch rows that is BatchedDMPEnv.evaluate: a fork of the leaves
// (a new batch, the plan table cloned), a rollout writing reward / done [H][m] to memory, then k_discount (k_misc.hip) over them.  Here
// one kernel does all of it on the pool's records:
//   prologue  every lane unpacks its leaf's header; the wave's E leaves' records are gathered into the kind's LDS image (K1D / K2D / K3D,
//             snac_dev.h) with the frame rebuilt, as the tile loaders do; 1D / 2D also stage each leaf's plan as load_plan does (3D reads
//             its one plan cell inside step()); then a barrier
//   loop      lane = leaf: the counter-RNG action of tick t0 + t, K::step (the rules of rules1d / rules2d / rules3d), and the sum in a
//             register, product and sum each rounded to float64 (fp contract off, as k_discount); gamma**t is a uniform load; no global
//             store; the wave leaves once none of its leaves is alive
//   epilogue  est and steps, one store each per leaf
// The pool is read only: no record changes, no auto-reset, no episodic sums.
namespace {

struct EvalArgs {
    const uint4* nodes;        // the pool's records
    const int32_t* node_rows;  // record of leaf i (NULL: i), clamped
    int32_t pool, m, H;
    const double* gpow;        // [H]
    double* est;               // [m] in / out
    int64_t* steps;            // [m] or NULL
};

// the wave's records -> the LDS image with its frame (and, 1D / 2D, the plans).  1D / 2D: lane = leaf, every load of the lane's record
// and plan row in flight at once (16-byte pieces), then its own columns of the image.  3D: 50 pieces of heights per leaf, spread over
// the wave in rounds of 13 loads per lane (a leaf per lane would hold 200 registers), after the whole image is set to frame.
template <class K>
__device__ __forceinline__ void load_image(uint32_t* lds, const KArgs& a, const EvalArgs& v, bool active, int nleaf, int row, int pidx, int lane) {
    constexpr int E = K::E;
    if constexpr (K::A == 3) {                                       // 1D: word e * 17 + j holds cells 2j - 2, 2j - 1 (frame: words 0, 16)
        if (!active) return;
        uint4 c[GRID_PIECES_1D], p[GRID_PIECES_1D];
        const uint4* const prow = (const uint4*)((const int16_t*)a.plans + (size_t)pidx * K::GE);
#pragma unroll
        for (int q = 0; q < GRID_PIECES_1D; ++q) { c[q] = v.nodes[(size_t)row * LINE_PIECES + REC_GRID_PIECE + q]; p[q] = prow[q]; }
        uint32_t* const h = lds + lane * (K::ES / 2);
        uint32_t* const pl = lds + K::P_OFF + lane * (K::ES / 2);
        h[0] = 0xFFFFFFFFu; h[16] = 0xFFFFFFFFu;
#pragma unroll
        for (int q = 0; q < GRID_PIECES_1D; ++q) {
            const uint32_t cw[4] = {c[q].x, c[q].y, c[q].z, c[q].w}, pw[4] = {p[q].x, p[q].y, p[q].z, p[q].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (q * 4 + j < 15) h[1 + q * 4 + j] = cw[j];        // (cells 30, 31 are pad: the frame stays there)
                pl[q * 4 + j] = pw[j];
            }
        }
    } else if constexpr (K::A == 5) {                                // 2D: C[(q + 3) * RS + e] = record row word q encoded, rows 0-2 / 23-25 frame
        if (!active) return;
        uint4 b[GRID_PIECES_2D], p[GRID_PIECES_2D];
        const uint4* const prow = (const uint4*)((const uint32_t*)a.plans + (size_t)pidx * K::GE);
#pragma unroll
        for (int q = 0; q < GRID_PIECES_2D; ++q) { b[q] = v.nodes[(size_t)row * LINE_PIECES + REC_GRID_PIECE + q]; p[q] = prow[q]; }
        uint64_t* const c = K::cells(lds) + lane;
#pragma unroll
        for (int q = 0; q < 3; ++q) { c[q * K::RS] = 0x000FFFFFFFFFFFFFull; c[(23 + q) * K::RS] = 0x000FFFFFFFFFFFFFull; }
#pragma unroll
        for (int q = 0; q < GRID_PIECES_2D; ++q) {
            const uint32_t bw[4] = {b[q].x, b[q].y, b[q].z, b[q].w}, pw[4] = {p[q].x, p[q].y, p[q].z, p[q].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[(q * 4 + j + 3) * K::RS] = K::encode_row(bw[j]);
                lds[K::P_OFF + (q * 4 + j) * K::RS + lane] = pw[j];
            }
        }
    } else {                                                         // 3D: H[e * 678 + (r + 3) * 26 + c + 3]
        static_assert((E * K::ES / 2) % 4 == 0, "the image is whole 16-byte pieces");
        for (int i = lane; i < E * K::ES / 8; i += 64) ((uint4*)lds)[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
        int16_t* const h = K::hmap(lds);
        constexpr int HP = GRID_PIECES_3D, R = 13;                   // 50 pieces of 8 cells per leaf; loads per lane per round
        for (int i0 = 0; i0 < nleaf * HP; i0 += 64 * R) {
            uint4 w[R];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int i = i0 + u * 64 + lane, e = min(i / HP, nleaf - 1), p = i - e * HP;
                const int re = __shfl(row, e);
                w[u] = i < nleaf * HP ? v.nodes[(size_t)re * REC3_PIECES + REC_GRID_PIECE + p] : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int i = i0 + u * 64 + lane, e = i / HP, p = i - e * HP;
                if (i < nleaf * HP) {
                    const uint32_t ww[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int cell = p * 8 + k, r = cell / 20, cc = cell - r * 20;
                        h[e * K::ES + (r + 3) * 26 + cc + 3] = (int16_t)((k & 1) ? (ww[k >> 1] >> 16) : (ww[k >> 1] & 0xffffu));
                    }
                }
            }
        }
    }
}

template <class K, int NP>
__global__ __launch_bounds__(64) void k_eval(const KArgs a, const EvalArgs v) {
    constexpr int E = K::E;
    const int lane = (int)threadIdx.x;
    const int leaf0 = (int)blockIdx.x * E;                           // one wave per block: leaf0 and nleaf are uniform
    const int nleaf = min(E, v.m - leaf0);
    const bool active = lane < nleaf;
    const int leaf = leaf0 + (active ? lane : 0);
    uint32_t* const lds = wave_lds<K, 1>();
    const int row = (int)row_of(v.node_rows, v.pool, leaf);
    Lane s;
    s.clear();
    {
        const uint4 h = v.nodes[(size_t)row * NP];                   // the leaf's header (piece 0 of its record)
        s.unpack(make_int4((int)h.x, (int)h.y, (int)h.z, (int)h.w));
    }
    double e = v.est[leaf];
    if (v.H > 0) load_image<K>(lds, a, v, active, nleaf, row, s.pidx, lane);
    __syncthreads();                                                 // the fill before any lane's own steps (one wave per block: the s_barrier
                                                                     // folds away, the workgroup fence -- lgkmcnt(0), no LDS access moved across -- stays)
    const EnvKeys sk = env_keys(a.key_step, (uint64_t)(a.env_id_base + leaf));
    bool alive = active && !(s.flags & SNAC_FLAG_NEED_RESET);
    long long n = 0;
    for (int t = 0; t < v.H; ++t) {
        if (!__any(alive)) break;
        const double g = v.gpow[t];                                  // t is uniform: one scalar load
        if (alive) {
            const uint32_t w = rng_word(sk, a.t0 + (uint32_t)t);
            const int act = draw_action<K::A>(w, a), k = 1 + (int)(((w & 0xffffu) * 3u) >> 16);
            int reward = 0;
            bool done = false;
            K::step(lds, a, s, act, k, a.ts_done, a.brick_gt, lane, reward, done);
            {
#pragma clang fp contract(off)                                      // no fma: the product and the sum each rounded, as the reference's python floats
                const double p = (double)(float)reward * g;
                e = e + p;
            }
            n += 1;
            alive = !done;
        }
    }
    if (active) {
        v.est[leaf] = e;
        if (v.steps) v.steps[leaf] = n;
    }
}

template <class K, int NP>
void launch_eval(const KArgs& a, const EvalArgs& v, hipStream_t s) {
    hipLaunchKernelGGL((k_eval<K, NP>), dim3((unsigned)((v.m + K::E - 1) / K::E)), dim3(64), 0, s, a, v);
}

// leaves per wave: 1D / 2D images are small (8.7 / 19 KB at 64 leaves), 3D's is 1356 bytes per leaf (87 KB at 64: one wave per CU)
template <template <bool, int> class KT, bool DYN, int NP>
void launch_kind(int E, const KArgs& a, const EvalArgs& v, hipStream_t s) {
    if (E == 16) launch_eval<KT<DYN, 16>, NP>(a, v, s);
    else if (E == 32) launch_eval<KT<DYN, 32>, NP>(a, v, s);
    else launch_eval<KT<DYN, 64>, NP>(a, v, s);
}

int evaluate_nodes(int kind, const char* name, const snac_env_desc* d, const snac_state* st, const void* nodes, int32_t pool_rows, int32_t m,
                   const int32_t* node_rows, int32_t H, uint32_t t0, const double* gpow, double* est, int64_t* steps, void* stream) {
    using namespace snac_detail;
    if (int rc = nodes_check(kind, d, st, nodes, pool_rows, m)) return rc;
    if (H < 0) return fail(SNAC_ERR_ARG, "H must be >= 0");
    if (!node_rows && m > pool_rows) return fail(SNAC_ERR_ARG, "m exceeds the pool");
    if (!est && m > 0) return fail(SNAC_ERR_ARG, "null est");
    if (!gpow && H > 0) return fail(SNAC_ERR_ARG, "null gpow");
    if (m == 0) return SNAC_OK;
    KArgs a = make_args(d, st);
    a.t0 = t0;
    const EvalArgs v{(const uint4*)nodes, node_rows, pool_rows, m, H, gpow, est, steps};
    const bool dyn = d->dynamic != 0;
    hipStream_t s = (hipStream_t)stream;
    g_kernel = "k_eval";
    if (kind == SNAC_ENV_1D) {
        const int E = tune(TN_EVAL_E);
        dyn ? launch_kind<K1D, true, LINE_PIECES>(E, a, v, s) : launch_kind<K1D, false, LINE_PIECES>(E, a, v, s);
    } else if (kind == SNAC_ENV_2D) {
        const int E = tune(TN_EVAL_E);
        dyn ? launch_kind<K2D, true, LINE_PIECES>(E, a, v, s) : launch_kind<K2D, false, LINE_PIECES>(E, a, v, s);
    } else {
        const int E = tune(TN_EVAL3D_E);
        dyn ? launch_kind<K3D, true, REC3_PIECES>(E, a, v, s) : launch_kind<K3D, false, REC3_PIECES>(E, a, v, s);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SNAC_OK : fail_hip(e, name);
}

}  // namespace

extern "C" {

int snac_evaluate_nodes1d(const snac_env_desc* d, const snac_state* st, const snac_node1d* nodes, int32_t pool_rows, int32_t m, const int32_t* node_rows,
                          int32_t H, uint32_t t0, const double* gpow, double* est, int64_t* steps, void* stream) {
    return evaluate_nodes(SNAC_ENV_1D, "snac_evaluate_nodes1d", d, st, nodes, pool_rows, m, node_rows, H, t0, gpow, est, steps, stream);
}

int snac_evaluate_nodes2d(const snac_env_desc* d, const snac_state* st, const snac_node2d* nodes, int32_t pool_rows, int32_t m, const int32_t* node_rows,
                          int32_t H, uint32_t t0, const double* gpow, double* est, int64_t* steps, void* stream) {
    return evaluate_nodes(SNAC_ENV_2D, "snac_evaluate_nodes2d", d, st, nodes, pool_rows, m, node_rows, H, t0, gpow, est, steps, stream);
}

int snac_evaluate_nodes3d(const snac_env_desc* d, const snac_state* st, const snac_node3d* nodes, int32_t pool_rows, int32_t m, const int32_t* node_rows,
                          int32_t H, uint32_t t0, const double* gpow, double* est, int64_t* steps, void* stream) {
    return evaluate_nodes(SNAC_ENV_3D, "snac_evaluate_nodes3d", d, st, nodes, pool_rows, m, node_rows, H, t0, gpow, est, steps, stream);
}

}  // extern "C"
