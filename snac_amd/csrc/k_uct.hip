// k_uct.hip -- UCT selection, backup and re-rooting over node pools: snac_uct_select / snac_uct_backup / snac_uct_advance, and the
// K-paths-per-tree iteration snac_uct_select_paths / snac_uct_backup_paths, and PUCT: snac_uct_select_puct / snac_uct_set_priors
// and their q_normalise forms snac_uct_select_paths_norm / snac_uct_select_puct_norm / snac_uct_backup_paths_norm with snac_uct_bounds,
// and the Gumbel root rule on top of the normalised PUCT selection, snac_uct_select_gumbel, with the Gumbel rule below the root as well,
// snac_uct_select_gumbel_interior / snac_uct_set_priors_value / snac_uct_improved_policy
// (include/snac_hip.h has the semantics)
#include <cmath>
#include <cstddef>
#include <type_traits>

#include "snac_units.h"
#include "snac_tune.h"
#include "uct_dev.h"

// lane = tree: both kernels are chains of dependent loads, one trip per tree level.  A node's record holds its children's rows, visits
// and values (line 0) beside its own header (line 1), so a selection step reads one record: the pieces it compares and the node's own
// header are all issued before the first is used.  The backup reads the parent's header (one trip) and writes the node's own N / W and
// their mirror in the parent.  The kernels depend on A (num_actions) only, not on the env kind.  Spreading the trees thinner (8, 16 or
// 64 lanes per wave with one working) measured no faster: a level costs a dependent trip whatever the wave holds (profiles/r10_uct.txt).
namespace {

struct UctSel {
    uint4* stats;
    int32_t B, cap;
    double c;
    const double* ltab;
    const double* rtab;
    int32_t tlen;
    int32_t* used;
    int32_t* src;
    int32_t* dst;
    int8_t* action;
    int32_t* leaf;
    uint8_t* expanded;
    float* r_leaf;
};

struct UctBack {
    uint4* stats;
    int32_t B, cap;
    double gamma;
    const int32_t* src;
    const int8_t* action;
    const int32_t* leaf;
    const uint8_t* expanded;
    const float* reward;
    const uint8_t* done;
    const double* est;
};

template <int A>
__global__ __launch_bounds__(64) void k_uct_select(const UctSel v) {
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= v.B) return;
    const int base = b * v.cap;
    int used = v.used[b];
    int n = base, leaf = base, act = 0;
    bool expanded = false;
    float r = 0.f;
    for (int depth = 0; depth < v.cap; ++depth) {                    // bounded: a corrupted tree cannot keep the wave spinning
        NodePieces<A, false> p;
        p.load(v.stats + (size_t)n * PIECES);
        leaf = n;
        r = __uint_as_float(p.own.z);
        if (p.hdr.z != 0u) break;                                    // terminal
        int child[A], cn[A];
        double cw[A];
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const uint4 c4 = p.pc[a / 4], n4 = p.pn[a / 4], w2 = p.pw[a / 2];
            const int j = a % 4;
            child[a] = (int)word_of(c4, j);
            cn[a] = (int)word_of(n4, j);
            cw[a] = (a % 2 == 0) ? f64(w2.x, w2.y) : f64(w2.z, w2.w);
        }
        int untried = -1;
#pragma unroll
        for (int a = A - 1; a >= 0; --a)
            if (child[a] < 0) untried = a;
        if (untried >= 0 && used < v.cap) {                          // expand the lowest untried action into the tree's next row
            const int row = base + used;
            used += 1;
            reinterpret_cast<int32_t*>(v.stats + (size_t)n * PIECES)[untried] = row;
            v.src[b] = n;
            leaf = row;
            act = untried;
            expanded = true;
            break;
        }
        const double lg = v.ltab[min(max((int)p.hdr.w, 0), v.tlen - 1)];
        int best = -1;
        double bu = 0.0;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            if (child[a] < 0) continue;
            double u;
            {
#pragma clang fp contract(off)                                      // no fma: U rounded step by step, as a host restatement computes it
                const double q = cw[a] / (double)cn[a];
                const double e = lg * v.rtab[min(max(cn[a], 0), v.tlen - 1)];
                u = q + v.c * e;
            }
            if (best < 0 || u > bu) { best = a; bu = u; }
        }
        if (best < 0) break;                                         // no children and the budget spent
        n = clamp_row(child[best], base, v.cap);
    }
    if (!expanded) v.src[b] = leaf;
    v.dst[b] = expanded ? leaf : v.B * v.cap + b;
    v.action[b] = (int8_t)act;
    v.leaf[b] = leaf;
    v.expanded[b] = expanded ? 1 : 0;
    v.r_leaf[b] = expanded ? 0.f : r;
    v.used[b] = used;
}

template <int A>
__global__ __launch_bounds__(64) void k_uct_backup(const UctBack v) {
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= v.B) return;
    const int base = b * v.cap;
    int x = clamp_row(v.leaf[b], base, v.cap);
    double g = v.est[b];
    int parent, action, visits;
    double w;
    if (v.expanded[b]) {                                             // the new node's row, whole: no children, no visits yet
        parent = clamp_row(v.src[b], base, v.cap);
        action = v.action[b];
        visits = 0;
        w = 0.0;
        uint4* const rec = v.stats + (size_t)x * PIECES;
        const uint4 none = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu), zero = make_uint4(0u, 0u, 0u, 0u);
        rec[P_CHILD] = none;
        rec[P_CHILD + 1] = none;
#pragma unroll
        for (int q = P_VISITS; q < P_HDR; ++q) rec[q] = zero;
        rec[P_HDR] = make_uint4((uint32_t)parent, (uint32_t)action, v.done[b] ? 1u : 0u, 0u);
        rec[P_OWN] = make_uint4(0u, 0u, __float_as_uint(v.reward[b]), 0u);
#pragma unroll
        for (int q = P_OWN + 1; q < PIECES; ++q) rec[q] = zero;
    } else {
        const uint4* const rec = v.stats + (size_t)x * PIECES;
        const uint4 hdr = rec[P_HDR], own = rec[P_OWN];
        parent = (int)hdr.x;
        action = (int)hdr.y;
        visits = (int)hdr.w;
        w = f64(own.x, own.y);
    }
    for (int depth = 0; depth < v.cap; ++depth) {                    // leaf .. root, bounded as the selection
        int32_t* const own = reinterpret_cast<int32_t*>(v.stats + (size_t)x * PIECES);
        visits += 1;
        {
#pragma clang fp contract(off)
            w = w + g;
        }
        own[W_VISITS] = visits;
        *reinterpret_cast<double*>(own + W_VALUE_SUM) = w;
        if (parent < 0) break;
        const int p = clamp_row(parent, base, v.cap);
        const int a = min(max(action, 0), A - 1);
        uint4* const prec = v.stats + (size_t)p * PIECES;
        const uint4 hdr = prec[P_HDR], pown = prec[P_OWN];
        int32_t* const pw = reinterpret_cast<int32_t*>(prec);
        pw[W_CHILD_VISITS + a] = visits;                             // the mirror in the parent's line 0
        *reinterpret_cast<double*>(pw + W_CHILD_VALUE + 2 * a) = w;
        {
#pragma clang fp contract(off)
            const double t = v.gamma * g;
            g = (double)__uint_as_float(pown.z) + t;
        }
        x = p;
        parent = (int)hdr.x;
        action = (int)hdr.y;
        visits = (int)hdr.w;
        w = f64(pown.x, pown.y);
    }
}

struct UctAdv {
    uint4* stats;
    uint4* records;
    int32_t B, cap;
    const int8_t* actions;
    const float* edge_reward;
    const uint8_t* edge_done;
    int32_t* used;
    int32_t* work;
    float* reward_out;
    uint8_t* done_out;
};

constexpr int ADV_ROWS = 32;                                         // new rows per move chunk

// a kept node's child or parent row -> its new row; -1 (untried) and anything outside the kept rows read as -1
__device__ __forceinline__ uint32_t remap(uint32_t r, const int32_t* o2n, int c, int end, int base) {
    const int x = (int)r;
    if (x < c || x >= end) return 0xFFFFFFFFu;
    const int k = o2n[x - base];
    return k < 0 ? 0xFFFFFFFFu : (uint32_t)(base + k);
}

// workgroup = tree.  Walk: a lane per candidate row, in chunks of 256 rows from c up; a walk follows parents only while they stay in
// its own chunk, since every row below the chunk already has its kept flag (its old -> new entry in `work`).  Scan: ballots and
// popcounts per wave, the four wave counts through LDS.  Move: ADV_ROWS new rows per chunk, each thread holding its 16-byte pieces of
// the chunk's source rows (stats row, then record) in registers across one barrier.  Compaction keeps the old order, so a chunk's
// stores land at or below its sources, and no chunk reads a row an earlier chunk wrote: the move is safe in place.
template <int A, int RP>                                             // RP: 16-byte pieces of a node record (8: 1D / 2D, 56: 3D)
__global__ __launch_bounds__(256) void k_uct_advance(const UctAdv v) {
    constexpr int P = PIECES + RP, PER = ADV_ROWS * P / 256;
    static_assert(ADV_ROWS * P % 256 == 0, "whole pieces per thread");
    __shared__ int wave_kept[4];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = v.cap, base = b * cap;
    const uint4* const root = v.stats + (size_t)base * PIECES;
    const uint4 hdr = root[P_HDR];
    const int a = min(max((int)v.actions[b], 0), A - 1);
    const int ch = reinterpret_cast<const int32_t*>(root)[a];
    const int used = min(max(v.used[b], 1), cap);
    __syncthreads();                                                 // every read of the root before the untried case rewrites it
    if (hdr.z != 0u) {                                               // terminal root: nothing changes
        if (tid == 0) {
            v.reward_out[b] = 0.f;
            v.done_out[b] = 1;
        }
        return;
    }
    if (ch < 0) {                                                    // untried: the edge's record alone, fresh statistics
        const bool done = v.edge_done[b] != 0;
        if (tid < RP) {
            v.records[(size_t)base * RP + tid] = v.records[(size_t)(v.B * cap + b) * RP + tid];
        } else if (tid >= 64 && tid < 64 + PIECES) {
            const int q = tid - 64;
            const uint4 none = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu), zero = make_uint4(0u, 0u, 0u, 0u);
            v.stats[(size_t)base * PIECES + q] =
                q < P_VISITS ? none : q == P_HDR ? make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, done ? 1u : 0u, 0u) : zero;
        }
        if (tid == 0) {
            v.used[b] = 1;
            v.reward_out[b] = v.edge_reward[b];
            v.done_out[b] = done ? 1 : 0;
        }
        return;
    }
    const int c = clamp_row(ch, base, cap), end = base + used;
    const uint4 cown = v.stats[(size_t)c * PIECES + P_OWN], chdr = v.stats[(size_t)c * PIECES + P_HDR];
    int32_t* const o2n = v.work + (size_t)b * 2 * cap;               // old row - base -> new index (-1: dropped), rows [c, end) only
    int32_t* const n2o = o2n + cap;                                  // new index -> old row
    int kept = 0;
    for (int s = c; s < end; s += 256) {
        const int i = s + tid;
        bool keep = false;
        if (i < end) {
            int x = i;
            for (int d = 0; d < cap && x >= s && x > c; ++d)         // bounded, as select and backup
                x = clamp_row(reinterpret_cast<const int32_t*>(v.stats + (size_t)x * PIECES)[W_PARENT], base, cap);
            keep = x == c || (x > c && x < s && o2n[x - base] >= 0);
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_kept[wave] = __popcll(m);
        __syncthreads();
        int before = kept + __popcll(m & ((1ull << lane) - 1ull)), total = kept;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int n = wave_kept[w];
            before += w < wave ? n : 0;
            total += n;
        }
        if (i < end) {
            o2n[i - base] = keep ? before : -1;
            if (keep) n2o[before] = i;
        }
        kept = total;
        __syncthreads();                                             // the chunk's flags before the next chunk's walks; LDS reuse
    }
    for (int j0 = 0; j0 < kept; j0 += ADV_ROWS) {
        uint4 val[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int q = k * 256 + tid, j = j0 + q / P, p = q % P;
            if (j >= kept) continue;
            const int o = n2o[j];
            uint4 x = p < PIECES ? v.stats[(size_t)o * PIECES + p] : v.records[(size_t)o * RP + (p - PIECES)];
            if (p < P_VISITS) {
                x.x = remap(x.x, o2n, c, end, base);
                x.y = remap(x.y, o2n, c, end, base);
                x.z = remap(x.z, o2n, c, end, base);
                x.w = remap(x.w, o2n, c, end, base);
            } else if (p == P_HDR) {
                x.x = j == 0 ? 0xFFFFFFFFu : remap(x.x, o2n, c, end, base);
                x.y = j == 0 ? 0xFFFFFFFFu : x.y;
            } else if (p == P_OWN && j == 0) {
                x.z = 0u;                                            // a root's reward
            }
            val[k] = x;
        }
        __syncthreads();                                             // every load of the chunk before any of its stores
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int q = k * 256 + tid, j = j0 + q / P, p = q % P;
            if (j >= kept) continue;
            if (p < PIECES) v.stats[(size_t)(base + j) * PIECES + p] = val[k];
            else v.records[(size_t)(base + j) * RP + (p - PIECES)] = val[k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        v.used[b] = kept;
        v.reward_out[b] = __uint_as_float(cown.z);
        v.done_out[b] = chdr.z != 0u ? 1 : 0;
    }
}

// ---- K paths per tree and iteration (virtual loss) ----------------------------------------------------------------------------------
// lane = tree, its K paths one after the other: path k + 1 reads the in-flight counts path k left, so a tree is one serial chain and
// every word a path reads back was stored by the same lane.  The in-flight count P of child a of node n is n's zero[1 + a] (pieces
// P_FLY, P_FLY + 1), incremented on the way down and cleared by the backup; a node's own count is that entry of its parent, carried
// down in a register, and the root's is the path index k.  A fresh row (>= base + used on entry) has no record and no header yet; its
// word W_SLOT (zero[0]) holds the slot that expanded it until the backup writes the row whole.
// The argument blocks: each form's is the one before it plus its own members (single inheritance: no base here has tail padding that a
// member could move into, so every kernarg layout is the one the nested structs had; static_asserts below pin them).
struct UctSelPaths : UctSel {
    int32_t K;
    double vl;
    int32_t* first_slot;
};

struct UctBackPaths : UctBack {
    int32_t K;
};

// Normalised q ("Normalised q" in include/snac_hip.h): the NORM forms take the same arguments and the bounds array, bounds[2 * b] = lo,
// bounds[2 * b + 1] = hi of tree b.  A selection reads its tree's pair once, before the descent (one 16-byte load that no level waits
// for), and a tried child's q becomes (q - lo) / (hi - lo) where hi > lo; the backup folds W / N of every node below the root into
// the pair, which it keeps in registers over its K walks and stores once.  NORM = false is the code of the unnormalised kernels.
struct UctSelPathsNorm : UctSelPaths {
    const double* bounds;
};

struct UctBackPathsNorm : UctBackPaths {
    double* bounds;
};

// tree b's pair as it enters U: on = hi > lo, lo and span = hi - lo (computed once per tree)
struct QRange {
    double lo, span;
    bool on;
};

__device__ __forceinline__ QRange q_range(const double* bounds, int b) {
    const double2 p = reinterpret_cast<const double2*>(bounds)[b];
    QRange r{p.x, 0.0, p.y > p.x};
    {
#pragma clang fp contract(off)
        r.span = p.y - p.x;
    }
    return r;
}

__device__ __forceinline__ double q_norm(double q, const QRange& r) {
#pragma clang fp contract(off)
    const double d = q - r.lo;
    return r.on ? d / r.span : q;
}

template <int A, bool NORM>
__global__ __launch_bounds__(64) void k_uct_select_paths(const std::conditional_t<NORM, UctSelPathsNorm, UctSelPaths> v) {
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= v.B) return;
    const int base = b * v.cap, K = v.K;
    QRange qr{0.0, 0.0, false};
    if constexpr (NORM) qr = q_range(v.bounds, b);
    const int used0 = v.used[b];
    const int fresh = base + used0;                                  // rows from here up are made by this launch
    int used = used0;
    for (int k = 0; k < K; ++k) {
        const int s = b * K + k;
        int n = base, leaf = base, act = 0, src = base, first = -1, fly = k;   // fly: earlier paths through n
        bool expanded = false;
        float r = 0.f;
        for (int depth = 0; depth < v.cap; ++depth) {
            NodePieces<A, true> p;
            p.load(v.stats + (size_t)n * PIECES);
            leaf = src = n;
            r = __uint_as_float(p.own.z);
            if (p.hdr.z != 0u) break;                                // terminal
            int child[A], cn[A], cf[A];
            double cw[A];
#pragma unroll
            for (int a = 0; a < A; ++a) {
                const uint4 c4 = p.pc[a / 4], n4 = p.pn[a / 4], f4 = p.pf[a / 4], w2 = p.pw[a / 2];
                const int j = a % 4;
                child[a] = (int)word_of(c4, j);
                cn[a] = (int)word_of(n4, j);
                cf[a] = (int)word_of(f4, j);
                cw[a] = (a % 2 == 0) ? f64(w2.x, w2.y) : f64(w2.z, w2.w);
            }
            int untried = -1;
#pragma unroll
            for (int a = A - 1; a >= 0; --a)
                if (child[a] < 0) untried = a;
            int32_t* const words = reinterpret_cast<int32_t*>(v.stats + (size_t)n * PIECES);
            if (untried >= 0 && used < v.cap) {                      // expand the lowest untried action into the tree's next row
                leaf = expand_path(words, v.stats, untried, base, used, s);
                act = untried;
                expanded = true;
                first = s;
                break;
            }
            const double lg = v.ltab[min(max((int)p.hdr.w + fly, 0), v.tlen - 1)];
            int best = -1, bf = 0;
            double bu = 0.0;
#pragma unroll
            for (int a = 0; a < A; ++a) {
                if (child[a] < 0) continue;
                double u;
                {
#pragma clang fp contract(off)
                    const int np = cn[a] + cf[a];
                    double q = (cw[a] - v.vl * (double)cf[a]) / (double)np;
                    if constexpr (NORM) q = q_norm(q, qr);
                    const double e = lg * v.rtab[min(max(np, 0), v.tlen - 1)];
                    u = q + v.c * e;
                }
                if (best < 0 || u > bu) { best = a; bu = u; bf = cf[a]; }
            }
            if (best < 0) break;                                     // no children and the budget spent
            words[W_FLY + best] = bf + 1;
            fly = bf;
            n = clamp_row(child[best], base, v.cap);
            if (n >= fresh) {                                        // made by an earlier path of this launch: stop on it
                leaf = n;
                src = base;                                          // the row is another edge's destination: step the root instead
                r = 0.f;
                first = fresh_row_slot(v.stats, n);
                break;
            }
        }
        v.src[s] = src;
        v.dst[s] = expanded ? leaf : v.B * v.cap + s;
        v.action[s] = (int8_t)act;
        v.leaf[s] = leaf;
        v.expanded[s] = expanded ? 1 : 0;
        v.r_leaf[s] = expanded ? 0.f : r;
        v.first_slot[s] = first;
    }
    v.used[b] = used;
}

template <int A, bool NORM>
__global__ __launch_bounds__(64) void k_uct_backup_paths(const std::conditional_t<NORM, UctBackPathsNorm, UctBackPaths> v) {
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= v.B) return;
    const int base = b * v.cap, K = v.K;
    double2 range = make_double2(0.0, 0.0);                          // NORM: the tree's (lo, hi), in registers over the K walks
    if constexpr (NORM) range = reinterpret_cast<const double2*>(v.bounds)[b];
    for (int k = 0; k < K; ++k) {                                    // the new nodes' rows, whole, before any walk reads one
        const int s = b * K + k;
        if (!v.expanded[s]) continue;
        uint4* const rec = v.stats + (size_t)clamp_row(v.leaf[s], base, v.cap) * PIECES;
        const uint4 none = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu), zero = make_uint4(0u, 0u, 0u, 0u);
        rec[P_CHILD] = none;
        rec[P_CHILD + 1] = none;
#pragma unroll
        for (int q = P_VISITS; q < P_HDR; ++q) rec[q] = zero;
        rec[P_HDR] = make_uint4((uint32_t)clamp_row(v.src[s], base, v.cap), (uint32_t)v.action[s], v.done[s] ? 1u : 0u, 0u);
        rec[P_OWN] = make_uint4(0u, 0u, __float_as_uint(v.reward[s]), 0u);
#pragma unroll
        for (int q = P_OWN + 1; q < PIECES; ++q) rec[q] = zero;
    }
    for (int k = 0; k < K; ++k) {                                    // the walks, in slot order: shared ancestors add in that order
        const int s = b * K + k;
        int x = clamp_row(v.leaf[s], base, v.cap);
        double g = v.est[s];
        const uint4* const rec = v.stats + (size_t)x * PIECES;
        uint4 hdr = rec[P_HDR], own = rec[P_OWN];
        for (int depth = 0; depth < v.cap; ++depth) {                // leaf .. root, bounded as the selection
            int32_t* const me = reinterpret_cast<int32_t*>(v.stats + (size_t)x * PIECES);
            const int visits = (int)hdr.w + 1;
            double sum;
            {
#pragma clang fp contract(off)
                sum = f64(own.x, own.y) + g;
            }
            me[W_VISITS] = visits;
            *reinterpret_cast<double*>(me + W_VALUE_SUM) = sum;
            const int parent = (int)hdr.x;
            if (parent < 0) break;
            const int p = clamp_row(parent, base, v.cap);
            const int a = min(max((int)hdr.y, 0), A - 1);
            uint4* const prec = v.stats + (size_t)p * PIECES;
            hdr = prec[P_HDR];
            own = prec[P_OWN];
            int32_t* const pw = reinterpret_cast<int32_t*>(prec);
            pw[W_CHILD_VISITS + a] = visits;                         // the mirror in the parent's line 0
            *reinterpret_cast<double*>(pw + W_CHILD_VALUE + 2 * a) = sum;
            pw[W_FLY + a] = 0;                                   // the edge's in-flight count
            if constexpr (NORM) {                                    // x is below the root: its mean is one that selection compares
                const double m = sum / (double)visits;
                range.x = m < range.x ? m : range.x;                 // a NaN fails both comparisons
                range.y = m > range.y ? m : range.y;
            }
            {
#pragma clang fp contract(off)
                const double t = v.gamma * g;
                g = (double)__uint_as_float(own.z) + t;
            }
            x = p;
        }
    }
    if constexpr (NORM) reinterpret_cast<double2*>(v.bounds)[b] = range;
}

// ---- PUCT: a policy / value network in place of UCB1 and the rollout ----------------------------------------------------------------
// k_uct_select_paths with another rule at a stored, non-terminal node: every action has a score, tried or not,
//     U = q + c * ((prior[a] * sqrt_table[N(n) + P(n)]) * inv_table[Np]),   q = (W_a - vl * P_a) / Np tried, first_play_value untried,
// and the best one is expanded or descended.  The priors are words 48-55 of the record (pieces P_PRIOR ..): two more pieces of line 1,
// issued with the others before the first is used; the chain of dependent loads per level is the one of k_uct_select_paths.
struct UctSelPuct : UctSelPaths {                                    // ltab / rtab: sqrt_table / inv_table
    double fpv;
};

struct UctSelPuctNorm : UctSelPuct {
    const double* bounds;
};

// Gumbel root ("Gumbel root" in include/snac_hip.h): the GUMBEL form is the NORM form with another rule at the ROOT of a tree whose
// candidate mask cand[b] is not zero: path k takes the ((offset + k) mod M)-th of the M candidates, in integers, and no U is computed
// there.  The mask is one 4-byte load beside the bounds pair, before the descent.  A tree with cand[b] == 0, and every level below a
// root, runs the NORM code.
struct UctSelGumbel : UctSelPuctNorm {
    const int32_t* cand;
    int32_t offset;
};

// Gumbel interior ("Gumbel interior" in include/snac_hip.h): the INTERIOR form is the GUMBEL form with another rule at every node that
// is not a root taking a candidate's turn: the action with the largest pi'(a) - (N_a + P_a) / (1 + sum N + sum P), pi' the improved policy
// of the node (gumbel_policy below).  No U is computed in this form.  The node's network value is words 56-57 of its record, the first
// half of piece P_NETV: one more piece of line 1, issued with the others before the first is used.
struct UctSelGumbelInterior : UctSelGumbel {
    double c_visit, c_scale;
};

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"                // a derived struct is not standard-layout; its offsets are what is pinned
static_assert(sizeof(UctSel) == 104 && offsetof(UctSelPaths, K) == 104 && offsetof(UctSelPaths, vl) == 112 &&
                  offsetof(UctSelPaths, first_slot) == 120 && sizeof(UctSelPaths) == 128 && offsetof(UctSelPathsNorm, bounds) == 128 &&
                  sizeof(UctSelPathsNorm) == 136,
              "the kernarg layouts of the selections");
static_assert(offsetof(UctSelPuct, fpv) == 128 && sizeof(UctSelPuct) == 136 && offsetof(UctSelPuctNorm, bounds) == 136 &&
                  sizeof(UctSelPuctNorm) == 144 && offsetof(UctSelGumbel, cand) == 144 && offsetof(UctSelGumbel, offset) == 152 &&
                  sizeof(UctSelGumbel) == 160 && offsetof(UctSelGumbelInterior, c_visit) == 160 &&
                  offsetof(UctSelGumbelInterior, c_scale) == 168 && sizeof(UctSelGumbelInterior) == 176,
              "the kernarg layouts of the PUCT selections");
static_assert(sizeof(UctBack) == 80 && offsetof(UctBackPaths, K) == 80 && sizeof(UctBackPaths) == 88 &&
                  offsetof(UctBackPathsNorm, bounds) == 88 && sizeof(UctBackPathsNorm) == 96,
              "the kernarg layouts of the backups");
#pragma clang diagnostic pop

template <bool NORM, bool GUMBEL, bool INTERIOR>
using UctSelPuctArg = std::conditional_t<INTERIOR, UctSelGumbelInterior,
                                         std::conditional_t<GUMBEL, UctSelGumbel, std::conditional_t<NORM, UctSelPuctNorm, UctSelPuct>>>;

// exp(x) for x <= 0 from float64 + - *, floor and ldexp alone, so that python floats reproduce it bit for bit: 0 for a NaN and below
// -700, x > 0 reads as 0; x = k ln 2 + r with k = floor(x log2(e) + 0.5) and ln 2 split in two so that k * LN2_HI is exact; the
// Taylor sum of exp(r) to r^13 / 13! (|r| <= 0.35: the remainder is below 4e-18) by Horner's rule; ldexp(sum, k).  Within 1 ulp of exp.
constexpr double UCT_EXP_LOG2E = 0x1.71547652b82fep+0, UCT_EXP_LN2_HI = 0x1.62e42fee00000p-1, UCT_EXP_LN2_LO = 0x1.a39ef35793c76p-33;
constexpr int UCT_EXP_TERMS = 14;
__device__ constexpr double UCT_EXP_COEF[UCT_EXP_TERMS] = {1.0 / 1.0,        1.0 / 1.0,         1.0 / 2.0,          1.0 / 6.0,         1.0 / 24.0,
                                                           1.0 / 120.0,      1.0 / 720.0,       1.0 / 5040.0,       1.0 / 40320.0,     1.0 / 362880.0,
                                                           1.0 / 3628800.0,  1.0 / 39916800.0,  1.0 / 479001600.0,  1.0 / 6227020800.0};

__device__ __forceinline__ double uct_exp(double x) {
#pragma clang fp contract(off)
    if (!(x >= -700.0)) return 0.0;                                  // a NaN too
    x = x > 0.0 ? 0.0 : x;
    const double t = x * UCT_EXP_LOG2E;
    const double k = floor(t + 0.5);
    const double hi = k * UCT_EXP_LN2_HI, lo = k * UCT_EXP_LN2_LO;
    const double r = (x - hi) - lo;
    double p = UCT_EXP_COEF[UCT_EXP_TERMS - 1];
#pragma unroll
    for (int i = UCT_EXP_TERMS - 2; i >= 0; --i) {
        const double pr = p * r;
        p = pr + UCT_EXP_COEF[i];
    }
    return ldexp(p, (int)k);
}

// a node's line-0 words and priors out of their pieces (pf: the in-flight counts' pieces, or nullptr: every P = 0)
template <int A>
__device__ __forceinline__ void node_actions(const uint4* pc, const uint4* pn, const uint4* pf, const uint4* pp, const uint4* pw, int (&child)[A],
                                             int (&cn)[A], int (&cf)[A], float (&pr)[A], double (&cw)[A]) {
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const uint4 c4 = pc[a / 4], n4 = pn[a / 4], p4 = pp[a / 4], w2 = pw[a / 2];
        const int j = a % 4;
        child[a] = (int)word_of(c4, j);
        cn[a] = (int)word_of(n4, j);
        cf[a] = 0;
        if (pf) {
            const uint4 f4 = pf[a / 4];
            cf[a] = (int)word_of(f4, j);
        }
        pr[a] = __uint_as_float(word_of(p4, j));
        cw[a] = (a % 2 == 0) ? f64(w2.x, w2.y) : f64(w2.z, w2.w);
    }
}

// The improved policy pi' of a node ("Gumbel interior" in include/snac_hip.h, whose order of operations this is): softmax of log prior +
// sigma(completed q), the q of an action without a visited child completed by v_mix, which mixes the node's network value `netv` with
// the prior-weighted mean of the visited children's q.  np[a] = N_a + P_a and total = sum N + sum P are what selection subtracts.
// TABLE: 1 / (1 + sum N) from inv_table (index clamped), else computed -- the same float64 wherever the index is inside the table.
template <int A, bool TABLE>
__device__ __forceinline__ void gumbel_policy(const int (&child)[A], const int (&cn)[A], const int (&cf)[A], const float (&pr)[A],
                                              const double (&cw)[A], double netv, const QRange& qr, double c_visit, double c_scale,
                                              const double* itab, int tlen, double (&pi)[A], int (&np)[A], int& total) {
#pragma clang fp contract(off)
    int N[A], sum_n = 0, sum_p = 0, max_n = 0;
    bool vis[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const bool has = child[a] >= 0;
        const int P = has ? cf[a] : 0;
        N[a] = has ? max(cn[a], 0) : 0;
        vis[a] = has && N[a] > 0;
        sum_n += N[a];
        sum_p += P;
        max_n = max(max_n, N[a]);
        np[a] = N[a] + P;
    }
    total = sum_n + sum_p;
    double q[A], sp = 0.0, spq = 0.0, sw = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        q[a] = 0.0;
        if (vis[a]) {
            const double p = (double)pr[a];
            q[a] = cw[a] / (double)N[a];
            const double pq = p * q[a];
            sp = sp + p;
            spq = spq + pq;
            sw = sw + cw[a];
        }
    }
    double vmix = netv;
    if (sum_n != 0) {
        const double n = (double)sum_n;
        const double mean = sp > 0.0 ? spq / sp : sw / n;
        const double nm = n * mean;
        const double num = netv + nm;
        double inv;
        if constexpr (TABLE) inv = itab[min(max(sum_n, 0), tlen - 1)];
        else inv = 1.0 / (1.0 + n);
        vmix = num * inv;
    }
    const double s1 = c_visit + (double)max_n;
    const double s2 = s1 * c_scale;
    double sig[A], smax = -INFINITY;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const double qh = q_norm(vis[a] ? q[a] : vmix, qr);
        sig[a] = s2 * qh;
        smax = sig[a] > smax ? sig[a] : smax;                        // a NaN never wins
    }
    double e[A], z = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const double d = sig[a] - smax;
        e[a] = (double)pr[a] * uct_exp(d);
        z = z + e[a];
    }
#pragma unroll
    for (int a = 0; a < A; ++a) pi[a] = z > 0.0 ? e[a] / z : 0.0;
}

// NORM: a tried child's q normalised (first_play_value is used as given); GUMBEL (with NORM): the candidates' turn at the root;
// INTERIOR (with GUMBEL): the improved policy's rule in place of U everywhere else
template <int A, bool NORM, bool GUMBEL = false, bool INTERIOR = false>
__global__ __launch_bounds__(64) void k_uct_select_puct(const UctSelPuctArg<NORM, GUMBEL, INTERIOR> v) {
    static_assert(NORM || !GUMBEL, "the Gumbel form extends the normalised one");
    static_assert(GUMBEL || !INTERIOR, "the interior form extends the Gumbel one");
    constexpr int CI = (A + 3) / 4, CW = (A + 1) / 2;
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= v.B) return;
    const int base = b * v.cap, K = v.K;
    QRange qr{0.0, 0.0, false};
    if constexpr (NORM) qr = q_range(v.bounds, b);
    [[maybe_unused]] int cmask = 0, cnum = 1;                        // GUMBEL: the tree's candidates and their number
    if constexpr (GUMBEL) {
        cmask = v.cand[b] & ((1 << A) - 1);
        cnum = max(__popc((unsigned)cmask), 1);
    }
    const int used0 = v.used[b];
    const int fresh = base + used0;                                  // rows from here up are made by this launch
    int used = used0;
    for (int k = 0; k < K; ++k) {
        const int s = b * K + k;
        int n = base, leaf = base, act = 0, src = base, first = -1, fly = k;   // fly: earlier paths through n
        bool expanded = false;
        float r = 0.f;
        for (int depth = 0; depth < v.cap; ++depth) {
            const uint4* const rec = v.stats + (size_t)n * PIECES;
            uint4 pc[CI], pn[CI], pf[CI], pp[CI], pw[CW];
#pragma unroll
            for (int q = 0; q < CI; ++q) { pc[q] = rec[P_CHILD + q]; pn[q] = rec[P_VISITS + q]; pf[q] = rec[P_FLY + q]; pp[q] = rec[P_PRIOR + q]; }
#pragma unroll
            for (int q = 0; q < CW; ++q) pw[q] = rec[P_VALUE + q];
            const uint4 hdr = rec[P_HDR], own = rec[P_OWN];
            [[maybe_unused]] uint4 pv = make_uint4(0u, 0u, 0u, 0u);  // INTERIOR: the node's network value
            if constexpr (INTERIOR) pv = rec[P_NETV];
            leaf = src = n;
            r = __uint_as_float(own.z);
            if (hdr.z != 0u) break;                                  // terminal
            [[maybe_unused]] const double sq = INTERIOR ? 0.0 : v.ltab[min(max((int)hdr.w + fly, 0), v.tlen - 1)];
            int best = -1, bf = 0, tried = -1, tf = 0, bchild = -1, tchild = -1;
            double bu = 0.0, tu = 0.0;
            [[maybe_unused]] int turn = -1;                          // GUMBEL, a root with candidates: the action whose turn it is
            if constexpr (GUMBEL) {
                if (depth == 0 && cmask != 0) {
                    int skip = (v.offset + k) % cnum;
#pragma unroll
                    for (int a = A - 1; a >= 0; --a) turn = (cmask >> a & 1) && __popc((unsigned)cmask & ((1u << a) - 1u)) == skip ? a : turn;
                }
            }
            [[maybe_unused]] double score[A] = {};                   // INTERIOR: pi'(a) - (N_a + P_a) / (1 + sum N + sum P), in place of U
            // The rule needs sums over every action before any score, so INTERIOR unpacks the pieces here (node_actions) and the shared loop
            // below unpacks child / visits / in-flight once more, with pr and cw it does not use: deliberate.  The loop stays the one the
            // other forms compile (their instruction streams are unchanged), and the compiler folds the repeated selects of the same registers.
            // Its selects are spelled out, and this kernel loads its own pieces: with word_of or NodePieces (uct_dev.h) several forms' listings move.
            if constexpr (INTERIOR) {
                if (turn < 0) {
                    int ch[A], cn[A], cf[A], np[A], total;
                    float pr[A];
                    double cw[A], pi[A];
                    node_actions<A>(pc, pn, pf, pp, pw, ch, cn, cf, pr, cw);
                    gumbel_policy<A, true>(ch, cn, cf, pr, cw, f64(pv.x, pv.y), qr, v.c_visit, v.c_scale, v.rtab, v.tlen, pi, np, total);
                    const double inv = v.rtab[min(max(total, 0), v.tlen - 1)];
#pragma unroll
                    for (int a = 0; a < A; ++a) {
#pragma clang fp contract(off)
                        const double t = (double)np[a] * inv;
                        score[a] = pi[a] - t;
                    }
                }
            }
#pragma unroll
            for (int a = 0; a < A; ++a) {
                const uint4 c4 = pc[a / 4], n4 = pn[a / 4], f4 = pf[a / 4], p4 = pp[a / 4], w2 = pw[a / 2];
                const int j = a % 4;
                const int child = (int)(j == 0 ? c4.x : j == 1 ? c4.y : j == 2 ? c4.z : c4.w);
                const int cn = (int)(j == 0 ? n4.x : j == 1 ? n4.y : j == 2 ? n4.z : n4.w);
                const int cf = (int)(j == 0 ? f4.x : j == 1 ? f4.y : j == 2 ? f4.z : f4.w);
                if constexpr (GUMBEL) {
                    if (turn >= 0) {                                 // no U: the action is given; untried with the budget spent stops here
                        if (a == turn) { best = a; bf = cf; bchild = child; }
                        continue;
                    }
                }
                const float pr = __uint_as_float(j == 0 ? p4.x : j == 1 ? p4.y : j == 2 ? p4.z : p4.w);
                const double cw = (a % 2 == 0) ? f64(w2.x, w2.y) : f64(w2.z, w2.w);
                const bool has = child >= 0;
                double u;
                if constexpr (INTERIOR) {
                    u = score[a];
                } else {
#pragma clang fp contract(off)                                      // no fma: U rounded step by step, as a host restatement computes it
                    const int np = has ? cn + cf : 0;
                    const double t = v.vl * (double)cf;
                    double q = has ? (cw - t) / (double)np : v.fpv;
                    if constexpr (NORM) q = has ? q_norm(q, qr) : q;
                    const double e0 = (double)pr * sq;
                    const double e = e0 * v.rtab[min(max(np, 0), v.tlen - 1)];
                    const double ce = v.c * e;
                    u = q + ce;
                }
                if (best < 0 || u > bu) { best = a; bu = u; bf = cf; bchild = child; }
                if (has && (tried < 0 || u > tu)) { tried = a; tu = u; tf = cf; tchild = child; }
            }
            int32_t* const words = reinterpret_cast<int32_t*>(v.stats + (size_t)n * PIECES);
            if (bchild < 0) {                                        // the best action is untried
                if (used < v.cap) {                                  // expand it into the tree's next row
                    leaf = expand_path(words, v.stats, best, base, used, s);
                    act = best;
                    expanded = true;
                    first = s;
                    break;
                }
                if (tried < 0) break;                                // no children and the budget spent
                best = tried; bf = tf; bchild = tchild;              // the budget spent: the best of the tried children
            }
            words[W_FLY + best] = bf + 1;
            fly = bf;
            n = clamp_row(bchild, base, v.cap);
            if (n >= fresh) {                                        // made by an earlier path of this launch: stop on it
                leaf = n;
                src = base;                                          // the row is another edge's destination: step the root instead
                r = 0.f;
                first = fresh_row_slot(v.stats, n);
                break;
            }
        }
        v.src[s] = src;
        v.dst[s] = expanded ? leaf : v.B * v.cap + s;
        v.action[s] = (int8_t)act;
        v.leaf[s] = leaf;
        v.expanded[s] = expanded ? 1 : 0;
        v.r_leaf[s] = expanded ? 0.f : r;
        v.first_slot[s] = first;
    }
    v.used[b] = used;
}

// priors into nodes: thread = node, the node's 32-byte span (pieces P_PRIOR, P_PRIOR + 1) as two 16-byte stores; a row outside the
// array is skipped.  VALUE: the node's net_value (words 56-57) too, as one 8-byte store, loaded before the first store.
template <int A, bool VALUE>
__device__ __forceinline__ void set_priors(uint4* stats, int32_t stats_rows, int32_t m, const int32_t* rows, const float* priors,
                                           const double* value, int only_unvisited) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= m) return;
    const int row = rows[i];
    if (row < 0 || row >= stats_rows) return;
    uint4* const rec = stats + (size_t)row * PIECES;
    if (only_unvisited && rec[P_HDR].w != 0u) return;
    uint32_t p[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) p[a] = a < A ? __float_as_uint(priors[(size_t)i * A + a]) : 0u;
    [[maybe_unused]] double nv = 0.0;
    if constexpr (VALUE) nv = value[i];
    rec[P_PRIOR] = make_uint4(p[0], p[1], p[2], p[3]);
    rec[P_PRIOR + 1] = make_uint4(p[4], p[5], p[6], p[7]);
    if constexpr (VALUE) *reinterpret_cast<double*>(rec + P_NETV) = nv;
}

template <int A>
__global__ __launch_bounds__(256) void k_uct_set_priors(uint4* stats, int32_t stats_rows, int32_t m, const int32_t* rows, const float* priors,
                                                        int only_unvisited) {
    set_priors<A, false>(stats, stats_rows, m, rows, priors, nullptr, only_unvisited);
}

template <int A>
__global__ __launch_bounds__(256) void k_uct_set_priors_value(uint4* stats, int32_t stats_rows, int32_t m, const int32_t* rows, const float* priors,
                                                              const double* value, int only_unvisited) {
    set_priors<A, true>(stats, stats_rows, m, rows, priors, value, only_unvisited);
}

// the improved policy of m nodes: thread = node, the statistics read only; the node's six kinds of pieces are all issued before the
// first is used; gumbel_policy with every P = 0; a row outside the trees or a terminal node gives zeros
struct UctImproved {
    const uint4* stats;
    int32_t B, cap, m;
    const int32_t* rows;
    double c_visit, c_scale;
    const double* bounds;
    float* pi;
};

template <int A>
__global__ __launch_bounds__(64) void k_uct_improved_policy(const UctImproved v) {
    constexpr int CI = (A + 3) / 4, CW = (A + 1) / 2;
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= v.m) return;
    const int row = v.rows[i];
    float out[A];
#pragma unroll
    for (int a = 0; a < A; ++a) out[a] = 0.f;
    if (row >= 0 && row < v.B * v.cap) {
        const uint4* const rec = v.stats + (size_t)row * PIECES;
        uint4 pc[CI], pn[CI], pp[CI], pw[CW];
#pragma unroll
        for (int q = 0; q < CI; ++q) { pc[q] = rec[P_CHILD + q]; pn[q] = rec[P_VISITS + q]; pp[q] = rec[P_PRIOR + q]; }
#pragma unroll
        for (int q = 0; q < CW; ++q) pw[q] = rec[P_VALUE + q];
        const uint4 hdr = rec[P_HDR], pv = rec[P_NETV];
        const QRange qr = q_range(v.bounds, row / v.cap);
        if (hdr.z == 0u) {
            int ch[A], cn[A], cf[A], np[A], total;
            float pr[A];
            double cw[A], pi[A];
            node_actions<A>(pc, pn, nullptr, pp, pw, ch, cn, cf, pr, cw);
            gumbel_policy<A, false>(ch, cn, cf, pr, cw, f64(pv.x, pv.y), qr, v.c_visit, v.c_scale, nullptr, 0, pi, np, total);
#pragma unroll
            for (int a = 0; a < A; ++a) out[a] = (float)pi[a];
        }
    }
#pragma unroll
    for (int a = 0; a < A; ++a) v.pi[(size_t)i * A + a] = out[a];
}

// ---- bounds from a tree as it stands ----------------------------------------------------------------------------------------------------
// G lanes = tree, 64 / G trees per one-wave workgroup: the lanes stride over the tree's rows below `used`, each row one 32-byte read of
// line 1 (P_HDR: visits, P_OWN: W), BOUNDS_ROWS rows in flight per lane; then min / max by < / > through the group's lanes (exact, so
// the result does not depend on G) and one 16-byte store per tree.  A tree with mask[b] == 0 is neither read nor written.
struct UctBounds {
    const uint4* stats;
    int32_t B, cap;
    const int32_t* used;
    const uint8_t* mask;
    double* bounds;
};

constexpr int BOUNDS_ROWS = 8;

template <int G>
__global__ __launch_bounds__(64) void k_uct_bounds(const UctBounds v) {
    const int lane = (int)threadIdx.x, g = lane % G;
    const int b = (int)blockIdx.x * (64 / G) + lane / G;
    const bool live = b < v.B && (!v.mask || v.mask[b] != 0);
    double lo = INFINITY, hi = -INFINITY;
    if (live) {
        const int used = min(max(v.used[b], 1), v.cap);
        const uint4* const tree = v.stats + (size_t)b * v.cap * PIECES;
        for (int j0 = 1 + g; j0 < used; j0 += G * BOUNDS_ROWS) {
            uint4 hdr[BOUNDS_ROWS], own[BOUNDS_ROWS];
#pragma unroll
            for (int i = 0; i < BOUNDS_ROWS; ++i) {                  // every load of the batch before the first is used
                const int j = min(j0 + i * G, used - 1);
                hdr[i] = tree[(size_t)j * PIECES + P_HDR];
                own[i] = tree[(size_t)j * PIECES + P_OWN];
            }
#pragma unroll
            for (int i = 0; i < BOUNDS_ROWS; ++i) {
                const int n = (int)hdr[i].w;
                if (j0 + i * G >= used || n <= 0) continue;
                const double m = f64(own[i].x, own[i].y) / (double)n;
                lo = m < lo ? m : lo;                                // a NaN fails both comparisons
                hi = m > hi ? m : hi;
            }
        }
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {                            // every lane of the wave takes part; a group's lanes are neighbours
        const double l = __shfl_xor(lo, o), h = __shfl_xor(hi, o);
        lo = l < lo ? l : lo;
        hi = h > hi ? h : hi;
    }
    if (live && g == 0) reinterpret_cast<double2*>(v.bounds)[b] = make_double2(lo, hi);
}

// lanes per tree of k_uct_bounds: about four rows per lane for small trees, a whole wave from 129 rows on (SNAC_UCT_BOUNDS_WIDTH forces one)
int bounds_width(int cap) {
    const int forced = snac_detail::tune(snac_detail::TN_UCT_BOUNDS_WIDTH);
    if (forced == 8 || forced == 16 || forced == 32 || forced == 64) return forced;
    return cap > 128 ? 64 : cap > 64 ? 32 : cap > 32 ? 16 : 8;
}

int actions_check(int A) { return A != 3 && A != 5 && A != 8 ? fail(SNAC_ERR_ARG, "num_actions must be 3, 5 or 8") : SNAC_OK; }

// the statistics array against B trees of cap rows: one slot and one scratch row per tree, or with `paths` (K paths per tree) B * K
// slots and B * (cap + K) rows
int uct_check_rows(const void* stats, int32_t rows, int32_t B, int32_t cap, const int32_t* paths = nullptr) {
    using namespace snac_detail;
    if (!stats) return fail(SNAC_ERR_ARG, "null stats");
    if (B < 1) return fail(SNAC_ERR_ARG, "B must be >= 1");
    if (cap < 1) return fail(SNAC_ERR_ARG, "cap must be >= 1");
    if (paths && *paths < 1) return fail(SNAC_ERR_ARG, "paths must be >= 1");
    if (paths && (long long)B * (long long)*paths > 0x7FFFFFFFll) return fail(SNAC_ERR_ARG, "B * paths slots exceed int32");
    const long long need = (long long)B * ((long long)cap + (paths ? (long long)*paths : 1));
    if (need > 0x7FFFFFFFll) return fail(SNAC_ERR_ARG, paths ? "B * (cap + paths) rows exceed int32" : "B * (cap + 1) rows exceed int32");
    if (need > rows) return fail(SNAC_ERR_ARG, paths ? "B * (cap + paths) rows exceed stats_rows" : "B * (cap + 1) rows exceed stats_rows");
    if (((uintptr_t)stats & 127) != 0) return fail(SNAC_ERR_ARG, "stats must be 128-byte aligned (records of whole lines)");
    return SNAC_OK;
}

int uct_check(int A, const void* stats, int32_t rows, int32_t B, int32_t cap) {
    if (int rc = actions_check(A)) return rc;
    return uct_check_rows(stats, rows, B, cap);
}

int uct_check_paths(int A, const void* stats, int32_t rows, int32_t B, int32_t cap, int32_t K) {
    if (int rc = actions_check(A)) return rc;
    return uct_check_rows(stats, rows, B, cap, &K);
}

int bounds_check(const void* bounds) {
    using namespace snac_detail;
    if (!bounds) return fail(SNAC_ERR_ARG, "null bounds");
    if (((uintptr_t)bounds & 15) != 0) return fail(SNAC_ERR_ARG, "bounds must be 16-byte aligned (a tree's pair is one piece)");
    return SNAC_OK;
}

// what the K-paths selections check after their scalars: the two tables (null_tables: the message that names them), the per-slot
// arrays, and with `norm` the bounds
int select_check(const UctSelPaths& v, const char* null_tables, bool norm, const double* bounds) {
    using namespace snac_detail;
    if (!v.ltab || !v.rtab) return fail(SNAC_ERR_ARG, null_tables);
    if (v.tlen < 2) return fail(SNAC_ERR_ARG, "table_len must be >= 2");
    if (!v.used || !v.src || !v.dst || !v.action || !v.leaf || !v.expanded || !v.r_leaf || !v.first_slot)
        return fail(SNAC_ERR_ARG, "null per-slot array (used / src / dst / action / leaf / expanded / r_leaf / first_slot)");
    return norm ? bounds_check(bounds) : SNAC_OK;
}

// what snac_uct_set_priors and snac_uct_set_priors_value check alike
int set_priors_check(int A, const void* stats, int32_t stats_rows, int32_t m, const int32_t* rows, const float* priors) {
    using namespace snac_detail;
    if (int rc = actions_check(A)) return rc;
    if (!stats) return fail(SNAC_ERR_ARG, "null stats");
    if (stats_rows < 1) return fail(SNAC_ERR_ARG, "stats_rows must be >= 1");
    if (m < 0) return fail(SNAC_ERR_ARG, "m must be >= 0");
    if (((uintptr_t)stats & 127) != 0) return fail(SNAC_ERR_ARG, "stats must be 128-byte aligned (records of whole lines)");
    if (!rows || !priors) return fail(SNAC_ERR_ARG, "null rows / priors");
    return SNAC_OK;
}

}  // namespace

extern "C" {

int snac_uct_select(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, double c, const double* log_table,
                    const double* rsqrt_table, int32_t table_len, int32_t* used, int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf,
                    uint8_t* expanded, float* r_leaf, void* stream) {
    using namespace snac_detail;
    if (int rc = uct_check(num_actions, stats, stats_rows, B, cap)) return rc;
    if (!log_table || !rsqrt_table) return fail(SNAC_ERR_ARG, "null log_table / rsqrt_table");
    if (table_len < 2) return fail(SNAC_ERR_ARG, "table_len must be >= 2");
    if (!used || !src || !dst || !action || !leaf || !expanded || !r_leaf)
        return fail(SNAC_ERR_ARG, "null per-tree array (used / src / dst / action / leaf / expanded / r_leaf)");
    const UctSel v{(uint4*)stats, B, cap, c, log_table, rsqrt_table, table_len, used, src, dst, action, leaf, expanded, r_leaf};
    g_kernel = "k_uct_select";
    return by_actions(num_actions, [&](auto k) {
        hipLaunchKernelGGL((k_uct_select<decltype(k)::value>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, v);
        return launched("snac_uct_select");
    });
}

int snac_uct_backup(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, double gamma, const int32_t* src,
                    const int8_t* action, const int32_t* leaf, const uint8_t* expanded, const float* reward, const uint8_t* done,
                    const double* est, void* stream) {
    using namespace snac_detail;
    if (int rc = uct_check(num_actions, stats, stats_rows, B, cap)) return rc;
    if (!src || !action || !leaf || !expanded || !reward || !done || !est)
        return fail(SNAC_ERR_ARG, "null per-tree array (src / action / leaf / expanded / reward / done / est)");
    const UctBack v{(uint4*)stats, B, cap, gamma, src, action, leaf, expanded, reward, done, est};
    g_kernel = "k_uct_backup";
    return by_actions(num_actions, [&](auto k) {
        hipLaunchKernelGGL((k_uct_backup<decltype(k)::value>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, v);
        return launched("snac_uct_backup");
    });
}

int snac_uct_advance(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, void* records, int32_t record_bytes,
                     int32_t record_rows, const int8_t* actions, const float* edge_reward, const uint8_t* edge_done, int32_t* used,
                     int32_t* work, float* reward_out, uint8_t* done_out, void* stream) {
    using namespace snac_detail;
    if (int rc = uct_check(num_actions, stats, stats_rows, B, cap)) return rc;
    if (!records) return fail(SNAC_ERR_ARG, "null records");
    if (((uintptr_t)records & 127) != 0) return fail(SNAC_ERR_ARG, "records must be 128-byte aligned");
    if (record_bytes != 128 && record_bytes != 896) return fail(SNAC_ERR_ARG, "record_bytes must be 128 or 896");
    if ((long long)B * ((long long)cap + 1) > record_rows) return fail(SNAC_ERR_ARG, "B * (cap + 1) rows exceed record_rows");
    if (!actions || !edge_reward || !edge_done || !used || !reward_out || !done_out)
        return fail(SNAC_ERR_ARG, "null per-tree array (actions / edge_reward / edge_done / used / reward_out / done_out)");
    if (!work) return fail(SNAC_ERR_ARG, "null work");
    const UctAdv v{(uint4*)stats, (uint4*)records, B, cap, actions, edge_reward, edge_done, used, work, reward_out, done_out};
    g_kernel = "k_uct_advance";
    return by_actions(num_actions, [&](auto k) {
        constexpr int A = decltype(k)::value;
        if (record_bytes == 128) hipLaunchKernelGGL((k_uct_advance<A, 8>), dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, v);
        else hipLaunchKernelGGL((k_uct_advance<A, 56>), dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, v);
        return launched("snac_uct_advance");
    });
}

// the plain and the _norm entry points share their checks and launches: bounds == nullptr is the plain form
static int select_paths(const char* name, int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths,
                        double c, double virtual_loss, const double* log_table, const double* rsqrt_table, int32_t table_len, int32_t* used,
                        int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf, uint8_t* expanded, float* r_leaf, int32_t* first_slot,
                        bool norm, const double* bounds, void* stream) {
    using namespace snac_detail;
    if (int rc = uct_check_paths(num_actions, stats, stats_rows, B, cap, paths)) return rc;
    if (!std::isfinite(virtual_loss)) return fail(SNAC_ERR_ARG, "virtual_loss must be finite");
    const UctSelPaths v{{(uint4*)stats, B, cap, c, log_table, rsqrt_table, table_len, used, src, dst, action, leaf, expanded, r_leaf},
                        paths, virtual_loss, first_slot};
    if (int rc = select_check(v, "null log_table / rsqrt_table", norm, bounds)) return rc;
    const dim3 grid((unsigned)((B + 63) / 64));
    g_kernel = "k_uct_select_paths";
    return by_actions(num_actions, [&](auto k) {
        constexpr int A = decltype(k)::value;
        if (norm) hipLaunchKernelGGL((k_uct_select_paths<A, true>), grid, dim3(64), 0, (hipStream_t)stream, UctSelPathsNorm{v, bounds});
        else hipLaunchKernelGGL((k_uct_select_paths<A, false>), grid, dim3(64), 0, (hipStream_t)stream, v);
        return launched(name);
    });
}

int snac_uct_select_paths(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double c,
                          double virtual_loss, const double* log_table, const double* rsqrt_table, int32_t table_len, int32_t* used,
                          int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf, uint8_t* expanded, float* r_leaf, int32_t* first_slot,
                          void* stream) {
    return select_paths("snac_uct_select_paths", num_actions, stats, stats_rows, B, cap, paths, c, virtual_loss, log_table, rsqrt_table, table_len,
                        used, src, dst, action, leaf, expanded, r_leaf, first_slot, false, nullptr, stream);
}

int snac_uct_select_paths_norm(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double c,
                               double virtual_loss, const double* log_table, const double* rsqrt_table, int32_t table_len, int32_t* used,
                               int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf, uint8_t* expanded, float* r_leaf,
                               int32_t* first_slot, const double* bounds, void* stream) {
    return select_paths("snac_uct_select_paths_norm", num_actions, stats, stats_rows, B, cap, paths, c, virtual_loss, log_table, rsqrt_table,
                        table_len, used, src, dst, action, leaf, expanded, r_leaf, first_slot, true, bounds, stream);
}

static int backup_paths(const char* name, int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths,
                        double gamma, const int32_t* src, const int8_t* action, const int32_t* leaf, const uint8_t* expanded, const float* reward,
                        const uint8_t* done, const double* est, bool norm, double* bounds, void* stream) {
    using namespace snac_detail;
    if (int rc = uct_check_paths(num_actions, stats, stats_rows, B, cap, paths)) return rc;
    if (!src || !action || !leaf || !expanded || !reward || !done || !est)
        return fail(SNAC_ERR_ARG, "null per-slot array (src / action / leaf / expanded / reward / done / est)");
    if (norm)
        if (int rc = bounds_check(bounds)) return rc;
    const UctBackPaths v{{(uint4*)stats, B, cap, gamma, src, action, leaf, expanded, reward, done, est}, paths};
    const dim3 grid((unsigned)((B + 63) / 64));
    g_kernel = "k_uct_backup_paths";
    return by_actions(num_actions, [&](auto k) {
        constexpr int A = decltype(k)::value;
        if (norm) hipLaunchKernelGGL((k_uct_backup_paths<A, true>), grid, dim3(64), 0, (hipStream_t)stream, UctBackPathsNorm{v, bounds});
        else hipLaunchKernelGGL((k_uct_backup_paths<A, false>), grid, dim3(64), 0, (hipStream_t)stream, v);
        return launched(name);
    });
}

int snac_uct_backup_paths(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double gamma,
                          const int32_t* src, const int8_t* action, const int32_t* leaf, const uint8_t* expanded, const float* reward,
                          const uint8_t* done, const double* est, void* stream) {
    return backup_paths("snac_uct_backup_paths", num_actions, stats, stats_rows, B, cap, paths, gamma, src, action, leaf, expanded, reward, done,
                        est, false, nullptr, stream);
}

int snac_uct_backup_paths_norm(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double gamma,
                               const int32_t* src, const int8_t* action, const int32_t* leaf, const uint8_t* expanded, const float* reward,
                               const uint8_t* done, const double* est, double* bounds, void* stream) {
    return backup_paths("snac_uct_backup_paths_norm", num_actions, stats, stats_rows, B, cap, paths, gamma, src, action, leaf, expanded, reward,
                        done, est, true, bounds, stream);
}

static int select_puct(const char* name, int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths,
                       double c, double virtual_loss, double first_play_value, const double* sqrt_table, const double* inv_table,
                       int32_t table_len, int32_t* used, int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf, uint8_t* expanded,
                       float* r_leaf, int32_t* first_slot, bool norm, const double* bounds, bool gumbel, const int32_t* cand, int32_t offset,
                       bool interior, double c_visit, double c_scale, void* stream) {
    using namespace snac_detail;
    if (int rc = uct_check_paths(num_actions, stats, stats_rows, B, cap, paths)) return rc;
    if (!std::isfinite(virtual_loss)) return fail(SNAC_ERR_ARG, "virtual_loss must be finite");
    if (!std::isfinite(first_play_value)) return fail(SNAC_ERR_ARG, "first_play_value must be finite");
    const UctSelPuct v{{{(uint4*)stats, B, cap, c, sqrt_table, inv_table, table_len, used, src, dst, action, leaf, expanded, r_leaf},
                        paths, virtual_loss, first_slot},
                       first_play_value};
    if (int rc = select_check(v, "null sqrt_table / inv_table", norm, bounds)) return rc;
    if (gumbel) {
        if (!cand) return fail(SNAC_ERR_ARG, "null cand");
        if (offset < 0) return fail(SNAC_ERR_ARG, "offset must be >= 0");
        if ((long long)offset + (long long)paths > 0x7FFFFFFFll) return fail(SNAC_ERR_ARG, "offset + paths exceeds int32");
    }
    if (interior && (!std::isfinite(c_visit) || !std::isfinite(c_scale))) return fail(SNAC_ERR_ARG, "c_visit and c_scale must be finite");
    const dim3 grid((unsigned)((B + 63) / 64));
    g_kernel = "k_uct_select_puct";
    return by_actions(num_actions, [&](auto k) {
        constexpr int A = decltype(k)::value;
        if (interior)
            hipLaunchKernelGGL((k_uct_select_puct<A, true, true, true>), grid, dim3(64), 0, (hipStream_t)stream,
                               UctSelGumbelInterior{{{v, bounds}, cand, offset}, c_visit, c_scale});
        else if (cand) hipLaunchKernelGGL((k_uct_select_puct<A, true, true>), grid, dim3(64), 0, (hipStream_t)stream, UctSelGumbel{{v, bounds}, cand, offset});
        else if (norm) hipLaunchKernelGGL((k_uct_select_puct<A, true>), grid, dim3(64), 0, (hipStream_t)stream, UctSelPuctNorm{v, bounds});
        else hipLaunchKernelGGL((k_uct_select_puct<A, false>), grid, dim3(64), 0, (hipStream_t)stream, v);
        return launched(name);
    });
}

int snac_uct_select_puct(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double c,
                         double virtual_loss, double first_play_value, const double* sqrt_table, const double* inv_table, int32_t table_len,
                         int32_t* used, int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf, uint8_t* expanded, float* r_leaf,
                         int32_t* first_slot, void* stream) {
    return select_puct("snac_uct_select_puct", num_actions, stats, stats_rows, B, cap, paths, c, virtual_loss, first_play_value, sqrt_table,
                       inv_table, table_len, used, src, dst, action, leaf, expanded, r_leaf, first_slot, false, nullptr, false, nullptr, 0, false, 0.0, 0.0,
                       stream);
}

int snac_uct_select_puct_norm(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double c,
                              double virtual_loss, double first_play_value, const double* sqrt_table, const double* inv_table,
                              int32_t table_len, int32_t* used, int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf, uint8_t* expanded,
                              float* r_leaf, int32_t* first_slot, const double* bounds, void* stream) {
    return select_puct("snac_uct_select_puct_norm", num_actions, stats, stats_rows, B, cap, paths, c, virtual_loss, first_play_value, sqrt_table,
                       inv_table, table_len, used, src, dst, action, leaf, expanded, r_leaf, first_slot, true, bounds, false, nullptr, 0, false, 0.0, 0.0,
                       stream);
}

int snac_uct_select_gumbel(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double c,
                           double virtual_loss, double first_play_value, const double* sqrt_table, const double* inv_table, int32_t table_len,
                           int32_t* used, int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf, uint8_t* expanded, float* r_leaf,
                           int32_t* first_slot, const double* bounds, const int32_t* cand, int32_t offset, void* stream) {
    return select_puct("snac_uct_select_gumbel", num_actions, stats, stats_rows, B, cap, paths, c, virtual_loss, first_play_value, sqrt_table,
                       inv_table, table_len, used, src, dst, action, leaf, expanded, r_leaf, first_slot, true, bounds, true, cand, offset, false, 0.0, 0.0,
                       stream);
}

int snac_uct_select_gumbel_interior(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t paths, double c,
                                    double virtual_loss, double first_play_value, const double* sqrt_table, const double* inv_table,
                                    int32_t table_len, int32_t* used, int32_t* src, int32_t* dst, int8_t* action, int32_t* leaf,
                                    uint8_t* expanded, float* r_leaf, int32_t* first_slot, const double* bounds, const int32_t* cand,
                                    int32_t offset, double c_visit, double c_scale, void* stream) {
    return select_puct("snac_uct_select_gumbel_interior", num_actions, stats, stats_rows, B, cap, paths, c, virtual_loss, first_play_value,
                       sqrt_table, inv_table, table_len, used, src, dst, action, leaf, expanded, r_leaf, first_slot, true, bounds, true, cand,
                       offset, true, c_visit, c_scale, stream);
}

int snac_uct_set_priors(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t m, const int32_t* rows, const float* priors,
                        int32_t only_unvisited, void* stream) {
    using namespace snac_detail;
    if (int rc = set_priors_check(num_actions, stats, stats_rows, m, rows, priors)) return rc;
    if (m == 0) return SNAC_OK;
    g_kernel = "k_uct_set_priors";
    return by_actions(num_actions, [&](auto k) {
        hipLaunchKernelGGL((k_uct_set_priors<decltype(k)::value>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint4*)stats,
                           stats_rows, m, rows, priors, only_unvisited != 0 ? 1 : 0);
        return launched("snac_uct_set_priors");
    });
}

int snac_uct_set_priors_value(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t m, const int32_t* rows, const float* priors,
                              const double* value, int32_t only_unvisited, void* stream) {
    using namespace snac_detail;
    if (int rc = set_priors_check(num_actions, stats, stats_rows, m, rows, priors)) return rc;
    if (!value) return fail(SNAC_ERR_ARG, "null value");
    if (m == 0) return SNAC_OK;
    g_kernel = "k_uct_set_priors_value";
    return by_actions(num_actions, [&](auto k) {
        hipLaunchKernelGGL((k_uct_set_priors_value<decltype(k)::value>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (uint4*)stats, stats_rows, m, rows, priors, value, only_unvisited != 0 ? 1 : 0);
        return launched("snac_uct_set_priors_value");
    });
}

int snac_uct_improved_policy(int32_t num_actions, const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, int32_t m,
                             const int32_t* rows, double c_visit, double c_scale, const double* bounds, float* pi, void* stream) {
    using namespace snac_detail;
    if (int rc = uct_check(num_actions, stats, stats_rows, B, cap)) return rc;
    if (m < 0) return fail(SNAC_ERR_ARG, "m must be >= 0");
    if (!rows) return fail(SNAC_ERR_ARG, "null rows");
    if (!std::isfinite(c_visit) || !std::isfinite(c_scale)) return fail(SNAC_ERR_ARG, "c_visit and c_scale must be finite");
    if (int rc = bounds_check(bounds)) return rc;
    if (!pi) return fail(SNAC_ERR_ARG, "null pi");
    if (m == 0) return SNAC_OK;
    const UctImproved v{(const uint4*)stats, B, cap, m, rows, c_visit, c_scale, bounds, pi};
    g_kernel = "k_uct_improved_policy";
    return by_actions(num_actions, [&](auto k) {
        hipLaunchKernelGGL((k_uct_improved_policy<decltype(k)::value>), dim3((unsigned)((m + 63) / 64)), dim3(64), 0, (hipStream_t)stream, v);
        return launched("snac_uct_improved_policy");
    });
}

int snac_uct_bounds(const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, const int32_t* used, const uint8_t* mask,
                    double* bounds, void* stream) {
    using namespace snac_detail;
    if (!used) return fail(SNAC_ERR_ARG, "null used");
    if (int rc = uct_check_rows(stats, stats_rows, B, cap)) return rc;
    if (int rc = bounds_check(bounds)) return rc;
    const UctBounds v{(const uint4*)stats, B, cap, used, mask, bounds};
    const int G = bounds_width(cap), per = 64 / G;
    const dim3 grid((unsigned)((B + per - 1) / per));
    g_kernel = "k_uct_bounds";
    if (G == 8) hipLaunchKernelGGL((k_uct_bounds<8>), grid, dim3(64), 0, (hipStream_t)stream, v);
    else if (G == 16) hipLaunchKernelGGL((k_uct_bounds<16>), grid, dim3(64), 0, (hipStream_t)stream, v);
    else if (G == 32) hipLaunchKernelGGL((k_uct_bounds<32>), grid, dim3(64), 0, (hipStream_t)stream, v);
    else hipLaunchKernelGGL((k_uct_bounds<64>), grid, dim3(64), 0, (hipStream_t)stream, v);
    return launched("snac_uct_bounds");
}

}  // extern "C"
