// k_uct.hip -- UCT selection and backup over node pools: snac_uct_select / snac_uct_backup (include/snac_hip.h has the semantics)
#include <cstddef>

#include "snac_dev.h"

// lane = tree: both kernels are chains of dependent loads, one trip per tree level.  A node's record holds its children's rows, visits
// and values (line 0) beside its own header (line 1), so a selection step reads one record: the pieces it compares and the node's own
// header are all issued before the first is used.  The backup reads the parent's header (one trip) and writes the node's own N / W and
// their mirror in the parent.  The kernels depend on A (num_actions) only, not on the env kind.  Spreading the trees thinner (8, 16 or
// 64 lanes per wave with one working) measured no faster: a level costs a dependent trip whatever the wave holds (profiles/r10_uct.txt).
namespace {

static_assert(sizeof(snac_uct_node) == 256, "snac_uct_node is two lines");
static_assert(offsetof(snac_uct_node, child_value) == 64 && offsetof(snac_uct_node, parent) == 128 && offsetof(snac_uct_node, value_sum) == 144 &&
                  offsetof(snac_uct_node, reward) == 152,
              "the piece map below");

constexpr int PIECES = 16;                                           // 16-byte pieces per record
constexpr int P_CHILD = 0, P_VISITS = 2, P_VALUE = 4, P_HDR = 8, P_OWN = 9;

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

__device__ __forceinline__ double f64(uint32_t lo, uint32_t hi) { return __hiloint2double((int)hi, (int)lo); }

__device__ __forceinline__ int clamp_row(int r, int base, int cap) { return min(max(r, base), base + cap - 1); }

template <int A>
__global__ __launch_bounds__(64) void k_uct_select(const UctSel v) {
    constexpr int CI = (A + 3) / 4, CW = (A + 1) / 2;                // pieces of child / child_visits, of child_value
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= v.B) return;
    const int base = b * v.cap;
    int used = v.used[b];
    int n = base, leaf = base, act = 0;
    bool expanded = false;
    float r = 0.f;
    for (int depth = 0; depth < v.cap; ++depth) {                    // bounded: a corrupted tree cannot keep the wave spinning
        const uint4* const rec = v.stats + (size_t)n * PIECES;
        uint4 pc[CI], pn[CI], pw[CW];
#pragma unroll
        for (int q = 0; q < CI; ++q) { pc[q] = rec[P_CHILD + q]; pn[q] = rec[P_VISITS + q]; }
#pragma unroll
        for (int q = 0; q < CW; ++q) pw[q] = rec[P_VALUE + q];
        const uint4 hdr = rec[P_HDR], own = rec[P_OWN];
        leaf = n;
        r = __uint_as_float(own.z);
        if (hdr.z != 0u) break;                                      // terminal
        int child[A], cn[A];
        double cw[A];
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const uint4 c4 = pc[a / 4], n4 = pn[a / 4], w2 = pw[a / 2];
            const int j = a % 4;
            child[a] = (int)(j == 0 ? c4.x : j == 1 ? c4.y : j == 2 ? c4.z : c4.w);
            cn[a] = (int)(j == 0 ? n4.x : j == 1 ? n4.y : j == 2 ? n4.z : n4.w);
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
        const double lg = v.ltab[min(max((int)hdr.w, 0), v.tlen - 1)];
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
        own[35] = visits;                                            // snac_uct_node.visits, .value_sum
        *reinterpret_cast<double*>(own + 36) = w;
        if (parent < 0) break;
        const int p = clamp_row(parent, base, v.cap);
        const int a = min(max(action, 0), A - 1);
        uint4* const prec = v.stats + (size_t)p * PIECES;
        const uint4 hdr = prec[P_HDR], pown = prec[P_OWN];
        int32_t* const pw = reinterpret_cast<int32_t*>(prec);
        pw[8 + a] = visits;                                          // the mirror in the parent's line 0
        *reinterpret_cast<double*>(pw + 16 + 2 * a) = w;
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

int uct_check(int A, const void* stats, int32_t rows, int32_t B, int32_t cap) {
    using namespace snac_detail;
    if (A != 3 && A != 5 && A != 8) return fail(SNAC_ERR_ARG, "num_actions must be 3, 5 or 8");
    if (!stats) return fail(SNAC_ERR_ARG, "null stats");
    if (B < 1) return fail(SNAC_ERR_ARG, "B must be >= 1");
    if (cap < 1) return fail(SNAC_ERR_ARG, "cap must be >= 1");
    const long long need = (long long)B * ((long long)cap + 1);
    if (need > 0x7FFFFFFFll) return fail(SNAC_ERR_ARG, "B * (cap + 1) rows exceed int32");
    if (need > rows) return fail(SNAC_ERR_ARG, "B * (cap + 1) rows exceed stats_rows");
    if (((uintptr_t)stats & 127) != 0) return fail(SNAC_ERR_ARG, "stats must be 128-byte aligned (records of whole lines)");
    return SNAC_OK;
}

template <class F>
void by_actions(int A, F f) {
    if (A == 3) f(std::integral_constant<int, 3>());
    else if (A == 5) f(std::integral_constant<int, 5>());
    else f(std::integral_constant<int, 8>());
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
    by_actions(num_actions, [&](auto k) {
        hipLaunchKernelGGL((k_uct_select<decltype(k)::value>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, v);
    });
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SNAC_OK : fail_hip(e, "snac_uct_select");
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
    by_actions(num_actions, [&](auto k) {
        hipLaunchKernelGGL((k_uct_backup<decltype(k)::value>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, v);
    });
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SNAC_OK : fail_hip(e, "snac_uct_backup");
}

}  // extern "C"
