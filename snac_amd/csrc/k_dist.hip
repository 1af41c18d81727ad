// k_dist.hip -- snac_c51_expect / snac_c51_project: the expected values of categorical (C51) value distributions, the greedy / double-DQN
// choice of the next action, and the projection of the distributional TD target onto the support.  include/snac_hip.h, "Distributional
// targets", has the rule; every float64 operation below is one of its operations, rounded on its own.
#include <cmath>
#include <cstddef>

#include "snac_units.h"
#include "lane_dev.h"

#pragma clang fp contract(off)                                       // the whole unit: no fused multiply-add anywhere in the rule

// lane = atom: a row of K <= 64 floats is one coalesced dword load of a wave (rows of 204 bytes at K = 51 are aligned as floats only, so
// nothing wider), the expected value is the header's shuffle-down tree, and the projection's scatter becomes a gather: lane i computes
// its own l_i and its two products, then lane j adds, for i = 0 .. K-1 in turn, the lower product where l_i == j and the upper one where
// l_i + 1 == j -- lane i's three values reach every lane through wave-uniform lane reads, so the additions into one atom happen in the
// rule's order and nothing is atomic.  A wave takes SPW samples in turn as a pipeline of two stages: while sample s is chosen (its A rows
// of p_select, ret and discount were loaded an iteration ago), the loads of sample s + 1 are on their way, and the chosen row of p_next,
// whose address needs a_star, is loaded at the end of the choice and used one iteration later, by the projection of sample s.
// k_c51_expect has no second stage: a wave takes two samples and issues both samples' loads together.  All arrays are indexed by unrolled
// constants: they live in registers, there is no scratch and no LDS.
namespace {

using namespace snac_detail;

constexpr int C51_WAVES = 4;                                         // waves per block
constexpr int C51_SPW = 4;                                           // samples a wave of k_c51_project takes in turn
constexpr int C51_EXPECT_SPW = 2;                                    // samples of a wave of k_c51_expect, their loads issued together

struct C51Args {
    int32_t B, K;
    double vmin, vmax, dz;                                           // dz = (vmax - vmin) / (K - 1), from the host
    const float* p_next;
    const float* p_select;                                           // never NULL in the kernel: p_next where the caller gave none
    const float* ret;
    const float* discount;
    float* m;
    int8_t* a_star;
    float* q_star;
    int32_t* bad_rows;
};

// the expected value of the row whose atom `lane` is p (live: lane < K), in every lane: the header's tree (lane_dev.h)
__device__ __forceinline__ double expect_row(float p, double z, bool live) {
    return tree_sum(live ? (double)p * z : 0.0);
}

__device__ __forceinline__ bool bad_sample(float r, float d) {
    return !(fabsf(r) < INFINITY) || !(fabsf(d) < INFINITY) || d < 0.0f;
}

template <int A>
struct C51Sample {                                                   // what the choice of one sample reads
    float p[A];                                                      // atom `lane` of the A rows of p_select
    float r, d;
};

template <int A>
__device__ __forceinline__ C51Sample<A> load_sample(const C51Args& g, size_t b, int lane, bool live) {
    C51Sample<A> s;
    const float* rows = g.p_select + (b * A) * (size_t)g.K + lane;
#pragma unroll
    for (int a = 0; a < A; ++a) s.p[a] = live ? rows[(size_t)a * g.K] : 0.0f;
    s.r = g.ret[b];
    s.d = g.discount[b];
    return s;
}

// the second stage: q_star and the projected row of sample b, whose chosen row of p_next has atom `lane` in `row`
__device__ __forceinline__ void project_sample(const C51Args& g, size_t b, float row, float rf, float df, double z, int lane, bool live) {
    float* out = g.m + b * (size_t)g.K;
    if (bad_sample(rf, df)) {                                        // wave-uniform
        if (live) out[lane] = 0.0f;
        if (lane == 0) {
            if (g.q_star) g.q_star[b] = 0.0f;
            if (g.bad_rows) atomicAdd(g.bad_rows, 1);
        }
        return;
    }
    if (g.q_star) {                                                  // uniform: a kernel argument
        const double qs = expect_row(row, z, live);
        if (lane == 0) g.q_star[b] = (float)qs;
    }
    const int K = g.K;
    const double r = (double)rf, d = (double)df, p = (double)row;
    double t = r + d * z;
    t = t < g.vmin ? g.vmin : t;
    t = t > g.vmax ? g.vmax : t;
    const double pos = (t - g.vmin) / g.dz;                          // in [0, K - 1] up to rounding: t is finite and clamped
    const int fl = (int)floor(pos);
    const int l = fl < K - 1 ? fl : K - 1;
    const double f = pos - (double)l;
    const double lower = l == K - 1 ? p : p * (1.0 - f);
    const double upper = p * f;
    double acc = 0.0;
    for (int i = 0; i < K; ++i) {                                    // wave-uniform; lanes >= K are never a source
        const int li = __builtin_amdgcn_readlane(l, i);
        const double lo_i = lane_read(lower, i), up_i = lane_read(upper, i);
        if (li == lane) acc = acc + lo_i;
        else if (li + 1 == lane) acc = acc + up_i;                   // li == K - 1 has no upper term: lane K, if there is one, stores nothing
    }
    if (live) out[lane] = (float)acc;
}

template <int A>
__global__ __launch_bounds__(64 * C51_WAVES) void k_c51_project(const C51Args g) {
    const int lane = (int)(threadIdx.x & 63u);
    const long long first = ((long long)blockIdx.x * C51_WAVES + (long long)(threadIdx.x >> 6)) * C51_SPW;
    if (first >= g.B) return;                                        // wave-uniform
    const int n = g.B - first < C51_SPW ? (int)(g.B - first) : C51_SPW;
    const bool live = lane < g.K;
    const double z = g.vmin + (double)lane * g.dz;

    C51Sample<A> cur = load_sample<A>(g, (size_t)first, lane, live);
    float row_prev = 0.0f, r_prev = 0.0f, d_prev = 0.0f;
    for (int s = 0; s < n; ++s) {
        const size_t b = (size_t)first + s;
        C51Sample<A> nxt = cur;
        if (s + 1 < n) nxt = load_sample<A>(g, b + 1, lane, live);   // on their way during this sample's choice
        double best = expect_row(cur.p[0], z, live);
        int a_star = 0;
#pragma unroll
        for (int a = 1; a < A; ++a) {
            const double q = expect_row(cur.p[a], z, live);
            if (q > best) { best = q; a_star = a; }                  // a NaN never wins; ties keep the lower index
        }
        if (bad_sample(cur.r, cur.d)) a_star = 0;
        const float row = live ? g.p_next[(b * A + a_star) * (size_t)g.K + lane] : 0.0f;      // a_star is in [0, A) whatever the inputs
        if (g.a_star && lane == 0) g.a_star[b] = (int8_t)a_star;
        if (s > 0) project_sample(g, b - 1, row_prev, r_prev, d_prev, z, lane, live);
        row_prev = row; r_prev = cur.r; d_prev = cur.d;
        cur = nxt;
    }
    project_sample(g, (size_t)first + n - 1, row_prev, r_prev, d_prev, z, lane, live);
}

struct C51ExpectArgs {
    int32_t B, K;
    double vmin, dz;
    const float* p;
    float* q;
};

template <int A>
__global__ __launch_bounds__(64 * C51_WAVES) void k_c51_expect(const C51ExpectArgs g) {
    const int lane = (int)(threadIdx.x & 63u);
    const long long first = ((long long)blockIdx.x * C51_WAVES + (long long)(threadIdx.x >> 6)) * C51_EXPECT_SPW;
    if (first >= g.B) return;
    const int n = g.B - first < C51_EXPECT_SPW ? (int)(g.B - first) : C51_EXPECT_SPW;
    const bool live = lane < g.K;
    const double z = g.vmin + (double)lane * g.dz;
    const float* rows = g.p + ((size_t)first * A) * (size_t)g.K + lane;
    float p[C51_EXPECT_SPW][A];
#pragma unroll
    for (int s = 0; s < C51_EXPECT_SPW; ++s)
#pragma unroll
        for (int a = 0; a < A; ++a) p[s][a] = live && s < n ? rows[(size_t)(s * A + a) * g.K] : 0.0f;
#pragma unroll
    for (int s = 0; s < C51_EXPECT_SPW; ++s) {
        if (s >= n) break;                                           // wave-uniform
        float mine = 0.0f;                                           // lane a keeps row a's value: one store of A floats
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const float q = (float)expect_row(p[s][a], z, live);
            mine = lane == a ? q : mine;
        }
        if (lane < A) g.q[((size_t)first + s) * A + lane] = mine;
    }
}

unsigned c51_blocks(int32_t B, int spw) { return (unsigned)(((long long)B + C51_WAVES * spw - 1) / (C51_WAVES * spw)); }

// the checks both entry points share before by_actions' own; *dz: the support's step
int c51_check(int32_t B, int32_t atoms, double vmin, double vmax, double* dz) {
    if (B < 1) return fail(SNAC_ERR_ARG, "B must be >= 1");
    if (atoms < 2 || atoms > 64) return fail(SNAC_ERR_ARG, "atoms must be in [2, 64]");
    if (!std::isfinite(vmin) || !std::isfinite(vmax) || !(vmin < vmax)) return fail(SNAC_ERR_ARG, "vmin and vmax must be finite, with vmin < vmax");
    *dz = (vmax - vmin) / (double)(atoms - 1);
    return SNAC_OK;
}

}  // namespace

extern "C" int snac_c51_expect(int32_t B, int32_t num_actions, int32_t atoms, double vmin, double vmax, const float* p, float* q, void* stream) {
    using namespace snac_detail;
    if (!p || !q) return fail(SNAC_ERR_ARG, "null p/q");
    double dz;
    if (int rc = c51_check(B, atoms, vmin, vmax, &dz)) return rc;
    return by_actions(num_actions, [&](auto actions) {
        const C51ExpectArgs g{B, atoms, vmin, dz, p, q};
        g_kernel = "k_c51_expect";
        const dim3 grid(c51_blocks(B, C51_EXPECT_SPW)), block(64 * C51_WAVES);
        hipLaunchKernelGGL(k_c51_expect<decltype(actions)::value>, grid, block, 0, (hipStream_t)stream, g);
        return launched("snac_c51_expect");
    });
}

extern "C" int snac_c51_project(int32_t B, int32_t num_actions, int32_t atoms, double vmin, double vmax, const float* p_next,
                                const float* p_select, const float* ret, const float* discount, float* m, int8_t* a_star, float* q_star,
                                int32_t* bad_rows, void* stream) {
    using namespace snac_detail;
    if (!p_next || !ret || !discount || !m) return fail(SNAC_ERR_ARG, "null p_next/ret/discount/m");
    double dz;
    if (int rc = c51_check(B, atoms, vmin, vmax, &dz)) return rc;
    return by_actions(num_actions, [&](auto actions) {
        const C51Args g{B, atoms, vmin, vmax, dz, p_next, p_select ? p_select : p_next, ret, discount, m, a_star, q_star, bad_rows};
        g_kernel = "k_c51_project";
        const dim3 grid(c51_blocks(B, C51_SPW)), block(64 * C51_WAVES);
        hipLaunchKernelGGL(k_c51_project<decltype(actions)::value>, grid, block, 0, (hipStream_t)stream, g);
        return launched("snac_c51_project");
    });
}
