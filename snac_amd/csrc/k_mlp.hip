// k_mlp.hip -- the policy / value network that guides the PUCT search, on the device: snac_mlp_forward (the forward pass of an MLP of up to
// four dense layers), snac_mlp_policy_value (with its softmax / value head) and snac_mlp_uct_value_leaves (with the search's "value the
// leaves" step behind the head), each ONE launch on the caller's stream.  include/snac_hip.h, "Policy / value network on the device", has
// the rule; mlp_rule.h states it per output and per row, for these kernels and for the host.  The weights are read in place from the
// caller's float32 arrays (torch.nn.Linear's parameters) at every launch: nothing is copied or cached between launches.
#include <cmath>
#include <cstddef>

#include "snac_units.h"
#include "mlp_rule.h"
#include "mlp_dev.h"

// k_mlp<A>: a block of 256 threads takes TR = 16 consecutive rows through every layer; the rows' activations stay in LDS from the input
// to the head.  Thread (r, g) = (tid & 15, tid >> 4) owns row r and, in a pass over 64 outputs of a layer, the four outputs
// jbase + 4 g + t: four independent float64 chains, each the stated sum in the stated order -- no sum is split or re-associated.  A
// layer's weights pass through LDS as float32 in tiles of 64 outputs x KC = 32 inputs and are widened to float64 where they are used
// (exact).  Per input a thread reads its row's activation (the 16 lanes of a group read 16 consecutive words, the four groups of a wave
// the same ones: a broadcast) and its four weights as one 16-byte read (one address per group); the reads of eight inputs are issued
// together, ahead of their steps.  The next tile's eight values per thread are loaded from global memory (a lane reads along a row of W:
// 128 contiguous bytes per 32 lanes) into registers before the current tile is used, so a tile costs two barriers.
// Scalar 4- and 8-byte global loads only: nothing of the caller's is assumed 16-byte aligned (a row of 51 float64 is 408 bytes).
// LDS: activations [512][17] + [256][17] float32 (the 17: rows of a column on distinct banks when the input is staged along i) and the
// tile [32][68] float32 (the 68: every thread's four weights 16-byte aligned) = 60 928 bytes, two blocks per CU.  Accumulators, the
// batch and the prefetch are indexed by unrolled constants: no scratch.
// The head (A = 3 / 5 / 8; A = 0: none) runs on the block's first 16 lanes, one row each, after the last layer's outputs are in LDS.
// What was tried and measured (profiles/r31_device_mlp.txt): with the tile as float64 (no widening at the use, twice the LDS bytes per
// step) [51, 256, 256, 6] took 82 us at 64 rows where it now takes 69; four tiles of loads in flight instead of one, and the batch of
// reads alone, changed nothing.
namespace {

using namespace snac_detail;
using namespace snac_spec;
using namespace snac_mlp_dev;                                        // mlp_dev.h: the shape's constants and the layer loop, shared with k_policy_roll.hip
constexpr int ROW_WORDS = sizeof(snac_uct_node) / 4, TERMINAL_WORD = offsetof(snac_uct_node, terminal) / 4;

struct MlpArgs {
    snac_mlp net;
    const void* x;
    int32_t x_is_f64, rows;
    float* y;                                                        // [rows][dim[L]]: forward's output, or the head's `logits`, or NULL
    float* priors;
    double* value;
    int32_t* bad_rows;
    const uint8_t* first_has;                                        // non-null: the search's fused step, which reads these
    const int32_t* first_idx;
    const uint8_t* done;
    const int32_t* stats;
    int32_t stats_rows;
    const int32_t* leaf;
    double* est;
};

template <int A>
__global__ __launch_bounds__(THREADS) void k_mlp(const MlpArgs g) {
    __shared__ float act_a[ACT_A_WORDS];
    __shared__ float act_b[ACT_B_WORDS];
    __shared__ __attribute__((aligned(16))) float wt[WT_WORDS];
    const int tid = threadIdx.x, r = tid & (TR - 1), grp = tid >> 4;
    const long long row0 = (long long)blockIdx.x * TR;
    const int32_t rows = g.rows, L = g.net.layers;

    {   // the block's input rows into act_a[i][r], rounded to float32; a row past the end reads the last row and is dropped at the end
        const int K = g.net.dim[0];
        const long long row = row0 + grp < rows ? row0 + grp : rows - 1;
        const bool f64 = g.x_is_f64 != 0;                            // uniform
        for (int i = r; i < K; i += TR) act_a[i * AS + grp] = mlp_input(g.x, f64, (size_t)row * K + i);
    }

    mlp_layers(g.net, act_a, act_b, wt, tid);
    const float* res = mlp_result(L, act_a, act_b);
    const int N = g.net.dim[L];
    if (g.y) {                                                       // the block's rows are one contiguous span of y
        const long long left = rows - row0;
        const int n = (int)(left < TR ? left : TR) * N;
        for (int e = tid; e < n; e += THREADS) {
            const int rr = e / N, j = e - rr * N;
            g.y[(size_t)row0 * N + e] = res[j * AS + rr];
        }
    }
    if constexpr (A > 0) {
        const long long s = row0 + tid;
        if (tid < TR && s < rows) {
            float yv[A + 1], p[A];
#pragma unroll
            for (int a = 0; a <= A; ++a) yv[a] = res[a * AS + tid];
            double v;
            const bool bad = mlp_head<A>(yv, p, v);
            if (bad && g.bad_rows) atomicAdd(g.bad_rows, 1);
            if (g.priors) {
#pragma unroll
                for (int a = 0; a < A; ++a) g.priors[(size_t)s * A + a] = p[a];
            }
            if (g.first_has) {                                       // the search's step (uniform: a kernel argument): S = rows
                const bool term = mlp_leaf_terminal(g.first_has[s] != 0, g.first_idx[s], g.done, rows, g.stats, g.stats_rows, g.leaf[s], ROW_WORDS,
                                                    TERMINAL_WORD);
                v = term ? 0.0 : v;
                if (g.est) g.est[s] = g.est[s] + v;
            }
            if (g.value) g.value[s] = v;
        }
    }
}

int aligned(const void* p, size_t n, const char* msg) { return ((uintptr_t)p % n) ? fail(SNAC_ERR_ARG, msg) : SNAC_OK; }

// the checks of the two entry points with a head
int head_check(const snac_mlp* net, int32_t num_actions, const float* priors, const double* value, const float* logits, const int32_t* bad_rows) {
    if (int rc = by_actions(num_actions, [](auto) { return (int)SNAC_OK; })) return rc;
    if (net->dim[net->layers] != num_actions + 1) return fail(SNAC_ERR_ARG, "dim[layers] must be num_actions + 1: the logits and the value");
    if (int rc = aligned(priors, 4, "priors must be 4-byte aligned")) return rc;
    if (int rc = aligned(logits, 4, "logits must be 4-byte aligned")) return rc;
    if (int rc = aligned(value, 8, "value must be 8-byte aligned")) return rc;
    return aligned(bad_rows, 4, "bad_rows must be 4-byte aligned");
}

template <int A>
int launch_mlp(const MlpArgs& g, const char* kernel, const char* entry, void* stream) {
    g_kernel = kernel;
    hipLaunchKernelGGL(k_mlp<A>, dim3((unsigned)(((long long)g.rows + TR - 1) / TR)), dim3(THREADS), 0, (hipStream_t)stream, g);
    return launched(entry);
}

}  // namespace

// the network's own checks (snac_units.h): its layers, every dim, its pointers and their alignment
int snac_detail::mlp_net_check(const snac_mlp* net) {
    if (!net) return fail(SNAC_ERR_ARG, "null net");
    if (const char* why = snac_spec::mlp_dims_refusal(net->layers, net->dim)) return fail(SNAC_ERR_ARG, why);
    for (int l = 0; l < net->layers; ++l) {
        if (!net->w[l] || !net->b[l]) return fail(SNAC_ERR_ARG, "null weights / bias of a layer");
        if ((uintptr_t)net->w[l] % 4 || (uintptr_t)net->b[l] % 4) return fail(SNAC_ERR_ARG, "weights and biases must be 4-byte aligned");
    }
    return SNAC_OK;
}

// the checks of the entry points on rows of inputs (snac_units.h): the network, the input rows and their alignment
int snac_detail::mlp_check(const snac_mlp* net, const void* x, int x_is_f64, int32_t rows) {
    if (int rc = mlp_net_check(net)) return rc;
    if (!x) return fail(SNAC_ERR_ARG, "null x");
    if (x_is_f64 != 0 && x_is_f64 != 1) return fail(SNAC_ERR_ARG, "x_is_f64 must be 0 or 1");
    if ((uintptr_t)x % (x_is_f64 ? 8 : 4)) return fail(SNAC_ERR_ARG, "x must be aligned as its element type");
    if (rows < 1) return fail(SNAC_ERR_ARG, "rows must be >= 1");
    return SNAC_OK;
}

extern "C" int snac_mlp_forward(const snac_mlp* net, const void* x, int x_is_f64, int32_t rows, float* y, void* stream) {
    using namespace snac_detail;
    if (int rc = mlp_check(net, x, x_is_f64, rows)) return rc;
    if (int rc = aligned(y, 4, "y must be 4-byte aligned")) return rc;
    if (!y) return SNAC_OK;                                          // nothing asked for
    MlpArgs g{};
    g.net = *net, g.x = x, g.x_is_f64 = x_is_f64, g.rows = rows, g.y = y;
    return launch_mlp<0>(g, "k_mlp_forward", "snac_mlp_forward", stream);
}

extern "C" int snac_mlp_policy_value(const snac_mlp* net, int32_t num_actions, const void* x, int x_is_f64, int32_t rows, float* priors, double* value,
                                     float* logits, int32_t* bad_rows, void* stream) {
    using namespace snac_detail;
    if (int rc = mlp_check(net, x, x_is_f64, rows)) return rc;
    if (int rc = head_check(net, num_actions, priors, value, logits, bad_rows)) return rc;
    if (!priors && !value && !logits && !bad_rows) return SNAC_OK;
    MlpArgs g{};
    g.net = *net, g.x = x, g.x_is_f64 = x_is_f64, g.rows = rows, g.y = logits, g.priors = priors, g.value = value, g.bad_rows = bad_rows;
    return by_actions(num_actions, [&](auto k) { return launch_mlp<decltype(k)::value>(g, "k_mlp_policy_value", "snac_mlp_policy_value", stream); });
}

extern "C" int snac_mlp_uct_value_leaves(const snac_mlp* net, int32_t num_actions, const void* obs, int obs_is_f64, int32_t S, const uint8_t* first_has,
                                         const int32_t* first_idx, const uint8_t* done, const int32_t* stats, int32_t stats_rows, const int32_t* leaf,
                                         float* priors, double* value, double* est, int32_t* bad_rows, void* stream) {
    using namespace snac_detail;
    if (int rc = mlp_check(net, obs, obs_is_f64, S)) return rc;
    if (int rc = head_check(net, num_actions, priors, value, nullptr, bad_rows)) return rc;
    if (!first_has || !first_idx || !done || !stats || !leaf) return fail(SNAC_ERR_ARG, "null first_has / first_idx / done / stats / leaf");
    if (stats_rows < 1) return fail(SNAC_ERR_ARG, "stats_rows must be >= 1");
    if ((uintptr_t)first_idx % 4 || (uintptr_t)stats % 4 || (uintptr_t)leaf % 4) return fail(SNAC_ERR_ARG, "first_idx, stats and leaf must be 4-byte aligned");
    if (int rc = aligned(est, 8, "est must be 8-byte aligned")) return rc;
    if (!priors && !value && !est && !bad_rows) return SNAC_OK;
    MlpArgs g{};
    g.net = *net, g.x = obs, g.x_is_f64 = obs_is_f64, g.rows = S, g.priors = priors, g.value = value, g.bad_rows = bad_rows;
    g.first_has = first_has, g.first_idx = first_idx, g.done = done, g.stats = stats, g.stats_rows = stats_rows, g.leaf = leaf, g.est = est;
    return by_actions(num_actions, [&](auto k) { return launch_mlp<decltype(k)::value>(g, "k_mlp_value_leaves", "snac_mlp_uct_value_leaves", stream); });
}
