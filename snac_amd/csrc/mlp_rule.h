// mlp_rule.h -- the rule of include/snac_hip.h, "Policy / value network on the device", in the pieces that k_mlp.hip runs per lane and
// that a host compiler can compile as they stand (tests/native/mlp_host.cpp, with -ffp-contract=off): the input value of a row, one
// step of an output's sum, the end of a hidden and of a last output, and the policy / value head of a row of A + 1 outputs.  The softmax
// is softmax_rule.h's.  mlp_layer below is the rule of one layer for one row as a plain loop: what the host runs, and what the kernel's
// tiles must equal -- the kernel takes the same steps in the same order, with the rows and the outputs spread over its lanes.
//
// The sum of one output is a chain: acc = (double)b[j], then acc = acc + (double)W[j][i] * (double)x[i] for i = 0, 1, .., K - 1 in that
// order.  The product of two float32 values is exact in float64 (24 + 24 bits of significand, exponents far inside the range), so the
// step rounds once whether the compiler emits a fused multiply-add or a multiply and an add: both give the same bits, and no contraction
// pragma is needed for that line.  What would change the bits is another order of the additions; the chain of one output is therefore
// never split across lanes or re-associated.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "softmax_rule.h"

namespace snac_spec {

constexpr int MLP_MAX_LAYERS = 4, MLP_MAX_IN = 512, MLP_MAX_HIDDEN = 256, MLP_MAX_OUT = 64;

// why a network is refused, or nullptr: 1 <= layers <= 4, dim[0] in 1..512, hidden widths in 1..256, dim[layers] in 1..64
SNAC_SPEC_FN const char* mlp_dims_refusal(int32_t layers, const int32_t* dim) {
    if (layers < 1 || layers > MLP_MAX_LAYERS) return "layers must be 1 .. 4";
    if (dim[0] < 1 || dim[0] > MLP_MAX_IN) return "dim[0] (the input width) must be 1 .. 512";
    for (int l = 1; l < layers; ++l)
        if (dim[l] < 1 || dim[l] > MLP_MAX_HIDDEN) return "a hidden width must be 1 .. 256";
    if (dim[layers] < 1 || dim[layers] > MLP_MAX_OUT) return "dim[layers] (the output width) must be 1 .. 64";
    return nullptr;
}

// value i of a row of inputs: float32 as it is, float64 rounded to float32 first
SNAC_SPEC_FN float mlp_input(const void* x, bool is_f64, size_t i) {
    return is_f64 ? (float)static_cast<const double*>(x)[i] : static_cast<const float*>(x)[i];
}

// one step of the chain (the product is exact: see above)
SNAC_SPEC_FN double mlp_step(double acc, double w, float x) { return acc + w * (double)x; }

// the end of the chain: a hidden output through ReLU (a NaN stays a NaN, -0.0 stays -0.0), an output of the last layer as it is
SNAC_SPEC_FN float mlp_hidden(double acc) { return acc < 0.0 ? 0.0f : (float)acc; }
SNAC_SPEC_FN float mlp_last(double acc) { return (float)acc; }

// One layer for one row: y[j] for j in [0, N) from x[0 .. K), W [N][K] row-major and b [N].
SNAC_SPEC_FN void mlp_layer(const float* W, const float* b, const float* x, int K, int N, bool last, float* y) {
    for (int j = 0; j < N; ++j) {
        double acc = (double)b[j];
        for (int i = 0; i < K; ++i) acc = mlp_step(acc, (double)W[(size_t)j * K + i], x[i]);
        y[j] = last ? mlp_last(acc) : mlp_hidden(acc);
    }
}

// The policy / value head of a row y[0 .. A]: logits y[0 .. A), value y[A].  Returns whether the row is bad (the scan says so, or y[A] is
// not finite); a bad row gets priors of +0.0 and value 0.0.
template <int A>
SNAC_SPEC_FN bool mlp_head(const float (&y)[A + 1], float (&p)[A], double& value) {
#pragma clang fp contract(off)
    float l[A];
#pragma unroll
    for (int a = 0; a < A; ++a) l[a] = y[a];
    float m;
    bool bad = softmax_scan(l, m);
    bad |= !(fabsf(y[A]) < INFINITY);
    value = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) p[a] = 0.0f;
    if (bad) return true;
    double x[A], e[A];
    softmax_terms(l, m, x, e);
    const SoftmaxSums s = softmax_sums(x, e);
#pragma unroll
    for (int a = 0; a < A; ++a) p[a] = (float)(e[a] / s.S);
    value = (double)y[A];
    return false;
}

// The fused step of the search for slot s: whether its leaf is terminal, from the expander's done or the stored node's terminal word
// (indices clamped into range), and what the leaf adds to est.
SNAC_SPEC_FN bool mlp_leaf_terminal(bool first_has, int32_t first_idx, const uint8_t* done, int32_t S, const int32_t* stats, int32_t stats_rows,
                                    int32_t leaf, int row_words, int terminal_word) {
    if (first_has) {
        const int32_t f = first_idx < 0 ? 0 : first_idx > S - 1 ? S - 1 : first_idx;
        return done[f] != 0;
    }
    const int32_t n = leaf < 0 ? 0 : leaf > stats_rows - 1 ? stats_rows - 1 : leaf;
    return stats[(size_t)n * row_words + terminal_word] != 0;
}

}  // namespace snac_spec
