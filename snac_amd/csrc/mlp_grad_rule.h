// mlp_grad_rule.h -- the rule of include/snac_hip.h, "Backward pass of the device network", in the pieces that k_mlp_grad.hip runs per lane
// and that a host compiler can compile as they stand (tests/native/mlp_grad_host.cpp, with -ffp-contract=off): one step of a delta chain
// and its mask, one step of a chunk's chain for a weight and for a bias, the chain over the chunks and the end with and without
// accumulation.  mlp_backward_row and mlp_grad_batch below are the rule as plain loops: what the host runs, and what the kernels' tiles
// must equal -- the kernels take the same steps in the same order, with the rows, the units and the chunks spread over lanes and blocks.
//
// Every product here is of two float32 values and therefore exact in float64 (mlp_rule.h), so each step rounds once, in its addition,
// whether the compiler contracts it or not.  What would change the bits is another order of the additions: the chain of a unit's delta
// over k, of a chunk's partial over its rows and of a total over the chunks is never split or re-associated.
#pragma once
#include <cstddef>
#include <cstdint>

#include "mlp_rule.h"

namespace snac_spec {

// one step of the chain of delta_l[i] over the units k of the layer above: acc + W_l[k][i] * delta_{l+1}[k]
SNAC_SPEC_FN double mlp_delta_step(double acc, float w, float d) { return acc + (double)w * (double)d; }

// the end of that chain: torch's threshold_backward on the forward rule's own activation (+0.0 and -0.0 pass nothing, a NaN passes acc)
SNAC_SPEC_FN float mlp_delta_mask(float h, double acc) { return h <= 0.0f ? 0.0f : (float)acc; }

// one step of a chunk's chain over its rows, for a weight (delta_{l+1}[b][j] * h_l[b][i]) and for a bias (delta_{l+1}[b][j])
SNAC_SPEC_FN double mlp_grad_step(double part, float d, float h) { return part + (double)d * (double)h; }
SNAC_SPEC_FN double mlp_grad_bias_step(double part, float d) { return part + (double)d; }

// the chain over the chunks' partials part[c * stride], c ascending
SNAC_SPEC_FN double mlp_grad_total(const double* part, size_t stride, int64_t chunks) {
    double total = 0.0;
    for (int64_t c = 0; c < chunks; ++c) total = total + part[(size_t)c * stride];
    return total;
}

// the result: written, or added to what was there in float64 and rounded once
SNAC_SPEC_FN float mlp_grad_end(double total, float g_old, bool accumulate) { return accumulate ? (float)((double)g_old + total) : (float)total; }

// P, the length of the flat gradient: per layer its weights [dim[l+1]][dim[l]] and then its bias [dim[l+1]]; off[l]: where layer l begins
SNAC_SPEC_FN int32_t mlp_grad_layout(int32_t layers, const int32_t* dim, int32_t* off) {
    int32_t P = 0;
    for (int l = 0; l < layers; ++l) {
        if (off) off[l] = P;
        P += dim[l + 1] * (dim[l] + 1);
    }
    return P;
}

// The deltas of one row, from the top down: delta[L] = the row of grad_y as it is; delta[l][i] for l = L-1 .. 1 from W_l, delta[l+1]
// and the forward rule's activation h[l] (h[l]: dim[l] values; h[0], the input, is not used).  delta[l]: dim[l] values, written for
// l = 1 .. L-1; delta[0] is not computed.
SNAC_SPEC_FN void mlp_backward_row(int32_t layers, const int32_t* dim, const float* const* w, const float* const* h, const float* grad_y,
                                   float* const* delta) {
    const float* up = grad_y;
    for (int l = layers - 1; l >= 1; --l) {
        const int K = dim[l + 1], N = dim[l];
        for (int i = 0; i < N; ++i) {
            double acc = 0.0;
            for (int k = 0; k < K; ++k) acc = mlp_delta_step(acc, w[l][(size_t)k * N + i], up[k]);
            delta[l][i] = mlp_delta_mask(h[l][i], acc);
        }
        up = delta[l];
    }
}

// The sums over the batch for one layer: d [rows][N] (delta_{l+1}), h [rows][K] (h_l), chunks of `chunk` rows; g: the layer's part of the
// flat gradient, N * K weights and then N biases.
SNAC_SPEC_FN void mlp_grad_batch(const float* d, const float* h, int64_t rows, int K, int N, int chunk, bool accumulate, float* g) {
    const int64_t chunks = (rows + chunk - 1) / chunk;
    for (int j = 0; j < N; ++j) {
        for (int i = 0; i <= K; ++i) {                               // i == K: the bias
            double total = 0.0;
            for (int64_t c = 0; c < chunks; ++c) {
                const int64_t end = (c + 1) * chunk < rows ? (c + 1) * chunk : rows;
                double part = 0.0;
                for (int64_t b = c * chunk; b < end; ++b)
                    part = i < K ? mlp_grad_step(part, d[(size_t)b * N + j], h[(size_t)b * K + i]) : mlp_grad_bias_step(part, d[(size_t)b * N + j]);
                total = total + part;
            }
            float* out = i < K ? g + (size_t)j * K + i : g + (size_t)N * K + j;
            *out = mlp_grad_end(total, accumulate ? *out : 0.0f, accumulate);
        }
    }
}

}  // namespace snac_spec
