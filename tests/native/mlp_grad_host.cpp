// mlp_grad_host.cpp -- the rule k_mlp_grad runs (snac_amd/csrc/mlp_grad_rule.h), compiled for the host as it stands:
// tests/test_mlp_backward_host.py builds this file into a shared object with the system compiler and -ffp-contract=off and compares every
// gradient's bytes with the numpy statement of the rule.  The loops below are the launch sequence's with the row a loop index: the
// forward rule's activations through mlp_layer, the deltas through mlp_backward_row, the sums over the batch through mlp_grad_batch.
// With -DMLP_GRAD_HOST_MAIN the file is a program: networks at the limits of every dimension in exactly sized heap arrays, for a run
// under the host sanitizers.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mlp_grad_rule.h"

// -> P, the number of gradients written to grad (in the layout of the header); -1 for a refused network or rows < 1 or chunk < 1
extern "C" int mlp_grad_host(int32_t layers, const int32_t* dim, const float* const* w, const float* const* b, const void* x, int x_is_f64,
                             int32_t rows, const float* grad_y, int32_t chunk, int32_t accumulate, float* grad) {
    using namespace snac_spec;
    if (mlp_dims_refusal(layers, dim) || rows < 1 || chunk < 1) return -1;
    int32_t off[MLP_MAX_LAYERS];
    const int32_t P = mlp_grad_layout(layers, dim, off);
    std::vector<std::vector<float>> h(layers + 1), d(layers + 1);    // h[l], d[l]: [rows][dim[l]]
    for (int l = 0; l <= layers; ++l) h[l].assign((size_t)rows * dim[l], 0.0f);
    for (int l = 1; l < layers; ++l) d[l].assign((size_t)rows * dim[l], 0.0f);
    for (long long s = 0; s < rows; ++s) {
        for (int i = 0; i < dim[0]; ++i) h[0][(size_t)s * dim[0] + i] = mlp_input(x, x_is_f64 != 0, (size_t)s * dim[0] + i);
        const float* hp[MLP_MAX_LAYERS + 1] = {};
        float* dp[MLP_MAX_LAYERS + 1] = {};
        for (int l = 0; l < layers; ++l)
            mlp_layer(w[l], b[l], h[l].data() + (size_t)s * dim[l], dim[l], dim[l + 1], l == layers - 1, h[l + 1].data() + (size_t)s * dim[l + 1]);
        for (int l = 0; l <= layers; ++l) hp[l] = h[l].data() + (size_t)s * dim[l];
        for (int l = 1; l < layers; ++l) dp[l] = d[l].data() + (size_t)s * dim[l];
        mlp_backward_row(layers, dim, w, hp, grad_y + (size_t)s * dim[layers], dp);
    }
    for (int l = 0; l < layers; ++l)
        mlp_grad_batch(l == layers - 1 ? grad_y : d[l + 1].data(), h[l].data(), rows, dim[l], dim[l + 1], chunk, accumulate != 0, grad + off[l]);
    return P;
}

#ifdef MLP_GRAD_HOST_MAIN
#include <cstdio>

// Networks at the limits of every dimension and the smallest ones, float32 and float64 inputs, rows on both sides of a chunk's end, a
// NaN row and a huge gradient, written and accumulated: anything indexed past a row, a layer or the flat gradient shows under
// -fsanitize=address,undefined.  Prints the counts; exit status 1 if one is off: the layout's P, and that a layer above a dead unit (every
// weight into it zero and a negative bias) gets no gradient through it.
int main() {
    struct Net { int layers; int32_t dim[5]; };
    const Net nets[] = {{1, {7, 4, 0, 0, 0}}, {2, {51, 64, 6, 0, 0}}, {3, {51, 65, 1, 9, 0}}, {3, {502, 256, 256, 6, 0}}, {3, {512, 256, 255, 64, 0}},
                        {1, {1, 1, 0, 0, 0}}, {4, {512, 256, 256, 256, 64}}};
    const int32_t chunk = 16;
    int status = 0;
    for (const Net& n : nets) {
        for (int32_t rows : {1, 16, 17, 33}) {
            for (int f64 = 0; f64 < 2; ++f64) {
                std::vector<std::vector<float>> w(n.layers), b(n.layers);
                const float* wp[4] = {nullptr, nullptr, nullptr, nullptr};
                const float* bp[4] = {nullptr, nullptr, nullptr, nullptr};
                int32_t want_P = 0;
                for (int l = 0; l < n.layers; ++l) {
                    const int K = n.dim[l], N = n.dim[l + 1];
                    want_P += N * K + N;
                    w[l].resize((size_t)K * N);
                    b[l].resize((size_t)N);
                    for (size_t e = 0; e < w[l].size(); ++e) w[l][e] = 0.03125f * (float)((int)((e * 7 + l * 3) % 31) - 15) / (float)(1 + K / 16);
                    for (int j = 0; j < N; ++j) b[l][j] = 0.125f * (float)((j * 5 + l) % 9 - 4);
                    wp[l] = w[l].data();
                    bp[l] = b[l].data();
                }
                const bool dead = n.layers >= 2;                     // hidden unit 0 of layer 0 is dead in every row
                if (dead) {
                    for (int i = 0; i < n.dim[0]; ++i) w[0][i] = 0.0f;
                    b[0][0] = -1.0f;
                }
                const int K0 = n.dim[0], N = n.dim[n.layers];
                std::vector<float> xf((size_t)rows * K0), gy((size_t)rows * N);
                std::vector<double> xd((size_t)rows * K0);
                for (int32_t s = 0; s < rows; ++s) {
                    for (int i = 0; i < K0; ++i) xf[(size_t)s * K0 + i] = 0.25f * (float)((s * 3 + i * 5) % 13 - 6);
                    if (s % 5 == 1 && !dead) xf[(size_t)s * K0 + (s % K0)] = NAN;
                    for (int i = 0; i < K0; ++i) xd[(size_t)s * K0 + i] = (double)xf[(size_t)s * K0 + i];
                    for (int k = 0; k < N; ++k) gy[(size_t)s * N + k] = (s % 7 == 3 ? 3.0e38f : 0.5f) * (float)((s + 2 * k) % 5 - 2);
                }
                std::vector<float> grad((size_t)want_P, 1.0f);
                const void* x = f64 ? (const void*)xd.data() : (const void*)xf.data();
                int bad = 0;
                for (int accumulate = 0; accumulate < 2; ++accumulate) {
                    const int P = mlp_grad_host(n.layers, n.dim, wp, bp, x, f64, rows, gy.data(), chunk, accumulate, grad.data());
                    bad += P != want_P;
                    if (dead) {                                      // the weights into the dead unit and its bias: exactly zero, then 0 + 0
                        for (int i = 0; i < K0; ++i) bad += grad[i] != 0.0f;
                        bad += grad[(size_t)n.dim[1] * K0] != 0.0f;
                    }
                }
                std::printf("layers %d in %d out %d rows %d f64 %d: P %d, off %d\n", n.layers, K0, N, (int)rows, f64, (int)want_P, bad);
                if (bad) status = 1;
            }
        }
    }
    const int32_t wide[5] = {513, 4, 0, 0, 0};
    if (mlp_grad_host(1, wide, nullptr, nullptr, nullptr, 0, 1, nullptr, 16, 0, nullptr) != -1) status = 1;
    return status;
}
#endif
