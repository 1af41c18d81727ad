// mlp_host.cpp -- the rule k_mlp runs (snac_amd/csrc/mlp_rule.h), compiled for the host as it stands: tests/test_mlp_host.py builds this
// file into a shared object with the system compiler and -ffp-contract=off and compares every output's bytes with the numpy statement of
// the rule.  The loop below is the kernel's with the row a loop index: the layers through mlp_layer, the head through mlp_head, the
// search's fused step through mlp_leaf_terminal; the entry points' conventions for NULL pointers hold.
// With -DMLP_HOST_MAIN the file is a program: networks at the limits of every dimension with masked, bad and overflowing rows, for a run
// under the host sanitizers.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mlp_rule.h"

namespace {

using namespace snac_spec;

struct Leaves {                                                      // the fused step's inputs; first_has null: no fused step
    const uint8_t* first_has;
    const int32_t* first_idx;
    const uint8_t* done;
    const int32_t* stats;
    int32_t stats_rows, row_words, terminal_word;
    const int32_t* leaf;
    double* est;
};

template <int A>
int head_row(const float* y, long long s, int32_t rows, const Leaves& lv, float* priors, double* value) {
    float yv[A + 1], p[A];
    for (int a = 0; a <= A; ++a) yv[a] = y[a];
    double v;
    const bool bad = mlp_head<A>(yv, p, v);
    if (priors)
        for (int a = 0; a < A; ++a) priors[(size_t)s * A + a] = p[a];
    if (lv.first_has) {
        const bool term = mlp_leaf_terminal(lv.first_has[s] != 0, lv.first_idx[s], lv.done, rows, lv.stats, lv.stats_rows, lv.leaf[s], lv.row_words,
                                            lv.terminal_word);
        v = term ? 0.0 : v;
        if (lv.est) lv.est[s] = lv.est[s] + v;
    }
    if (value) value[s] = v;
    return bad;
}

}  // namespace

// -> the number of bad rows (0 without a head), -1 for a refused network, -2 for an unsupported num_actions (0: no head)
extern "C" int mlp_host(int32_t layers, const int32_t* dim, const float* const* w, const float* const* b, const void* x, int x_is_f64, int32_t rows,
                        int32_t num_actions, float* y, float* priors, double* value, const uint8_t* first_has, const int32_t* first_idx,
                        const uint8_t* done, const int32_t* stats, int32_t stats_rows, int32_t row_words, int32_t terminal_word, const int32_t* leaf,
                        double* est) {
    if (mlp_dims_refusal(layers, dim)) return -1;
    if (num_actions != 0 && num_actions != 3 && num_actions != 5 && num_actions != 8) return -2;
    if (num_actions != 0 && dim[layers] != num_actions + 1) return -1;
    const Leaves lv{first_has, first_idx, done, stats, stats_rows, row_words, terminal_word, leaf, est};
    int bad = 0;
    std::vector<float> cur, next;
    for (long long s = 0; s < rows; ++s) {
        cur.assign((size_t)dim[0], 0.0f);
        for (int i = 0; i < dim[0]; ++i) cur[i] = mlp_input(x, x_is_f64 != 0, (size_t)s * dim[0] + i);
        for (int l = 0; l < layers; ++l) {
            next.assign((size_t)dim[l + 1], 0.0f);
            mlp_layer(w[l], b[l], cur.data(), dim[l], dim[l + 1], l == layers - 1, next.data());
            cur.swap(next);
        }
        const int N = dim[layers];
        if (y)
            for (int j = 0; j < N; ++j) y[(size_t)s * N + j] = cur[j];
        switch (num_actions) {
            case 3: bad += head_row<3>(cur.data(), s, rows, lv, priors, value); break;
            case 5: bad += head_row<5>(cur.data(), s, rows, lv, priors, value); break;
            case 8: bad += head_row<8>(cur.data(), s, rows, lv, priors, value); break;
            default: break;
        }
    }
    return bad;
}

#ifdef MLP_HOST_MAIN
#include <cstdio>

// Networks at the limits of every dimension and the smallest ones, in exactly sized heap arrays, float32 and float64 inputs, with rows
// that overflow a hidden unit, carry a NaN, mask a logit, mask every logit and give a value that is not finite, and the fused step with
// indices outside their range: anything indexed past a row or a layer shows under -fsanitize=address,undefined.  Prints the counts; exit
// status 1 if a count is off.
int main() {
    struct Net { int layers; int32_t dim[5]; int A; };
    const Net nets[] = {{1, {7, 4, 0, 0, 0}, 3}, {2, {51, 64, 6, 0, 0}, 5}, {3, {51, 65, 1, 9, 0}, 8}, {3, {502, 256, 256, 6, 0}, 5},
                        {3, {512, 256, 255, 64, 0}, 0}, {1, {1, 1, 0, 0, 0}, 0}, {4, {512, 256, 256, 256, 64}, 0}};
    int status = 0;
    for (const Net& n : nets) {
        for (int32_t rows : {1, 17, 65}) {
            for (int f64 = 0; f64 < 2; ++f64) {
                std::vector<std::vector<float>> w(n.layers), b(n.layers);
                const float* wp[4] = {nullptr, nullptr, nullptr, nullptr};
                const float* bp[4] = {nullptr, nullptr, nullptr, nullptr};
                for (int l = 0; l < n.layers; ++l) {
                    const int K = n.dim[l], N = n.dim[l + 1];
                    w[l].resize((size_t)K * N);
                    b[l].resize((size_t)N);
                    for (size_t e = 0; e < w[l].size(); ++e) w[l][e] = 0.03125f * (float)((int)((e * 7 + l * 3) % 31) - 15) / (float)(1 + K / 16);
                    for (int j = 0; j < N; ++j) b[l][j] = 0.125f * (float)((j * 5 + l) % 9 - 4);
                    wp[l] = w[l].data();
                    bp[l] = b[l].data();
                }
                const int K0 = n.dim[0], N = n.dim[n.layers];
                std::vector<float> xf((size_t)rows * K0);
                std::vector<double> xd((size_t)rows * K0);
                int want_bad = 0;
                for (int32_t s = 0; s < rows; ++s) {
                    for (int i = 0; i < K0; ++i) xf[(size_t)s * K0 + i] = 0.25f * (float)((s * 3 + i * 5) % 13 - 6);
                    if (s % 5 == 1) xf[(size_t)s * K0 + (s % K0)] = NAN;                         // a NaN goes through every layer: a bad row
                    if (s % 5 == 3) xf[(size_t)s * K0] = 3.0e38f;                                // a huge input: overflow wherever its weight is not 0
                    for (int i = 0; i < K0; ++i) xd[(size_t)s * K0 + i] = (double)xf[(size_t)s * K0 + i];
                }
                std::vector<float> y((size_t)rows * N), priors((size_t)rows * (n.A ? n.A : 1));
                std::vector<double> value(rows), est(rows, 1.0);
                std::vector<uint8_t> first_has(rows), done(rows);
                std::vector<int32_t> first_idx(rows), leaf(rows), stats((size_t)3 * 64, 0);
                stats[1 * 64 + 34] = 1;
                for (int32_t s = 0; s < rows; ++s) {
                    first_has[s] = s % 2;
                    first_idx[s] = s % 7 == 0 ? -5 : s % 7 == 1 ? rows + 9 : s;                  // outside the range: clamped
                    done[s] = s % 3 == 0;
                    leaf[s] = s % 4 == 0 ? -1 : s % 4 == 1 ? 99 : s % 3;
                }
                const void* x = f64 ? (const void*)xd.data() : (const void*)xf.data();
                const int bad = mlp_host(n.layers, n.dim, wp, bp, x, f64, rows, n.A, y.data(), n.A ? priors.data() : nullptr, n.A ? value.data() : nullptr,
                                         n.A ? first_has.data() : nullptr, first_idx.data(), done.data(), stats.data(), 3, 64, 34, leaf.data(),
                                         n.A ? est.data() : nullptr);
                if (n.A) {                                           // the head's own count of the rows it refused, from y
                    for (int32_t s = 0; s < rows; ++s) {
                        bool any = false, all_masked = true;
                        for (int a = 0; a < n.A; ++a) {
                            const float l = y[(size_t)s * N + a];
                            any |= l != l || l == INFINITY;
                            all_masked &= l == -INFINITY;
                        }
                        want_bad += any || all_masked || !(std::fabs(y[(size_t)s * N + n.A]) < INFINITY);
                    }
                }
                std::printf("layers %d in %d out %d rows %d f64 %d: bad %d (want %d)\n", n.layers, K0, N, (int)rows, f64, bad, want_bad);
                if (bad != want_bad) status = 1;
            }
        }
    }
    const int32_t wide[5] = {513, 4, 0, 0, 0};
    if (mlp_host(1, wide, nullptr, nullptr, nullptr, 0, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 64, 34, nullptr, nullptr) != -1)
        status = 1;
    return status;
}
#endif
