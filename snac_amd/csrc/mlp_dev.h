// mlp_dev.h -- the layer loop of the device network, once, for the kernels that run it: k_mlp (k_mlp.hip: rows from memory, one pass),
// k_policy_rollout (k_policy_roll.hip: the rows are the block's envs, one pass per tick) and k_mlp_grad_rows (k_mlp_grad.hip: the
// activations recomputed for the backward pass, parked through the hook below).  A block of 256 threads takes TR = 16 rows through every
// layer with the rows' activations in LDS; k_mlp.hip's head comment has the shape and what was measured.  Device code only.
#pragma once
#include "snac_units.h"
#include "mlp_rule.h"

namespace snac_mlp_dev {

using namespace snac_spec;

constexpr int TR = 16, THREADS = 256, JT = 4, PASS = 64, KC = 32, WS = PASS + 4, AS = TR + 1, PRE = PASS * KC / THREADS;
constexpr int BATCH = 8;                                             // inputs whose LDS reads are issued together
constexpr int ACT_A_WORDS = MLP_MAX_IN * AS, ACT_B_WORDS = MLP_MAX_HIDDEN * AS, WT_WORDS = KC * WS;
static_assert(PRE * THREADS == PASS * KC && JT * (THREADS / TR) == PASS, "the tile is covered once by the prefetch and once by the chains");

// Every layer of `net` for the block's 16 rows.  In: act_a[i * AS + r] = input i of row r, written by any thread before the call (the
// first barrier below orders those writes before the first read).  Out: the last layer's outputs at res[j * AS + r], res = mlp_result(),
// visible to every thread (the loop ends in a barrier).  wt: the 16-byte aligned weight tile.  Thread (r, g) = (tid & 15, tid >> 4) owns
// row r and, in a pass over 64 outputs, the four outputs jbase + 4 g + t.  Every thread of the block calls it (uniform throughout).
// park(l, j, r, v): called by the owning thread with every value v = output j of layer l for row r as it is written (k_mlp_grad.hip keeps
// the hidden activations that the two LDS arrays, used in turn, do not); the default does nothing.
struct MlpNoPark {
    __device__ __forceinline__ void operator()(int, int, int, float) const {}
};
template <class Park = MlpNoPark>
__device__ __forceinline__ void mlp_layers(const snac_mlp& net, float* act_a, float* act_b, float* wt, int tid, Park park = Park()) {
    const int r = tid & (TR - 1), grp = tid >> 4;
    const int32_t L = net.layers;
    for (int l = 0; l < L; ++l) {                                    // uniform throughout
        const int K = net.dim[l], N = net.dim[l + 1];
        const float* W = net.w[l];
        const float* bias = net.b[l];
        const float* in = (l & 1) ? act_b : act_a;
        float* out = (l & 1) ? act_a : act_b;
        const bool last = l == L - 1;
        for (int jbase = 0; jbase < N; jbase += PASS) {
            double acc[JT];
#pragma unroll
            for (int t = 0; t < JT; ++t) {
                const int j = jbase + grp * JT + t;
                acc[t] = j < N ? (double)bias[j] : 0.0;
            }
            float pre[PRE];
            auto prefetch = [&](int k0) {                            // element e of the tile: input k0 + (e & 31) of output jbase + (e >> 5)
#pragma unroll
                for (int q = 0; q < PRE; ++q) {
                    const int e = tid + q * THREADS, j = jbase + e / KC, k = k0 + (e & (KC - 1));
                    pre[q] = (j < N && k < K) ? W[(size_t)j * K + k] : 0.0f;
                }
            };
            prefetch(0);
            for (int k0 = 0; k0 < K; k0 += KC) {
                __syncthreads();                                     // the tile's readers are done; the first of a layer: its inputs are written
#pragma unroll
                for (int q = 0; q < PRE; ++q) {
                    const int e = tid + q * THREADS;
                    wt[(e & (KC - 1)) * WS + e / KC] = pre[q];
                }
                __syncthreads();
                if (k0 + KC < K) prefetch(k0 + KC);
                const int kc = K - k0 < KC ? K - k0 : KC;
                auto steps = [&](int i) {
                    const float xv = in[(k0 + i) * AS + r];
                    const float* wrow = wt + i * WS + grp * JT;
#pragma unroll
                    for (int t = 0; t < JT; ++t) acc[t] = mlp_step(acc[t], (double)wrow[t], xv);
                };
                if (kc == KC) {                                      // a whole tile: the LDS reads of BATCH inputs issued together, then their steps
#pragma unroll
                    for (int i0 = 0; i0 < KC; i0 += BATCH) {
                        float xv[BATCH];
                        float w[BATCH][JT];
#pragma unroll
                        for (int i = 0; i < BATCH; ++i) {
                            xv[i] = in[(k0 + i0 + i) * AS + r];
#pragma unroll
                            for (int t = 0; t < JT; ++t) w[i][t] = wt[(i0 + i) * WS + grp * JT + t];
                        }
#pragma unroll
                        for (int i = 0; i < BATCH; ++i) {
#pragma unroll
                            for (int t = 0; t < JT; ++t) acc[t] = mlp_step(acc[t], (double)w[i][t], xv[i]);
                        }
                    }
                } else {
                    for (int i = 0; i < kc; ++i) steps(i);
                }
            }
#pragma unroll
            for (int t = 0; t < JT; ++t) {                           // outputs past N ran on zero weights and are dropped
                const int j = jbase + grp * JT + t;
                if (j < N) {
                    const float v = last ? mlp_last(acc[t]) : mlp_hidden(acc[t]);
                    out[j * AS + r] = v;
                    park(l, j, r, v);
                }
            }
        }
    }
    __syncthreads();
}

// where the last of L layers wrote
__device__ __forceinline__ const float* mlp_result(int32_t L, const float* act_a, const float* act_b) { return (L & 1) ? act_b : act_a; }

}  // namespace snac_mlp_dev
