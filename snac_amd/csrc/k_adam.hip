// k_adam.hip -- the optimiser step of the device network: snac_mlp_adam_step (the global gradient norm, the clip, Adam and the slow copy
// of a target network, from one flat gradient into the parameters where they lie, as two launches on the caller's stream) and
// snac_mlp_lerp (the target's move alone).  include/snac_hip.h, "Optimiser step of the device network", has the rule; adam_rule.h states
// it per parameter, for these kernels and for the host.  These are the only kernels that write the arrays a snac_mlp points to.
//
//   k_adam_sumsq   a wave per 64 consecutive flat indices (four waves a block): the squares in float64, batch_sum.h's butterfly, lane 0
//                  writes the wave's partial.
//   k_adam_update  a block of 256 threads takes ITEMS * 256 consecutive flat indices.  Wave 0 of EVERY block redoes stage two from the
//                  partials -- lane j adds partials[j], partials[j + 64], .. in ascending order, the loads of eight of them issued
//                  together, then the butterfly -- which is the same order and so the same bits in every block: no grid synchronisation
//                  and no third launch.  ss reaches the other waves through LDS (one barrier).  A bad step (ss not finite) returns
//                  before any store but block 0's count and norm_out.  A lane finds the array of its flat index in a table of at most
//                  eight segments (per layer the weights, then the bias) passed by value: compares over unrolled constants, never a
//                  register array indexed by a variable, so no scratch.
//   k_mlp_lerp     the same table walk, the target's rule on theta as it is.
// Scalar 4-byte accesses to the float32 arrays: only 4-byte alignment is assumed.  Both launches of a step run at the launch rate (P is
// at most about 2.8 x 10^5): the point is the launch count and the stated bytes, not bandwidth.  DESIGN.md 3.18 has the registers and
// the measured times.
#include <climits>
#include <cmath>
#include <cstddef>

#include "snac_units.h"
#include "batch_sum.h"
#include "mlp_rule.h"
#include "mlp_grad_rule.h"
#include "adam_rule.h"

namespace {

using namespace snac_detail;
using namespace snac_spec;

constexpr int THREADS = 256, ITEMS = 4, SEGS = 2 * MLP_MAX_LAYERS, BATCH = 8;

// the flat layout as segments: segment s begins at flat index off[s] in the array ptr[s]; off of an unused segment is INT32_MAX
struct Segments {
    int32_t off[SEGS];
    float* net[SEGS];
    float* tgt[SEGS];                                                // all NULL without a target
};

struct AdamArgs {
    Segments seg;
    int32_t P, W;
    const float* grad;
    float* m;
    float* v;
    AdamStep step;
    double max_norm, tau;
    int32_t has_target;
    double* norm_out;
    const double* partials;
    int32_t* bad_steps;
};

// the place of flat index p: its segment's array and where the segment begins
struct Place { float* net; float* tgt; int32_t start; };
__device__ __forceinline__ Place place_of(const Segments& seg, int32_t p) {
    Place at{seg.net[0], seg.tgt[0], 0};
#pragma unroll
    for (int s = 1; s < SEGS; ++s) {
        if (p >= seg.off[s]) at.net = seg.net[s], at.tgt = seg.tgt[s], at.start = seg.off[s];
    }
    return at;
}

__global__ __launch_bounds__(THREADS) void k_adam_sumsq(const float* grad, int32_t P, int32_t W, double* partials) {
#pragma clang fp contract(off)
    const int32_t w = (int32_t)blockIdx.x * (THREADS / 64) + ((int32_t)threadIdx.x >> 6);
    if (w >= W) return;                                              // the whole wave
    const int32_t p = 64 * w + ((int32_t)threadIdx.x & 63);
    double u = 0.0;
    if (p < P) {
        const double g = (double)grad[p];
        u = g * g;
    }
    u = wave_sum(u);
    if ((threadIdx.x & 63) == 0) partials[w] = u;
}

__global__ __launch_bounds__(THREADS) void k_adam_update(const AdamArgs a) {
#pragma clang fp contract(off)
    __shared__ double ss_shared;
    const int tid = threadIdx.x;
    if (tid < 64) {                                                  // stage two, in every block: the same order, the same bits
        double s = 0.0;
        for (int32_t w0 = tid; w0 < a.W; w0 += 64 * BATCH) {
            double t[BATCH];
#pragma unroll
            for (int q = 0; q < BATCH; ++q) {
                const int32_t w = w0 + 64 * q;
                t[q] = w < a.W ? a.partials[w] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < BATCH; ++q) {
                const double next = s + t[q];
                s = w0 + 64 * q < a.W ? next : s;
            }
        }
        s = wave_sum(s);
        if (tid == 0) ss_shared = s;
    }
    __syncthreads();
    const double ss = ss_shared;
    const bool bad = adam_bad(ss);                                   // uniform over the grid
    const double coef = bad ? 0.0 : adam_coef(ss, a.max_norm);
    if (blockIdx.x == 0 && tid == 0) {
        if (a.norm_out) a.norm_out[0] = adam_norm(ss), a.norm_out[1] = coef;
        if (bad && a.bad_steps) atomicAdd(a.bad_steps, 1);
    }
    if (bad) return;
    const bool has_target = a.has_target != 0;                       // uniform
    // every load of the lane's ITEMS parameters on its way before the first store (a flat index belongs to one lane, and the arrays
    // are distinct: no store of this launch is read by it)
    float* pt[ITEMS];
    float* tt[ITEMS];
    float th[ITEMS], gr[ITEMS], mo[ITEMS], ve[ITEMS], tg[ITEMS];
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
        const int32_t p = ((int32_t)blockIdx.x * ITEMS + q) * THREADS + tid;
        const bool in = p < a.P;
        const int32_t pp = in ? p : 0;                               // a lane past P reads index 0 and drops it
        const Place at = place_of(a.seg, pp);
        pt[q] = at.net + (pp - at.start);
        tt[q] = has_target ? at.tgt + (pp - at.start) : nullptr;
        th[q] = *pt[q], gr[q] = a.grad[pp], mo[q] = a.m[pp], ve[q] = a.v[pp];
        tg[q] = has_target ? *tt[q] : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
        const int32_t p = ((int32_t)blockIdx.x * ITEMS + q) * THREADS + tid;
        if (p >= a.P) continue;
        const AdamParam o = adam_param(th[q], gr[q], mo[q], ve[q], coef, a.step);
        a.m[p] = o.m;
        a.v[p] = o.v;
        *pt[q] = o.theta;
        if (has_target) *tt[q] = lerp_param(tg[q], o.theta, a.tau);
    }
}

__global__ __launch_bounds__(THREADS) void k_mlp_lerp(const Segments seg, int32_t P, double tau) {
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
        const int32_t p = ((int32_t)blockIdx.x * ITEMS + q) * THREADS + (int32_t)threadIdx.x;
        if (p >= P) continue;
        const Place at = place_of(seg, p);
        const int32_t i = p - at.start;
        at.tgt[i] = lerp_param(at.tgt[i], at.net[i], tau);
    }
}

// the checks of a target beside its network: dims, pointers, their alignment, no array shared with the network, tau
int target_check(const snac_mlp* target, const snac_mlp* net, double tau) {
    if (target->layers != net->layers) return fail(SNAC_ERR_ARG, "the target must have the network's layers");
    for (int l = 0; l <= net->layers; ++l)
        if (target->dim[l] != net->dim[l]) return fail(SNAC_ERR_ARG, "the target must have the network's dims");
    for (int l = 0; l < net->layers; ++l) {
        if (!target->w[l] || !target->b[l]) return fail(SNAC_ERR_ARG, "null weights / bias of a layer of the target");
        if ((uintptr_t)target->w[l] % 4 || (uintptr_t)target->b[l] % 4) return fail(SNAC_ERR_ARG, "the target's weights and biases must be 4-byte aligned");
    }
    for (int l = 0; l < net->layers; ++l)
        for (int k = 0; k < net->layers; ++k)
            if (target->w[l] == net->w[k] || target->w[l] == net->b[k] || target->b[l] == net->w[k] || target->b[l] == net->b[k])
                return fail(SNAC_ERR_ARG, "the target shares an array with the network");
    if (!(tau > 0.0 && tau <= 1.0)) return fail(SNAC_ERR_ARG, "tau must be in (0, 1]");
    return SNAC_OK;
}

// the segments of the network (and of the target, or NULLs); -> P.  These entry points write the arrays the descriptors point to.
int32_t segments_of(const snac_mlp* net, const snac_mlp* target, Segments* seg) {
    int32_t off[MLP_MAX_LAYERS];
    const int32_t P = mlp_grad_layout(net->layers, net->dim, off);
    for (int s = 0; s < SEGS; ++s) seg->off[s] = INT32_MAX, seg->net[s] = nullptr, seg->tgt[s] = nullptr;
    for (int l = 0; l < net->layers; ++l) {
        seg->off[2 * l] = off[l];
        seg->off[2 * l + 1] = off[l] + net->dim[l + 1] * net->dim[l];
        seg->net[2 * l] = const_cast<float*>(net->w[l]);
        seg->net[2 * l + 1] = const_cast<float*>(net->b[l]);
        if (target) {
            seg->tgt[2 * l] = const_cast<float*>(target->w[l]);
            seg->tgt[2 * l + 1] = const_cast<float*>(target->b[l]);
        }
    }
    return P;
}

unsigned blocks_of(int32_t P) { return (unsigned)((P + THREADS * ITEMS - 1) / (THREADS * ITEMS)); }

}  // namespace

extern "C" int snac_mlp_adam_step(const snac_mlp* net, const float* grad, float* m, float* v, double lr, double beta1, double beta2, double eps,
                                  double bias1, double bias2, double max_norm, const snac_mlp* target, double tau, double* norm_out,
                                  double* partials, int32_t* bad_steps, void* stream) {
    using namespace snac_detail;
    if (int rc = mlp_net_check(net)) return rc;
    if (!grad || !m || !v) return fail(SNAC_ERR_ARG, "null grad / m / v");
    if ((uintptr_t)grad % 4 || (uintptr_t)m % 4 || (uintptr_t)v % 4) return fail(SNAC_ERR_ARG, "grad, m and v must be 4-byte aligned");
    if (grad == m || grad == v || m == v) return fail(SNAC_ERR_ARG, "grad, m and v must be distinct arrays");
    if (!partials) return fail(SNAC_ERR_ARG, "null partials");
    if ((uintptr_t)partials % 8) return fail(SNAC_ERR_ARG, "partials must be 8-byte aligned");
    if ((uintptr_t)norm_out % 8) return fail(SNAC_ERR_ARG, "norm_out must be 8-byte aligned");
    if ((uintptr_t)bad_steps % 4) return fail(SNAC_ERR_ARG, "bad_steps must be 4-byte aligned");
    if (!std::isfinite(lr) || lr < 0.0) return fail(SNAC_ERR_ARG, "lr must be finite and >= 0");
    if (!std::isfinite(eps) || eps < 0.0) return fail(SNAC_ERR_ARG, "eps must be finite and >= 0");
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return fail(SNAC_ERR_ARG, "beta1 must be in [0, 1)");
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return fail(SNAC_ERR_ARG, "beta2 must be in [0, 1)");
    if (!(bias1 > 0.0 && bias1 <= 1.0)) return fail(SNAC_ERR_ARG, "bias1 must be in (0, 1]");
    if (!(bias2 > 0.0 && bias2 <= 1.0)) return fail(SNAC_ERR_ARG, "bias2 must be in (0, 1]");
    if (!std::isfinite(max_norm) || max_norm < 0.0) return fail(SNAC_ERR_ARG, "max_norm must be finite and >= 0 (0: no clip)");
    if (target)
        if (int rc = target_check(target, net, tau)) return rc;

    AdamArgs a{};
    a.P = segments_of(net, target, &a.seg);
    a.W = (a.P + 63) / 64;
    a.grad = grad, a.m = m, a.v = v;
    a.step = snac_spec::adam_step_of(lr, beta1, beta2, eps, bias1, bias2);
    a.max_norm = max_norm, a.tau = target ? tau : 1.0, a.has_target = target != nullptr;
    a.norm_out = norm_out, a.partials = partials, a.bad_steps = bad_steps;

    const hipStream_t s = (hipStream_t)stream;
    g_kernel = "k_adam_sumsq";
    hipLaunchKernelGGL(k_adam_sumsq, dim3((unsigned)((a.W + THREADS / 64 - 1) / (THREADS / 64))), dim3(THREADS), 0, s, grad, a.P, a.W, partials);
    if (int rc = launched("snac_mlp_adam_step")) return rc;          // each launch's own error, under the kernel snac_last_kernel() names
    g_kernel = "k_adam_update";
    hipLaunchKernelGGL(k_adam_update, dim3(blocks_of(a.P)), dim3(THREADS), 0, s, a);
    return launched("snac_mlp_adam_step");
}

extern "C" int snac_mlp_lerp(const snac_mlp* target, const snac_mlp* net, double tau, void* stream) {
    using namespace snac_detail;
    if (int rc = mlp_net_check(net)) return rc;
    if (!target) return fail(SNAC_ERR_ARG, "null target");
    if (int rc = target_check(target, net, tau)) return rc;
    Segments seg;
    const int32_t P = segments_of(net, target, &seg);
    g_kernel = "k_mlp_lerp";
    hipLaunchKernelGGL(k_mlp_lerp, dim3(blocks_of(P)), dim3(THREADS), 0, (hipStream_t)stream, seg, P, tau);
    return launched("snac_mlp_lerp");
}
