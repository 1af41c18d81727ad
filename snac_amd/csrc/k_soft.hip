// k_soft.hip -- snac_soft_value: discrete SAC's soft state value, TD target, entropy and the gradient of the actor loss with respect to
// the logits, from one softmax and one elementwise minimum per sample, in one launch.  include/snac_hip.h, "Soft values (discrete SAC)",
// has the rule; soft_rule.h states it per sample, for this kernel and for the host.
#include <cmath>
#include <cstddef>

#include "snac_units.h"
#include "soft_rule.h"

// lane = sample, blocks of one wave, as k_policy_act: the outputs of a wave are coalesced spans of v / y / entropy and one span of 64 * A
// floats of grad, and nothing crosses lanes.  A lane reads its rows of logits, q1 and q2 as 3A strided dword loads, and ret and discount,
// all issued before the first use; a wave's rows are one contiguous span per input, so every line is used whole, and the inputs are
// aligned as floats only (rows of 12 and 20 bytes), so nothing wider.  alpha[0] is one wave-uniform load.  All arrays are indexed by
// unrolled constants: they live in registers, there is no scratch and no LDS.  The float64 series of the A exponentials outweigh the
// 6 MB that 65 536 samples of 8 actions read.
namespace {

using namespace snac_detail;
using namespace snac_spec;

struct SoftArgs {
    int32_t B;
    const float* logits;
    const float* q1;
    const float* q2;
    const float* alpha;
    const float* ret;
    const float* discount;
    double scale;
    float* v;
    float* y;
    float* entropy;
    float* grad;
    int32_t* bad_rows;
};

template <int A, bool TWO_Q>
__global__ __launch_bounds__(64) void k_soft_value(const SoftArgs g) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= g.B) return;
    const bool use_q = g.v || g.y || g.grad;                         // uniform: kernel arguments
    const bool want_y = g.y != nullptr;
    const size_t at = (size_t)i * A;
    float l[A], q1[A], q2[A];
#pragma unroll
    for (int a = 0; a < A; ++a) l[a] = g.logits[at + a];             // every load of the lane on its way before the first use
#pragma unroll
    for (int a = 0; a < A; ++a) q1[a] = use_q ? g.q1[at + a] : 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) q2[a] = TWO_Q ? g.q2[at + a] : 0.0f;
    const float ret = want_y ? g.ret[i] : 0.0f, discount = want_y ? g.discount[i] : 0.0f;
    const float alpha = use_q ? g.alpha[0] : 0.0f;

    const SoftSample<A> o = soft_sample<A, TWO_Q>(l, q1, q2, alpha, ret, discount, use_q, want_y, g.scale);
    if (o.bad && g.bad_rows) atomicAdd(g.bad_rows, 1);
    if (g.v) g.v[i] = o.v;
    if (g.y) g.y[i] = o.y;
    if (g.entropy) g.entropy[i] = o.entropy;
    if (g.grad) {
#pragma unroll
        for (int a = 0; a < A; ++a) g.grad[at + a] = o.grad[a];
    }
}

}  // namespace

extern "C" int snac_soft_value(int32_t B, int32_t num_actions, const float* logits, const float* q1, const float* q2, const float* alpha,
                               const float* ret, const float* discount, double scale, float* v, float* y, float* entropy, float* grad,
                               int32_t* bad_rows, void* stream) {
    using namespace snac_detail;
    if (!logits) return fail(SNAC_ERR_ARG, "null logits");
    if (B < 1) return fail(SNAC_ERR_ARG, "B must be >= 1");
    if (!std::isfinite(scale)) return fail(SNAC_ERR_ARG, "scale must be finite");
    const bool use_q = v || y || grad;
    if (use_q && (!q1 || !alpha)) return fail(SNAC_ERR_ARG, "q1 and alpha are needed for v, y and grad");
    if (y && (!ret || !discount)) return fail(SNAC_ERR_ARG, "ret and discount are needed for y");
    if (!y && (ret || discount)) return fail(SNAC_ERR_ARG, "ret and discount belong to y");
    return by_actions(num_actions, [&](auto actions) -> int {
        constexpr int A = decltype(actions)::value;
        if (!use_q && !entropy) return SNAC_OK;                      // nothing asked for
        const SoftArgs g{B, logits, q1, q2, alpha, ret, discount, scale, v, y, entropy, grad, bad_rows};
        g_kernel = "k_soft_value";
        const dim3 grid((unsigned)(((long long)B + 63) / 64)), block(64);
        const hipStream_t s = (hipStream_t)stream;
        if (use_q && q2) hipLaunchKernelGGL((k_soft_value<A, true>), grid, block, 0, s, g);
        else hipLaunchKernelGGL((k_soft_value<A, false>), grid, block, 0, s, g);
        return launched("snac_soft_value");
    });
}
