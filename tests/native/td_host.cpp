// td_host.cpp -- the per-sample function k_td_loss runs (snac_amd/csrc/td_rule.h), compiled for the host as it stands, with a C++
// restatement of both stages of the batch reduction: tests/test_qloss_host.py builds this file into a shared object with the system
// compiler and -ffp-contract=off and compares every output's bytes with the numpy statement of the rule.  The loops below are
// k_td_loss's and k_td_reduce's bodies with the lane a loop index; snac_td_loss's conventions for NULL pointers hold.
// With -DTD_HOST_MAIN the file is a program: cases with actions out of range, for a run under the host sanitizers.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "td_rule.h"

namespace {

using namespace snac_spec;

// the xor butterfly over 64 values: every j of a step together
double butterfly(const double* v) {
    double u[64], t[64];
    for (int j = 0; j < 64; ++j) u[j] = v[j];
    for (int off = 32; off >= 1; off >>= 1) {
        for (int j = 0; j < 64; ++j) t[j] = u[j] + u[j ^ off];
        for (int j = 0; j < 64; ++j) u[j] = t[j];
    }
    return u[0];
}

template <int A, bool NEXT>
int run(int32_t B, const float* q, const int64_t* action, const float* y, const float* q_next, const float* q_select, const float* ret,
        const float* discount, const float* weight, const TdParams& p, float* loss, float* priority, float* y_out, float* grad_q, double* stats,
        float* mean_loss, double* partials) {
    int bad_rows = 0;
    const long long W = ((long long)B + 63) / 64;
    for (long long w = 0; w < W; ++w) {
        double u[TD_STATS][64];
        for (int j = 0; j < 64; ++j) {
            const long long i = w * 64 + j;
            for (int k = 0; k < TD_STATS; ++k) u[k][j] = 0.0;
            if (i >= B) continue;
            const size_t at = (size_t)i * A;
            float qr[A], nxt[A], sel[A];
            for (int a = 0; a < A; ++a) {
                qr[a] = q[at + a];
                nxt[a] = NEXT ? q_next[at + a] : 0.0f;
                sel[a] = NEXT && q_select ? q_select[at + a] : nxt[a];
            }
            const TdSample<A> o = td_sample<A, NEXT>(qr, action[i], sel, nxt, NEXT ? ret[i] : 0.0f, NEXT ? discount[i] : 0.0f, NEXT ? 0.0f : y[i],
                                                     weight ? weight[i] : 1.0f, weight != nullptr, p);
            bad_rows += o.bad;
            if (loss) loss[i] = o.loss;
            if (priority) priority[i] = o.priority;
            if (y_out) y_out[i] = o.y;
            if (grad_q)
                for (int a = 0; a < A; ++a) grad_q[at + a] = o.grad[a];
            for (int k = 0; k < TD_STATS; ++k) u[k][j] = o.u[k];
        }
        if (stats)
            for (int k = 0; k < TD_STATS; ++k) partials[w * TD_STATS + k] = butterfly(u[k]);
    }
    if (stats) {
        for (int k = 0; k < TD_STATS; ++k) {
            double t[64];
            for (int j = 0; j < 64; ++j) t[j] = td_lane_sum(partials, W, j, k);
            const double s = butterfly(t);
            stats[k] = k == TD_GOOD ? s : s / (double)B;
        }
        if (mean_loss) mean_loss[0] = (float)stats[TD_TOTAL];
    }
    return bad_rows;
}

}  // namespace

// -> the number of bad samples, or -1 for an unsupported num_actions.  y given: mode Y; else mode NEXT
extern "C" int td_host(int32_t B, int32_t num_actions, const float* q, const int64_t* action, const float* y, const float* q_next,
                       const float* q_select, const float* ret, const float* discount, const float* weight, double delta, double scale, float* loss,
                       float* priority, float* y_out, float* grad_q, double* stats, float* mean_loss, double* partials) {
    const TdParams p{delta, scale};
#define TD_HOST_RUN(A)                                                                                                                          \
    return y ? run<A, false>(B, q, action, y, q_next, q_select, ret, discount, weight, p, loss, priority, y_out, grad_q, stats, mean_loss, partials) \
             : run<A, true>(B, q, action, y, q_next, q_select, ret, discount, weight, p, loss, priority, y_out, grad_q, stats, mean_loss, partials)
    switch (num_actions) {
        case 3: TD_HOST_RUN(3);
        case 5: TD_HOST_RUN(5);
        case 8: TD_HOST_RUN(8);
        default: return -1;
    }
#undef TD_HOST_RUN
}

#ifdef TD_HOST_MAIN
#include <cstdio>

// One case per action count whose actions run from -2 to A + 1 and beyond (and the int64 extremes), through ragged waves and a second
// stage of more than 64 partials, in exactly sized heap arrays: an action that indexed anything, or a lane past B that wrote, shows
// under -fsanitize=address,undefined.  Prints the counts; exit status 1 if a count is off.
int main() {
    int status = 0;
    for (int A : {3, 5, 8}) {
        for (int32_t B : {1, 65, 4097}) {
            const long long W = ((long long)B + 63) / 64;
            std::vector<float> q((size_t)B * A), qn((size_t)B * A), qs((size_t)B * A), y(B), ret(B), discount(B), weight(B), loss(B), prio(B), yo(B),
                gq((size_t)B * A);
            std::vector<int64_t> action(B);
            std::vector<double> stats(TD_STATS), partials((size_t)W * TD_STATS);
            int want_bad = 0;
            for (int32_t i = 0; i < B; ++i) {
                for (int a = 0; a < A; ++a) {
                    q[(size_t)i * A + a] = 0.25f * (float)((i * 7 + a * 3) % 11) - 1.0f;
                    qn[(size_t)i * A + a] = 0.5f * (float)((i * 5 + a * 7) % 13) - 2.0f;
                    qs[(size_t)i * A + a] = 0.125f * (float)((i * 3 + a * 5) % 17);
                }
                const int64_t special[4] = {INT64_MIN, INT64_MAX, (int64_t)1 << 32, -((int64_t)1 << 32)};
                action[i] = i % 13 == 12 ? special[(i / 13) % 4] : (int64_t)(i % (A + 4)) - 2;      // -2 .. A + 1
                want_bad += action[i] < 0 || action[i] >= A;
                y[i] = 0.3f * (float)(i % 7) - 1.0f;
                ret[i] = 0.1f * (float)(i % 17);
                discount[i] = i % 9 ? 0.97f : 0.0f;
                weight[i] = 0.1f * (float)(1 + i % 10);
            }
            for (int mode = 0; mode < 3; ++mode) {                   // Y, NEXT, NEXT with q_select
                for (double delta : {0.0, 1.0}) {
                    float mean = 0.0f;
                    const int bad = td_host(B, A, q.data(), action.data(), mode == 0 ? y.data() : nullptr, mode ? qn.data() : nullptr,
                                            mode == 2 ? qs.data() : nullptr, mode ? ret.data() : nullptr, mode ? discount.data() : nullptr,
                                            mode == 1 ? nullptr : weight.data(), delta, 1.0 / B, loss.data(), prio.data(), yo.data(), gq.data(), stats.data(),
                                            &mean, partials.data());
                    std::printf("A %d B %d mode %d delta %g: bad %d (want %d), good %.0f, mean loss %.9g\n", A, (int)B, mode, delta, bad, want_bad,
                                stats[TD_GOOD], (double)mean);
                    if (bad != want_bad || stats[TD_GOOD] != (double)(B - want_bad)) status = 1;
                }
            }
        }
    }
    return status;
}
#endif
