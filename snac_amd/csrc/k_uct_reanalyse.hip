// k_uct_reanalyse.hip -- Reanalyse on the UCT trees of k_uct.hip: snac_uct_save_roots (the roots' records into a caller's array: the state
// a self-play ring keeps per move), snac_uct_load_roots (trees started over from stored records), snac_uct_store_targets (the roots' policy
// and value into indexed ring entries) and snac_uct_returns_nstep (n-step value targets that bootstrap from the ring's values).
// include/snac_hip.h, "Reanalyse", has the semantics.
#include <cmath>
#include <cstddef>

#include "snac_units.h"
#include "uct_dev.h"

// Four small, latency-bound kernels beside those of k_uct_play.hip, with its shapes.  save is lane = piece: the B root records leave as
// one run of 16-byte pieces.  load is wave = tree, as k_uct_restart: the record (8 or 56 pieces) is read once and stored twice, the
// statistics row (16 pieces) is written whole, one piece per lane.  store and returns are lane = tree, as k_uct_pick and k_uct_returns.
namespace {

struct UctSave {
    const uint4* records;
    uint4* out;
    int32_t B, cap;
};

template <int RP>                                                    // 16-byte pieces of a node record (8: 1D / 2D, 56: 3D)
__global__ __launch_bounds__(256) void k_uct_save_roots(const UctSave v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // piece i of the output: B * RP < 2^31 * 56
    if (i >= (long long)v.B * RP) return;
    const int b = (int)(i / RP), p = (int)(i % RP);
    v.out[i] = v.records[(size_t)b * v.cap * RP + p];
}

struct UctLoad {
    uint4* stats;
    uint4* records;
    const uint4* src;
    const int32_t* index;
    int32_t B, cap, src_rows;
    int32_t* used;
};

constexpr int LOAD_WAVES = 4;                                        // trees per workgroup

template <int RP>
__global__ __launch_bounds__(64 * LOAD_WAVES) void k_uct_load_roots(const UctLoad v) {
    static_assert(RP <= 64, "a record is at most one piece per lane");
    const int lane = (int)threadIdx.x & 63;
    const int b = (int)blockIdx.x * LOAD_WAVES + ((int)threadIdx.x >> 6);
    if (b >= v.B) return;
    const int s = v.index ? min(max(v.index[b], 0), v.src_rows - 1) : b;
    const uint4* const from = v.src + (size_t)s * RP;
    const size_t root = (size_t)b * v.cap, scratch = (size_t)v.B * v.cap + b;
    const uint32_t word0 = from[0].x;                                // every lane: the record's position and flags (one line, one trip)
    if (lane < RP) {
        const uint4 piece = from[lane];
        v.records[root * RP + lane] = piece;
        v.records[scratch * RP + lane] = piece;
    }
    if (lane < PIECES) {
        const bool term = ((word0 >> 16) & (uint32_t)SNAC_FLAG_NEED_RESET) != 0;
        const uint4 none = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu), zero = make_uint4(0u, 0u, 0u, 0u);
        v.stats[root * PIECES + lane] =                              // the row k_uct_restart writes
            lane < P_VISITS ? none : lane == P_HDR ? make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, term ? 1u : 0u, 0u) : zero;
    }
    if (lane == 0) v.used[b] = 1;
}

struct UctStore {
    const uint4* stats;
    int32_t B, cap, entries;
    const int32_t* index;
    const float* policy;
    float* pi;
    float* value;
    int32_t* refreshed;
};

template <int A>
__global__ __launch_bounds__(64) void k_uct_store_targets(const UctStore v) {
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= v.B) return;
    const int e = v.index[b];
    if (e < 0 || e >= v.entries) return;                             // no entry for this tree
    const uint4* const rec = v.stats + (size_t)b * v.cap * PIECES;
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    uint4 n0 = zero4, n1 = zero4;
    if (!v.policy) { n0 = rec[P_VISITS]; n1 = rec[P_VISITS + 1]; }   // line 0 only for the visit distribution
    const uint4 hdr = rec[P_HDR], own = rec[P_OWN];
    const int was = v.refreshed[e];
    float p[A];
    if (v.policy) {
#pragma unroll
        for (int a = 0; a < A; ++a) p[a] = v.policy[(size_t)b * A + a];
    } else {                                                         // k_uct_pick's pi
        const uint32_t raw[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
        uint32_t n[A];
        uint64_t total = 0;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            n[a] = (uint32_t)max((int)raw[a], 0);
            total += n[a];
        }
#pragma unroll
        for (int a = 0; a < A; ++a) p[a] = total ? (float)((double)n[a] / (double)total) : 0.f;
    }
#pragma unroll
    for (int a = 0; a < A; ++a) v.pi[(size_t)e * A + a] = p[a];
    const int visits = (int)hdr.w;                                   // k_uct_pick's value
    v.value[e] = visits ? (float)(__hiloint2double((int)own.y, (int)own.x) / (double)visits) : 0.f;
    v.refreshed[e] = was + 1;
}

struct UctNstep {
    int32_t B, cap_moves, first, count, n;
    double gamma;
    const float* reward;
    const uint8_t* done;
    const float* value;
    const float* bootstrap;
    float* z;
};

__global__ __launch_bounds__(64) void k_uct_returns_nstep(const UctNstep v) {
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= v.B) return;
    const double boot = v.bootstrap ? (double)v.bootstrap[b] : 0.0;
    for (int i = 0; i < v.count; ++i) {                              // the specification's double loop: slot i's window is [i, e)
        const int e = v.n >= v.count - i ? v.count : i + v.n;
        double g = e < v.count ? (double)v.value[(size_t)(((long long)v.first + e) % v.cap_moves) * v.B + b] : boot;
        int slot = (int)(((long long)v.first + e - 1) % v.cap_moves);
        size_t at = 0;
        for (int j = e - 1; j >= i; --j) {                           // slot e - 1 back to slot i
            at = (size_t)slot * v.B + b;
            const double r = (double)v.reward[at];
            const bool d = v.done[at] != 0;
            {
#pragma clang fp contract(off)                                      // no fma: product and sum each rounded, as k_uct_returns
                const double t = v.gamma * g;
                g = r + (d ? 0.0 : t);
            }
            slot = slot == 0 ? v.cap_moves - 1 : slot - 1;
        }
        v.z[at] = (float)g;                                          // e > i: the inner loop ran, `at` is slot i
    }
}

// records / record_bytes / record_rows as snac_uct_restart checks them
int records_check(const void* records, int32_t record_bytes, int32_t record_rows, int32_t B, int32_t cap) {
    using namespace snac_detail;
    if (!records) return fail(SNAC_ERR_ARG, "null records");
    if (((uintptr_t)records & 127) != 0) return fail(SNAC_ERR_ARG, "records must be 128-byte aligned");
    if (record_bytes != 128 && record_bytes != 896) return fail(SNAC_ERR_ARG, "record_bytes must be 128 or 896");
    if ((long long)B * ((long long)cap + 1) > record_rows) return fail(SNAC_ERR_ARG, "B * (cap + 1) rows exceed record_rows");
    return SNAC_OK;
}

}  // namespace

extern "C" {

int snac_uct_save_roots(int32_t B, int32_t cap, const void* records, int32_t record_bytes, int32_t record_rows, void* out, void* stream) {
    using namespace snac_detail;
    if (B < 1) return fail(SNAC_ERR_ARG, "B must be >= 1");
    if (cap < 1) return fail(SNAC_ERR_ARG, "cap must be >= 1");
    if ((long long)B * ((long long)cap + 1) > 0x7FFFFFFFll) return fail(SNAC_ERR_ARG, "B * (cap + 1) rows exceed int32");
    if (int rc = records_check(records, record_bytes, record_rows, B, cap)) return rc;
    if (!out) return fail(SNAC_ERR_ARG, "null out");
    if (((uintptr_t)out & 127) != 0) return fail(SNAC_ERR_ARG, "out must be 128-byte aligned");
    const UctSave v{(const uint4*)records, (uint4*)out, B, cap};
    const long long pieces = (long long)B * (record_bytes / 16);
    const dim3 grid((unsigned)((pieces + 255) / 256));
    g_kernel = "k_uct_save_roots";
    if (record_bytes == 128) hipLaunchKernelGGL((k_uct_save_roots<8>), grid, dim3(256), 0, (hipStream_t)stream, v);
    else hipLaunchKernelGGL((k_uct_save_roots<56>), grid, dim3(256), 0, (hipStream_t)stream, v);
    return launched("snac_uct_save_roots");
}

int snac_uct_load_roots(int32_t num_actions, snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, void* records, int32_t record_bytes,
                        int32_t record_rows, const void* src, int32_t src_rows, const int32_t* index, int32_t* used, void* stream) {
    using namespace snac_detail;
    if (int rc = play_check(num_actions, stats, stats_rows, B, cap)) return rc;
    if (int rc = records_check(records, record_bytes, record_rows, B, cap)) return rc;
    if (!src) return fail(SNAC_ERR_ARG, "null src");
    if (((uintptr_t)src & 127) != 0) return fail(SNAC_ERR_ARG, "src must be 128-byte aligned");
    if (src_rows < 1) return fail(SNAC_ERR_ARG, "src_rows must be >= 1");
    if (!index && src_rows < B) return fail(SNAC_ERR_ARG, "src_rows must be >= B without an index");
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)src_rows * (uintptr_t)record_bytes;
    const uintptr_t r0 = (uintptr_t)records, r1 = r0 + (uintptr_t)record_rows * (uintptr_t)record_bytes;
    if (s0 < r1 && r0 < s1) return fail(SNAC_ERR_ARG, "src must not overlap records");
    if (!used) return fail(SNAC_ERR_ARG, "null used");
    const UctLoad v{(uint4*)stats, (uint4*)records, (const uint4*)src, index, B, cap, src_rows, used};
    const dim3 grid((unsigned)((B + LOAD_WAVES - 1) / LOAD_WAVES)), block(64 * LOAD_WAVES);
    g_kernel = "k_uct_load_roots";
    if (record_bytes == 128) hipLaunchKernelGGL((k_uct_load_roots<8>), grid, block, 0, (hipStream_t)stream, v);
    else hipLaunchKernelGGL((k_uct_load_roots<56>), grid, block, 0, (hipStream_t)stream, v);
    return launched("snac_uct_load_roots");
}

int snac_uct_store_targets(int32_t num_actions, const snac_uct_node* stats, int32_t stats_rows, int32_t B, int32_t cap, const int32_t* index,
                           int32_t entries, const float* policy, float* pi, float* value, int32_t* refreshed, void* stream) {
    using namespace snac_detail;
    if (int rc = play_check(num_actions, stats, stats_rows, B, cap)) return rc;
    if (!index) return fail(SNAC_ERR_ARG, "null index");
    if (entries < 0) return fail(SNAC_ERR_ARG, "entries must be >= 0");
    if (!pi || !value || !refreshed) return fail(SNAC_ERR_ARG, "null ring array (pi / value / refreshed)");
    if (entries == 0) return SNAC_OK;                                // no entry to write
    const UctStore v{(const uint4*)stats, B, cap, entries, index, policy, pi, value, refreshed};
    const dim3 grid((unsigned)((B + 63) / 64));
    g_kernel = "k_uct_store_targets";
    if (num_actions == 3) hipLaunchKernelGGL((k_uct_store_targets<3>), grid, dim3(64), 0, (hipStream_t)stream, v);
    else if (num_actions == 5) hipLaunchKernelGGL((k_uct_store_targets<5>), grid, dim3(64), 0, (hipStream_t)stream, v);
    else hipLaunchKernelGGL((k_uct_store_targets<8>), grid, dim3(64), 0, (hipStream_t)stream, v);
    return launched("snac_uct_store_targets");
}

int snac_uct_returns_nstep(int32_t B, int32_t cap_moves, int32_t first, int32_t count, int32_t n, double gamma, const float* reward,
                           const uint8_t* done, const float* value, const float* bootstrap, float* z, void* stream) {
    using namespace snac_detail;
    if (B < 1) return fail(SNAC_ERR_ARG, "B must be >= 1");
    if (cap_moves < 1) return fail(SNAC_ERR_ARG, "cap_moves must be >= 1");
    if ((long long)B * (long long)cap_moves > 0x7FFFFFFFll) return fail(SNAC_ERR_ARG, "B * cap_moves entries exceed int32");
    if (first < 0 || first >= cap_moves) return fail(SNAC_ERR_ARG, "first must be in [0, cap_moves)");
    if (count < 0 || count > cap_moves) return fail(SNAC_ERR_ARG, "count must be in [0, cap_moves]");
    if (n < 1) return fail(SNAC_ERR_ARG, "n must be >= 1");
    if (!std::isfinite(gamma)) return fail(SNAC_ERR_ARG, "gamma must be finite");
    if (!reward || !done || !z) return fail(SNAC_ERR_ARG, "null ring array (reward / done / z)");
    if (!value) return fail(SNAC_ERR_ARG, "null value");
    if (count == 0) return SNAC_OK;                                  // no slot to fill
    const UctNstep v{B, cap_moves, first, count, n, gamma, reward, done, value, bootstrap, z};
    g_kernel = "k_uct_returns_nstep";
    hipLaunchKernelGGL(k_uct_returns_nstep, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, v);
    return launched("snac_uct_returns_nstep");
}

}  // extern "C"
