// k_prio.hip -- prioritised replay: a 64-ary sum tree of integer weights in device memory (snac_prio_layout / snac_prio_init /
// snac_prio_update / snac_prio_fill / snac_prio_sample).  include/snac_hip.h, "Prioritised replay", has the layout and the semantics.
#include <cmath>
#include <cstddef>

#include "snac_units.h"

// Small, latency-bound kernels.  The leaves are written lane = entry; every sum is recomputed from its 64 children by one wavefront
// (lane = child, a wave reduction, one lane stores the parent), level by level, one launch per level: the launches' order on the stream
// is the synchronisation, and a sum never depends on the order in which anything arrived.  A draw is wave = sample: per level a 64-bit
// inclusive scan over the 64 children, the lowest lane whose prefix passes u, and u less that lane's exclusive prefix goes one level down.
namespace {

constexpr int PRIO_MAX_LEVELS = 7;                                   // sum levels of 2^31 - 64 entries: 6
constexpr long long PRIO_MAX_ENTRIES = 0x7FFFFFFFll - 63;            // 2^31 - 64: every sum below 2^63
constexpr int PRIO_WAVES = 4;                                        // wavefronts per workgroup where a wave is the unit of work

struct PrioLayout {
    int64_t bytes;
    int32_t levels;
    int64_t off[8];                                                  // bytes from the buffer's start; [0] = leaves, [l] = sum level l
    int64_t count[8];                                                // values of each level before padding; [0] = entries
};

PrioLayout prio_layout(int64_t entries) {
    PrioLayout L{};
    const int64_t e64 = (entries + 63) / 64 * 64;
    L.off[0] = 128;
    L.count[0] = entries;
    int64_t at = 128 + e64 * 4, n = e64 / 64;
    int l = 1;
    for (;; ++l) {
        L.off[l] = at;
        L.count[l] = n;
        at += (n + 63) / 64 * 64 * 8;
        if (n == 1) break;
        n = (n + 63) / 64;
    }
    L.levels = l;
    L.bytes = at;
    return L;
}

// what the kernels know of the buffer: the start of each level in bytes, and how many 64-child groups each sum level holds
struct PrioTree {
    unsigned char* base;
    int32_t entries, levels;
    long long off[8];
};

PrioTree prio_tree(void* tree, int32_t entries, const PrioLayout& L) {
    PrioTree t{};
    t.base = (unsigned char*)tree;
    t.entries = entries;
    t.levels = L.levels;
    for (int i = 0; i < 8; ++i) t.off[i] = L.off[i];
    return t;
}

__device__ inline uint32_t* prio_leaves(const PrioTree& t) { return (uint32_t*)(t.base + t.off[0]); }
__device__ inline unsigned long long* prio_level(const PrioTree& t, int l) { return (unsigned long long*)(t.base + t.off[l]); }

// quant(p, s) of the header
__device__ inline uint32_t prio_quant(float p, double scale) {
    if (p == 0.f) return 0u;
    if (!(p > 0.f)) return 1u;                                       // NaN or negative
    const double x = rint((double)p * scale);
    return x < 1.0 ? 1u : x >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)x;
}

__device__ inline unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

struct PrioInit {
    uint4* pieces;                                                   // the buffer as 16-byte pieces
    long long count;
    unsigned long long max_weight, entries, levels;
};

__global__ __launch_bounds__(256) void k_prio_init(const PrioInit v) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < v.count; i += stride) {
        uint4 piece = make_uint4(0u, 0u, 0u, 0u);
        if (i == 0) piece = make_uint4((uint32_t)v.max_weight, (uint32_t)(v.max_weight >> 32), (uint32_t)v.entries, (uint32_t)(v.entries >> 32));
        if (i == 1) piece.x = (uint32_t)v.levels;
        v.pieces[i] = piece;
    }
}

struct PrioUpdate {
    PrioTree t;
    const int32_t* index;
    const float* priority;
    int32_t n;
    double scale;
};

__global__ __launch_bounds__(256) void k_prio_zero(const PrioUpdate v) {
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    if (j >= v.n) return;
    const int i = v.index[j];
    if (i < 0 || i >= v.t.entries) return;
    prio_leaves(v.t)[i] = 0u;
}

__global__ __launch_bounds__(256) void k_prio_max(const PrioUpdate v) {
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    uint32_t w = 0u;
    if (j < v.n) {
        const int i = v.index[j];
        if (i >= 0 && i < v.t.entries) {
            w = prio_quant(v.priority[j], v.scale);
            if (w) atomicMax(prio_leaves(v.t) + i, w);               // the leaf is 0 since k_prio_zero: the largest of the duplicates stays
        }
    }
    uint32_t m = w;                                                  // one atomic per wave on the head word
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax((unsigned long long*)v.t.base, (unsigned long long)m);
}

// parent g of level `l` <- the sum of its 64 children of level l - 1 (the leaves for l == 1); every level is padded to whole groups
__device__ inline void prio_parent(const PrioTree& t, int l, long long g, int lane) {
    const unsigned long long c = l == 1 ? (unsigned long long)prio_leaves(t)[g * 64 + lane] : prio_level(t, l - 1)[g * 64 + lane];
    const unsigned long long s = wave_sum(c);
    if (lane == 0) prio_level(t, l)[g] = s;
}

struct PrioLevelIdx {
    PrioTree t;
    const int32_t* index;
    int32_t n, level;
};

// wave j: the level's ancestor of entry index[j]
__global__ __launch_bounds__(64 * PRIO_WAVES) void k_prio_level_idx(const PrioLevelIdx v) {
    const int lane = (int)threadIdx.x & 63;
    const int j = (int)blockIdx.x * PRIO_WAVES + ((int)threadIdx.x >> 6);
    if (j >= v.n) return;
    const int i = v.index[j];
    if (i < 0 || i >= v.t.entries) return;
    prio_parent(v.t, v.level, (long long)i >> (6 * v.level), lane);
}

struct PrioLevelRange {
    PrioTree t;
    long long g0, groups;                                            // parents [g0, g0 + groups) of the level
    int32_t level;
};

__global__ __launch_bounds__(64 * PRIO_WAVES) void k_prio_level_range(const PrioLevelRange v) {
    const int lane = (int)threadIdx.x & 63;
    const long long k = (long long)blockIdx.x * PRIO_WAVES + ((int)threadIdx.x >> 6);
    if (k >= v.groups) return;
    prio_parent(v.t, v.level, v.g0 + k, lane);
}

struct PrioFill {
    PrioTree t;
    int32_t first, count;
    uint32_t weight;
    int32_t use_max;                                                 // the head's max_weight instead of `weight`
};

__global__ __launch_bounds__(256) void k_prio_fill(const PrioFill v) {
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k >= v.count) return;
    const uint32_t w = v.use_max ? (uint32_t)*(const unsigned long long*)v.t.base : v.weight;    // max_weight < 2^32
    prio_leaves(v.t)[(long long)v.first + k] = w;
}

struct PrioSample {
    PrioTree t;
    uint32_t key;                                                    // stream 4's
    long long sampler_id;
    uint32_t t0;                                                     // 2 * draw
    int32_t n, stratified;
    int32_t* index;
    float* prob;
    uint32_t* weight;
};

__global__ __launch_bounds__(64 * PRIO_WAVES) void k_prio_sample(const PrioSample v) {
    const int lane = (int)threadIdx.x & 63;
    const int j = (int)blockIdx.x * PRIO_WAVES + ((int)threadIdx.x >> 6);
    if (j >= v.n) return;
    const unsigned long long T = prio_level(v.t, v.t.levels)[0];
    const EnvKeys k = env_keys(v.key, (uint64_t)(v.sampler_id + j));
    const unsigned long long r = ((unsigned long long)rng_word(k, v.t0) << 32) | rng_word(k, v.t0 + 1u);
    const unsigned long long n = (unsigned long long)v.n, q = T / n, rem = T % n;
    unsigned long long u;
    if (v.stratified && q >= 1) {
        const unsigned long long jj = (unsigned long long)j;
        u = jj * q + (jj < rem ? jj : rem) + __umul64hi(r, q + (jj < rem ? 1ull : 0ull));
    } else {
        u = __umul64hi(r, T);
    }
    long long g = 0;
    unsigned long long own = 0;
    bool found = T != 0;
    for (int l = v.t.levels; l >= 1 && found; --l) {                 // the children of group g of level l: level l - 1, all in bounds
        const unsigned long long c = l == 1 ? (unsigned long long)prio_leaves(v.t)[g * 64 + lane] : prio_level(v.t, l - 1)[g * 64 + lane];
        unsigned long long incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        const unsigned long long pass = __ballot(incl > u);
        if (pass == 0) { found = false; break; }                     // sums that do not match their children: no entry, never a wild index
        const int pick = __ffsll((long long)pass) - 1;
        u -= __shfl(incl - c, pick, 64);
        own = __shfl(c, pick, 64);
        g = g * 64 + pick;
    }
    if (lane == 0) {
        v.index[j] = found ? (int32_t)g : -1;
        v.prob[j] = found ? (float)((double)own / (double)T) : 0.f;
        if (v.weight) v.weight[j] = found ? (uint32_t)own : 0u;
    }
}

int prio_check(const void* tree, int32_t entries) {
    using namespace snac_detail;
    if (!tree) return fail(SNAC_ERR_ARG, "null tree");
    if (((uintptr_t)tree & 127) != 0) return fail(SNAC_ERR_ARG, "tree must be 128-byte aligned");
    if (entries < 1 || (long long)entries > PRIO_MAX_ENTRIES) return fail(SNAC_ERR_ARG, "entries must be in [1, 2^31 - 64]");
    return SNAC_OK;
}

int scale_check(int32_t scale_log2) {
    return scale_log2 < 0 || scale_log2 > 31 ? snac_detail::fail(SNAC_ERR_ARG, "scale_log2 must be in 0 .. 31") : (int)SNAC_OK;
}

unsigned wave_grid(long long waves) { return (unsigned)((waves + PRIO_WAVES - 1) / PRIO_WAVES); }

// sum level l over the parents of the entries [first, first + count)
void launch_range(const PrioTree& t, int l, long long first, long long count, hipStream_t s) {
    const long long g0 = first >> (6 * l), g1 = ((first + count - 1) >> (6 * l)) + 1;
    const PrioLevelRange v{t, g0, g1 - g0, l};
    snac_detail::g_kernel = "k_prio_level_range";
    hipLaunchKernelGGL(k_prio_level_range, dim3(wave_grid(g1 - g0)), dim3(64 * PRIO_WAVES), 0, s, v);
}

}  // namespace

extern "C" {

int snac_prio_layout(int32_t entries, int64_t* bytes, int32_t* levels, int64_t* level_offset) {
    using namespace snac_detail;
    if (entries < 1 || (long long)entries > PRIO_MAX_ENTRIES) return fail(SNAC_ERR_ARG, "entries must be in [1, 2^31 - 64]");
    if (!bytes || !levels || !level_offset) return fail(SNAC_ERR_ARG, "null output (bytes / levels / level_offset)");
    const PrioLayout L = prio_layout(entries);
    static_assert(PRIO_MAX_LEVELS < 8, "level_offset holds 8 offsets");
    *bytes = L.bytes;
    *levels = L.levels;
    for (int i = 0; i < 8; ++i) level_offset[i] = L.off[i];
    return SNAC_OK;
}

int snac_prio_init(void* tree, int32_t entries, int32_t scale_log2, void* stream) {
    using namespace snac_detail;
    if (int rc = prio_check(tree, entries)) return rc;
    if (int rc = scale_check(scale_log2)) return rc;
    const PrioLayout L = prio_layout(entries);
    const PrioInit v{(uint4*)tree, L.bytes / 16, 1ull << scale_log2, (unsigned long long)entries, (unsigned long long)L.levels};
    const long long blocks = (v.count + 255) / 256;
    g_kernel = "k_prio_init";
    hipLaunchKernelGGL(k_prio_init, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, v);
    return launched("snac_prio_init");
}

int snac_prio_update(void* tree, int32_t entries, int32_t scale_log2, const int32_t* index, const float* priority, int32_t n, void* stream) {
    using namespace snac_detail;
    if (int rc = prio_check(tree, entries)) return rc;
    if (int rc = scale_check(scale_log2)) return rc;
    if (n < 0) return fail(SNAC_ERR_ARG, "n must be >= 0");
    if (!index) return fail(SNAC_ERR_ARG, "null index");
    if (!priority) return fail(SNAC_ERR_ARG, "null priority");
    if (n == 0) return SNAC_OK;                                      // no entry to update
    const PrioLayout L = prio_layout(entries);
    const PrioTree t = prio_tree(tree, entries, L);
    const hipStream_t s = (hipStream_t)stream;
    const PrioUpdate v{t, index, priority, n, (double)(1ull << scale_log2)};
    const dim3 lanes((unsigned)(((long long)n + 255) / 256));
    g_kernel = "k_prio_max";
    hipLaunchKernelGGL(k_prio_zero, lanes, dim3(256), 0, s, v);
    hipLaunchKernelGGL(k_prio_max, lanes, dim3(256), 0, s, v);
    for (int l = 1; l <= L.levels; ++l) {
        if (L.count[l] <= (int64_t)n) {                              // no more parents than updates: the whole level, without the index
            launch_range(t, l, 0, entries, s);
        } else {
            const PrioLevelIdx w{t, index, n, l};
            g_kernel = "k_prio_level_idx";
            hipLaunchKernelGGL(k_prio_level_idx, dim3(wave_grid(n)), dim3(64 * PRIO_WAVES), 0, s, w);
        }
    }
    return launched("snac_prio_update");
}

int snac_prio_fill(void* tree, int32_t entries, int32_t scale_log2, int32_t first, int32_t count, double priority, void* stream) {
    using namespace snac_detail;
    if (int rc = prio_check(tree, entries)) return rc;
    if (int rc = scale_check(scale_log2)) return rc;
    if (first < 0 || first >= entries) return fail(SNAC_ERR_ARG, "first must be in [0, entries)");
    if (count < 0 || (long long)first + count > entries) return fail(SNAC_ERR_ARG, "count must be in [0, entries - first]");
    if (priority != priority) return fail(SNAC_ERR_ARG, "priority must not be NaN");
    if (count == 0) return SNAC_OK;                                  // no entry to set
    uint32_t w = 0u;
    if (priority > 0.0) {                                            // quant(priority)
        const double x = std::rint(priority * (double)(1ull << scale_log2));
        w = x < 1.0 ? 1u : x >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)x;
    }
    const PrioLayout L = prio_layout(entries);
    const PrioTree t = prio_tree(tree, entries, L);
    const hipStream_t s = (hipStream_t)stream;
    const PrioFill v{t, first, count, w, priority < 0.0 ? 1 : 0};
    g_kernel = "k_prio_fill";
    hipLaunchKernelGGL(k_prio_fill, dim3((unsigned)(((long long)count + 255) / 256)), dim3(256), 0, s, v);
    for (int l = 1; l <= L.levels; ++l) launch_range(t, l, first, count, s);
    return launched("snac_prio_fill");
}

int snac_prio_sample(const void* tree, int32_t entries, uint64_t seed, int64_t sampler_id, int32_t draw, int32_t n, int32_t stratified,
                     int32_t* index, float* prob, uint32_t* weight, void* stream) {
    using namespace snac_detail;
    if (int rc = prio_check(tree, entries)) return rc;
    if (draw < 0) return fail(SNAC_ERR_ARG, "draw must be in [0, 2^31)");
    if (n < 0) return fail(SNAC_ERR_ARG, "n must be >= 0");
    if (!index) return fail(SNAC_ERR_ARG, "null index");
    if (!prob) return fail(SNAC_ERR_ARG, "null prob");
    if (n == 0) return SNAC_OK;                                      // no sample to draw
    const PrioLayout L = prio_layout(entries);
    const PrioSample v{prio_tree((void*)tree, entries, L), stream_key(seed, 4), (long long)sampler_id, 2u * (uint32_t)draw, n, stratified != 0,
                       index, prob, weight};
    g_kernel = "k_prio_sample";
    hipLaunchKernelGGL(k_prio_sample, dim3(wave_grid(n)), dim3(64 * PRIO_WAVES), 0, (hipStream_t)stream, v);
    return launched("snac_prio_sample");
}

}  // extern "C"
