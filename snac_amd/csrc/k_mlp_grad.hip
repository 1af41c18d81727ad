// k_mlp_grad.hip -- the backward pass of the device network: snac_mlp_backward, from the gradient of the outputs to the gradient of every
// weight and bias in one flat array, as three launches on the caller's stream.  include/snac_hip.h, "Backward pass of the device network",
// has the rule; mlp_grad_rule.h states it per step, for these kernels and for the host.  Nothing is kept from a forward call: the row
// pass recomputes the activations with the forward pass's own layer loop (mlp_dev.h), so they are the forward rule's bits.
//
//   k_mlp_grad_rows    (L >= 2 only) a block of 256 threads takes 16 rows: mlp_layers() with a hook that parks every hidden activation
//                      h_1 .. h_{L-1} in `work` as it is written, then the layers downward with the rows' deltas in LDS (two arrays of
//                      [256][17] float32 in the space of the forward pass's input array, used in turn).  Thread (r, g) owns row r and, in
//                      a pass over 64 units of h_l, the four units ibase + 4 g + t: four float64 chains over k in order.  W_l passes
//                      through LDS in tiles of 32 k x 64 units (a lane reads along a row of W_l: coalesced, no transpose).  The mask reads
//                      h_l[r][i] from `work`: the thread that parked it is the thread that reads it (the same (r, g) -> unit map), and
//                      barriers lie between.  delta_1 .. delta_{L-1} go to `work`.
//   k_mlp_grad_chunk   block (chunk c, tile): a tile is 64 outputs j x 64 inputs i of one layer, the bias one more input column whose
//                      h is 1.0 (d * 1.0 is d: the bias step).  The chunk's rows pass through LDS 32 at a time, delta [32][68] and h [32][68]
//                      float32; thread (tj, ti) = (tid >> 4, tid & 15) holds the 4 x 4 chains of j0 + 4 tj + t, i0 + 4 ti + u over the rows
//                      in ascending order, reads its four deltas and four activations of a row as two 16-byte LDS reads, and writes its
//                      partials to `work`.  h_0 is read from x (rounded as the forward pass rounds it), delta_L from grad_y.
//   k_mlp_grad_reduce  one thread per parameter: the chain over the chunks' partials in order, then grad written or accumulated.
// Scalar 4- and 8-byte global accesses only; accumulators indexed by unrolled constants: no scratch.  DESIGN.md 3.17 has the registers,
// the LDS and the measured times.
#include <cstddef>

#include "snac_units.h"
#include "mlp_rule.h"
#include "mlp_grad_rule.h"
#include "mlp_dev.h"

namespace {

using namespace snac_detail;
using namespace snac_spec;
using namespace snac_mlp_dev;

constexpr int CHUNK = SNAC_MLP_GRAD_CHUNK;
constexpr int DELTA_WORDS = MLP_MAX_HIDDEN * AS;                     // one delta array; two of them fit the forward pass's input array
constexpr int UT = 64, UPRE = KC * UT / THREADS;                     // the row pass's weight tile: 32 k x 64 units
constexpr int TJ = 64, TI = 64, RB = 32, TS = 68;                    // the chunk pass's tile, its rows per trip through LDS, its LDS row stride
static_assert(2 * DELTA_WORDS <= ACT_A_WORDS && KC * (UT + 4) <= WT_WORDS, "the row pass reuses the forward pass's LDS");
static_assert(CHUNK % RB == 0 && (CHUNK == 64 || CHUNK == 128 || CHUNK == 256 || CHUNK == 512), "a chunk is whole trips of RB rows");

struct GradArgs {
    snac_mlp net;
    const void* x;
    int32_t x_is_f64, rows;
    const float* grad_y;
    float* grad;
    int32_t accumulate, P;
    int32_t off[MLP_MAX_LAYERS];                                     // where layer l begins in grad and in a chunk's partials
    double* part;                                                    // [chunks][P]
    float* h[MLP_MAX_LAYERS];                                        // h[l], l = 1 .. L-1: [rows][dim[l]] in work
    float* d[MLP_MAX_LAYERS];                                        // d[l], l = 1 .. L-1: [rows][dim[l]] in work
};

__global__ __launch_bounds__(THREADS) void k_mlp_grad_rows(const GradArgs g) {
    __shared__ float act_a[ACT_A_WORDS];
    __shared__ float act_b[ACT_B_WORDS];
    __shared__ __attribute__((aligned(16))) float wt[WT_WORDS];
    const int tid = threadIdx.x, r = tid & (TR - 1), grp = tid >> 4;
    const long long row0 = (long long)blockIdx.x * TR;
    const int32_t rows = g.rows, L = g.net.layers;
    const bool mine = row0 + r < rows;                               // whether row r of the block exists (a row past the end copies the last)
    const size_t myrow = (size_t)(row0 + r);

    {   // as k_mlp: the block's input rows into act_a[i][r], rounded to float32
        const int K = g.net.dim[0];
        const long long row = row0 + grp < rows ? row0 + grp : rows - 1;
        const bool f64 = g.x_is_f64 != 0;
        for (int i = r; i < K; i += TR) act_a[i * AS + grp] = mlp_input(g.x, f64, (size_t)row * K + i);
    }
    mlp_layers(g.net, act_a, act_b, wt, tid, [&](int l, int j, int rr, float v) {
        if (l < L - 1 && mine) g.h[l + 1][myrow * g.net.dim[l + 1] + j] = v;         // rr == r: the owning thread calls
    });

    // delta_L = the rows of grad_y, into din[k][r]; mlp_layers ended in a barrier, so act_a is free
    float* din = act_a;
    float* dout = act_a + DELTA_WORDS;
    {
        const int N = g.net.dim[L];
        const long long row = row0 + grp < rows ? row0 + grp : rows - 1;
        for (int k = r; k < N; k += TR) din[k * AS + grp] = g.grad_y[(size_t)row * N + k];
    }
    for (int l = L - 1; l >= 1; --l) {                               // uniform throughout
        const int K = g.net.dim[l + 1], N = g.net.dim[l];            // the chain runs over the K units above; N units of h_l get a delta
        const float* W = g.net.w[l];                                 // [K][N]
        for (int ibase = 0; ibase < N; ibase += UT) {
            double acc[JT];
#pragma unroll
            for (int t = 0; t < JT; ++t) acc[t] = 0.0;
            float pre[UPRE];
            auto prefetch = [&](int k0) {                            // element e of the tile: unit ibase + (e & 63) of k0 + (e >> 6)
#pragma unroll
                for (int q = 0; q < UPRE; ++q) {
                    const int e = tid + q * THREADS, k = k0 + e / UT, i = ibase + (e & (UT - 1));
                    pre[q] = (k < K && i < N) ? W[(size_t)k * N + i] : 0.0f;
                }
            };
            prefetch(0);
            for (int k0 = 0; k0 < K; k0 += KC) {
                __syncthreads();                                     // the tile's readers are done; the first of a layer: din is written
#pragma unroll
                for (int q = 0; q < UPRE; ++q) {
                    const int e = tid + q * THREADS;
                    wt[(e / UT) * WS + (e & (UT - 1))] = pre[q];
                }
                __syncthreads();
                if (k0 + KC < K) prefetch(k0 + KC);
                const int kc = K - k0 < KC ? K - k0 : KC;
                for (int kk = 0; kk < kc; ++kk) {                    // k ascending: the stated order
                    const float dv = din[(k0 + kk) * AS + r];
                    const float* wrow = wt + kk * WS + grp * JT;
#pragma unroll
                    for (int t = 0; t < JT; ++t) acc[t] = mlp_delta_step(acc[t], wrow[t], dv);
                }
            }
#pragma unroll
            for (int t = 0; t < JT; ++t) {
                const int i = ibase + grp * JT + t;
                if (i < N) {
                    const float hv = mine ? g.h[l][myrow * N + i] : 0.0f;                // parked above by this thread
                    const float dv = mlp_delta_mask(hv, acc[t]);
                    dout[i * AS + r] = dv;
                    if (mine) g.d[l][myrow * N + i] = dv;
                }
            }
        }
        float* t = din;
        din = dout, dout = t;
    }
}

// which tile of which layer block y is: the layers in order, each with ceil(N / 64) x ceil((K + 1) / 64) tiles, j-major
struct Tile { int l, j0, i0; };
__device__ __forceinline__ Tile tile_of(const snac_mlp& net, int y) {
    Tile t{0, 0, 0};
    for (int l = 0; l < net.layers; ++l) {
        const int nj = (net.dim[l + 1] + TJ - 1) / TJ, ni = (net.dim[l] + 1 + TI - 1) / TI;
        if (y < nj * ni || l == net.layers - 1) {
            t.l = l, t.j0 = (y / ni) * TJ, t.i0 = (y % ni) * TI;
            break;
        }
        y -= nj * ni;
    }
    return t;
}

__global__ __launch_bounds__(THREADS) void k_mlp_grad_chunk(const GradArgs g) {
    __shared__ __attribute__((aligned(16))) float ds[RB * TS];
    __shared__ __attribute__((aligned(16))) float hs[RB * TS];
    const int tid = threadIdx.x, tj = tid >> 4, ti = tid & 15;
    const Tile tl = tile_of(g.net, (int)blockIdx.y);                 // uniform
    const int l = tl.l, K = g.net.dim[l], N = g.net.dim[l + 1], L = g.net.layers;
    const long long c = blockIdx.x, rows = g.rows;
    const long long first = c * CHUNK, end = first + CHUNK < rows ? first + CHUNK : rows;
    const float* dsrc = l == L - 1 ? g.grad_y : g.d[l + 1];          // delta_{l+1} [rows][N]
    const bool f64 = g.x_is_f64 != 0;

    double acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[t][u] = 0.0;

    for (long long b0 = first; b0 < end; b0 += RB) {                 // uniform
        const int nb = (int)(end - b0 < RB ? end - b0 : RB);
        __syncthreads();                                             // the readers of the rows before are done
#pragma unroll
        for (int q = 0; q < RB * TJ / THREADS; ++q) {
            const int e = tid + q * THREADS, b = e >> 6, col = e & 63;
            const size_t row = (size_t)(b0 + b);
            const int j = tl.j0 + col, i = tl.i0 + col;
            float dv = 0.0f, hv = 0.0f;
            if (b < nb) {
                if (j < N) dv = dsrc[row * N + j];
                if (i < K) hv = l == 0 ? mlp_input(g.x, f64, row * K + i) : g.h[l][row * K + i];
                else if (i == K) hv = 1.0f;                          // the bias column
            }
            ds[b * TS + col] = dv;
            hs[b * TS + col] = hv;
        }
        __syncthreads();
        for (int b = 0; b < nb; ++b) {                               // rows ascending: the stated order
            const float4 dv = *reinterpret_cast<const float4*>(ds + b * TS + tj * 4);
            const float4 hv = *reinterpret_cast<const float4*>(hs + b * TS + ti * 4);
            const float d4[4] = {dv.x, dv.y, dv.z, dv.w}, h4[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[t][u] = mlp_grad_step(acc[t][u], d4[t], h4[u]);
        }
    }
    double* part = g.part + (size_t)c * g.P + g.off[l];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = tl.j0 + tj * 4 + t;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = tl.i0 + ti * 4 + u;
            if (j < N && i < K) part[(size_t)j * K + i] = acc[t][u];
            else if (j < N && i == K) part[(size_t)N * K + j] = acc[t][u];
        }
    }
}

__global__ __launch_bounds__(THREADS) void k_mlp_grad_reduce(const GradArgs g, const long long chunks) {
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= g.P) return;
    const double total = mlp_grad_total(g.part + p, (size_t)g.P, chunks);
    const bool acc = g.accumulate != 0;                              // uniform
    g.grad[p] = mlp_grad_end(total, acc ? g.grad[p] : 0.0f, acc);
}

long long chunks_of(int32_t rows) { return ((long long)rows + CHUNK - 1) / CHUNK; }

// the float32 values parked per row: h_l and delta_l for l = 1 .. L-1
long long parked_per_row(const snac_mlp* net) {
    long long n = 0;
    for (int l = 1; l < net->layers; ++l) n += 2LL * net->dim[l];
    return n;
}

int64_t work_bytes_of(const snac_mlp* net, int32_t rows) {
    const long long P = mlp_grad_layout(net->layers, net->dim, nullptr);
    return 8 * chunks_of(rows) * P + 4 * (long long)rows * parked_per_row(net);
}

}  // namespace

extern "C" int64_t snac_mlp_backward_work_bytes(const snac_mlp* net, int32_t rows) {
    using namespace snac_detail;
    if (!net) return fail(SNAC_ERR_ARG, "null net");
    if (const char* why = snac_spec::mlp_dims_refusal(net->layers, net->dim)) return fail(SNAC_ERR_ARG, why);
    if (rows < 1) return fail(SNAC_ERR_ARG, "rows must be >= 1");
    return work_bytes_of(net, rows);
}

extern "C" int snac_mlp_backward(const snac_mlp* net, const void* x, int x_is_f64, int32_t rows, const float* grad_y, float* grad,
                                 int32_t accumulate, void* work, int64_t work_bytes, void* stream) {
    using namespace snac_detail;
    if (int rc = mlp_check(net, x, x_is_f64, rows)) return rc;
    if (!grad_y || !grad) return fail(SNAC_ERR_ARG, "null grad_y / grad");
    if ((uintptr_t)grad_y % 4 || (uintptr_t)grad % 4) return fail(SNAC_ERR_ARG, "grad_y and grad must be 4-byte aligned");
    if (accumulate != 0 && accumulate != 1) return fail(SNAC_ERR_ARG, "accumulate must be 0 or 1");
    if (!work) return fail(SNAC_ERR_ARG, "null work");
    if ((uintptr_t)work % 8) return fail(SNAC_ERR_ARG, "work must be 8-byte aligned");
    if (work_bytes < work_bytes_of(net, rows)) return fail(SNAC_ERR_ARG, "work_bytes is less than snac_mlp_backward_work_bytes() asks for");

    GradArgs g{};
    g.net = *net, g.x = x, g.x_is_f64 = x_is_f64, g.rows = rows, g.grad_y = grad_y, g.grad = grad, g.accumulate = accumulate;
    g.P = mlp_grad_layout(net->layers, net->dim, g.off);
    const long long chunks = chunks_of(rows);
    const int L = net->layers;
    g.part = static_cast<double*>(work);
    float* at = reinterpret_cast<float*>(g.part + (size_t)chunks * g.P);
    for (int l = 1; l < L; ++l) g.h[l] = at, at += (size_t)rows * net->dim[l];
    for (int l = 1; l < L; ++l) g.d[l] = at, at += (size_t)rows * net->dim[l];
    int tiles = 0;
    for (int l = 0; l < L; ++l) tiles += ((net->dim[l + 1] + TJ - 1) / TJ) * ((net->dim[l] + 1 + TI - 1) / TI);

    const hipStream_t s = (hipStream_t)stream;
    if (L >= 2) {
        g_kernel = "k_mlp_grad_rows";
        hipLaunchKernelGGL(k_mlp_grad_rows, dim3((unsigned)(((long long)rows + TR - 1) / TR)), dim3(THREADS), 0, s, g);
        if (int rc = launched("snac_mlp_backward")) return rc;       // each launch's own error, under the kernel snac_last_kernel() names
    }
    g_kernel = "k_mlp_grad_chunk";
    hipLaunchKernelGGL(k_mlp_grad_chunk, dim3((unsigned)chunks, (unsigned)tiles), dim3(THREADS), 0, s, g);
    if (int rc = launched("snac_mlp_backward")) return rc;
    g_kernel = "k_mlp_grad_reduce";
    hipLaunchKernelGGL(k_mlp_grad_reduce, dim3((unsigned)((g.P + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, g, chunks);
    return launched("snac_mlp_backward");
}
