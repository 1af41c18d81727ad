// nodes_dev.h -- what the node-pool kernels share (k_nodes.hip: tree edges, k_nodes_obs.hip: observation rows, k_eval.hip: leaf evaluation):
// the map of a record, a line record's trip through LDS, the window decoders of the three kinds, the scalar slots with the value-by-value
// row writer, and the head / tail split of a call.  Internal.
#pragma once
#include <cstddef>

#include "snac_units.h"

// ------------------------------------------------------------------------------------------------
// The record map, in 16-byte pieces (include/snac_hip.h has the structs):
//     snac_node1d   0 header | 1 episode counter, 3 zero words | 2-5 the 32 cells (30 interior + 2 pad) | 6-7 zero      = ONE 128-byte line
//     snac_node2d   0 header | 1 episode counter, 3 zero words | 2-6 the board (20 row words)            | 7 zero        = ONE 128-byte line
//     snac_node3d   0 header | 1 episode counter, 3 zero words | 2-51 the 400 heights                    | 52-55 zero    = seven lines
static_assert(sizeof(snac_node1d) == 128 && offsetof(snac_node1d, episode) == 16 && offsetof(snac_node1d, cells) == 32 &&
              offsetof(snac_node1d, zero1) == 96, "snac_node1d: one line");
static_assert(sizeof(snac_node2d) == 128 && offsetof(snac_node2d, episode) == 16 && offsetof(snac_node2d, board) == 32 &&
              offsetof(snac_node2d, zero1) == 112, "snac_node2d: one line");
static_assert(sizeof(snac_node3d) == 896 && offsetof(snac_node3d, episode) == 16 && offsetof(snac_node3d, heights) == 32 &&
              offsetof(snac_node3d, zero1) == 832, "snac_node3d: seven lines");

namespace {

constexpr int LINE_PIECES = 8, LINE_WORDS = 32;                      // a line record (1D / 2D) in 16-byte pieces / 4-byte words
constexpr int REC_EPISODE = 4, REC_GRID = 8;                         // the words of the episode counter and of the grid's start, every kind
constexpr int REC_GRID_PIECE = REC_GRID / 4;                         // (the grid's first piece)
constexpr int GRID_PIECES_1D = 4, GRID_PIECES_2D = 5, GRID_PIECES_3D = 50;   // grid pieces per record: what k_nodes_copy moves per row
constexpr int REC3_PIECES = 56;                                      // the 3D record; GRID_PIECES_3D of them are its heights

// ------------------------------------------------------------------------------------------------
// A wave's 64 line records in LDS.  A record's eight pieces are fetched by eight neighbouring lanes (512 pieces = eight load instructions:
// the memory side reads whole 128-byte lines, profiles/r06_rd_gran.txt) and piece p of record e lies at piece slot p ^ (e & 7): the lanes'
// reads of one logical word spread over eight bank groups.  Lane = record from then on.  rec: LINE_WORDS * 64 words of this wave.
// the piece slot of piece `part` of record e in a wave's LDS slice: the one place that knows the swizzle
__device__ __forceinline__ constexpr int line_slot(int e, int part) { return e * LINE_PIECES + (part ^ (e & 7)); }
struct LineRecs {
    uint32_t* rec;
    uint32_t* mine;                                                  // this lane's record
    int lane, sw;
    __device__ __forceinline__ LineRecs(uint32_t* rec_, int lane_) : rec(rec_), mine(rec_ + lane_ * LINE_WORDS), lane(lane_), sw(lane_ & 7) {}
    // record srow (of the lane's element) of each of the wave's first nlive elements arrives; FETCH: bit p set = piece p is loaded, the
    // others -- and the pieces of elements past nlive -- are zero in LDS.  Plain loads: children share their parents.  (The test of FETCH is
    // spelled as compares -- no piece from TOP up, none of the holes below -- which the compiler folds into the load's predicate; a shift
    // of the mask by the piece costs registers in the observe kernels.)
    template <uint32_t FETCH>
    __device__ __forceinline__ void gather(const uint4* nodes, int srow, int nlive) {
        constexpr int TOP = 32 - __builtin_clz(FETCH);
        static_assert(FETCH != 0u && TOP <= LINE_PIECES, "a mask of the record's pieces");
        uint4 rv[LINE_PIECES];
#pragma unroll
        for (int i = 0; i < LINE_PIECES; ++i) {
            const int g = i * 64 + lane, e = g >> 3, part = g & 7;
            const int se = __builtin_amdgcn_ds_bpermute(e << 2, srow);
            rv[i] = make_uint4(0u, 0u, 0u, 0u);
            bool fetch = g < nlive * LINE_PIECES;
#pragma unroll
            for (int p = 0; p < TOP; ++p)
                if (!((FETCH >> p) & 1u)) fetch = fetch && part != p;
            if (fetch && (TOP == LINE_PIECES || part < TOP)) rv[i] = nodes[(size_t)se * LINE_PIECES + part];
        }
#pragma unroll
        for (int i = 0; i < LINE_PIECES; ++i) {
            const int g = i * 64 + lane, e = g >> 3, part = g & 7;
            ((uint4*)rec)[line_slot(e, part)] = rv[i];
        }
    }
    // the records leave for rows drow, whole lines, the same way; clean(piece, part): what piece `part` leaves as
    template <class F>
    __device__ __forceinline__ void scatter(uint4* nodes, int drow, int nlive, F clean) const {
#pragma unroll
        for (int i = 0; i < LINE_PIECES; ++i) {
            const int g = i * 64 + lane, e = g >> 3, part = g & 7;
            const int de = __builtin_amdgcn_ds_bpermute(e << 2, drow);
            if (g < nlive * LINE_PIECES) nodes[(size_t)de * LINE_PIECES + part] = clean(((const uint4*)rec)[line_slot(e, part)], part);
        }
    }
    // logical word wd of this lane's record: word() reads it (by value: the decoders' selects stay selects), word_at() is the place itself
    __device__ __forceinline__ uint32_t& word_at(int wd) const { return mine[(((wd >> 2) ^ sw) << 2) + (wd & 3)]; }
    __device__ __forceinline__ uint32_t word(int wd) const { return word_at(wd); }
    __device__ __forceinline__ Lane header() const {
        const uint4 h = *(const uint4*)&mine[(0 ^ sw) << 2];
        Lane s;
        s.unpack(make_int4((int)h.x, (int)h.y, (int)h.z, (int)h.w));
        return s;
    }
    __device__ __forceinline__ void set_header(const Lane& s) const {
        const int4 h = s.pack();
        *(uint4*)&mine[(0 ^ sw) << 2] = make_uint4((uint32_t)h.x, (uint32_t)h.y, (uint32_t)h.z, (uint32_t)h.w);
    }
};
constexpr uint32_t FETCH_ALL = 0xFFu;
constexpr uint32_t fetch_but(int p0, int p1 = 8, int p2 = 8) { return FETCH_ALL & ~((1u << p0) | (1u << p1) | (1u << p2)); }

// ------------------------------------------------------------------------------------------------
// The window decoders: the cells round position (r, c) of a record, as the canonical observation row shows them.

// 2D: the 7 x 7 window as two-bit codes (00 empty / 01 brick / 11 frame), 14 bits per row.  sh: the first window column, bordered, 0..19
// (s.c - 3 of a position that rules2d made; a hand-made record's is clamped by the caller).  GE: the board's row words.
struct Window2D {
    uint32_t wr[7];
    __device__ __forceinline__ Window2D(const LineRecs& n, int r, int sh, int GE) {
        constexpr uint32_t FRAME26 = 0x3800007u;                     // frame columns 0-2 and 23-25 of an interior row
        const uint32_t frm = spread16((FRAME26 >> sh) & 0x7Fu) * 3u;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const int q = r - 6 + i;                                 // board row of window row i
            const bool in = (unsigned)q < (unsigned)GE;
            const uint32_t g = n.word(REC_GRID + (in ? q : 0));
            wr[i] = in ? (spread16(((g << 3) >> sh) & 0x7Fu) | frm) : 0x3FFFu;
        }
    }
    __device__ __forceinline__ int operator()(int el) const { const int i = el / 7, j = el - 7 * i; return ((int)(wr[i] << (30 - 2 * j))) >> 30; }
};

// 1D: interior cell j of the lane's record, or the frame (-1) for j outside 0..29; the 5-cell window round bordered position r (= interior cell r - 2)
__device__ __forceinline__ int cell1d(const LineRecs& n, int j) {
    const bool in = (unsigned)j < 30u;
    const int jj = in ? j : 0;
    const uint32_t v = n.word(REC_GRID + (jj >> 1));
    return in ? (int)(int16_t)((jj & 1) ? (v >> 16) : (v & 0xffffu)) : -1;
}
__device__ __forceinline__ void window1d(const LineRecs& n, int r, int (&win)[5]) {
#pragma unroll
    for (int i = 0; i < 5; ++i) win[i] = cell1d(n, r - 4 + i);
}

// 3D: a wave takes 32 records, their heights through LDS as REC[element][400 cells]; lane l and its shadow l + 32 own element l & 31 and
// load its header (and counter) themselves -- those never pass through LDS.  rec: WAVE_BYTES of this wave (the staging tile of emit_tile
// takes the heights' place afterwards).
struct Heights3D {
    static constexpr int E = 32, RECB = GRID_PIECES_3D * 16, HP = GRID_PIECES_3D;
    static constexpr int WAVE_BYTES = E * RECB > TILE_STG_BYTES ? E * RECB : TILE_STG_BYTES;
    char* rec;
    int16_t* mine;                                                   // the heights of this lane's element
    int lane;
    __device__ __forceinline__ Heights3D(char* rec_, int lane_) : rec(rec_), mine((int16_t*)(rec_ + (lane_ & (E - 1)) * RECB)), lane(lane_) {}
    // piece q of the wave's 32 x 50 height pieces (element q / 50) comes from piece 2 + q % 50 of its record: 25 loads in flight per lane
    __device__ __forceinline__ void gather(const uint4* nodes, int srow, int nlive) const {
        uint4 pv[HP / 2];
#pragma unroll
        for (int p = 0; p < HP / 2; ++p) {
            const int q = p * 64 + lane, e = q / HP, l = q - HP * e;
            const int se = __shfl(srow, e);
            pv[p] = e < nlive ? nodes[(size_t)se * REC3_PIECES + REC_GRID_PIECE + l] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int p = 0; p < HP / 2; ++p) *(uint4*)(rec + (p * 64 + lane) * 16) = pv[p];
    }
    __device__ __forceinline__ int cell(int R, int C) const {        // a cell of the element's map in bordered coordinates: the frame is -1
        const bool in = (unsigned)(R - 3) < 20u && (unsigned)(C - 3) < 20u;
        const int v = (int)mine[in ? (R - 3) * 20 + (C - 3) : 0];
        return in ? v : -1;
    }
    __device__ __forceinline__ void window(int r, int c, int (&cellv)[49]) const {
#pragma unroll
        for (int el = 0; el < 49; ++el) { const int i = el / 7, j = el - 7 * i; cellv[el] = cell(r - 3 + i, c - 3 + j); }
    }
};

// ------------------------------------------------------------------------------------------------
// The two scalar slots of a canonical row, and a row written value by value (the VEC = false forms: W window cells, then the slots)
struct Slots { double v0, v1; };
template <bool DYN>
__device__ __forceinline__ Slots scalar_slots(const Lane& s, int total_step) {
    const double c0 = (double)s.cb, c1 = (double)s.cs;
    return {DYN ? c0 / (double)s.tb : c0, DYN ? c1 / (double)total_step : c1};
}
template <int W, typename OT, class F>
__device__ __forceinline__ void write_row(OT* o, F cell, const Slots& v) {
#pragma unroll
    for (int el = 0; el < W; ++el) o[el] = (OT)cell(el);
    o[W] = (OT)v.v0; o[W + 1] = (OT)v.v1;
}

// ------------------------------------------------------------------------------------------------
// Whole 16-byte pieces of rows (m % 4 = 0, an aligned obs) through the wave's run; otherwise rows value by value.  A wave of m % 4 != 0
// edges -- five actions per parent make most expansions such -- runs its first m & ~3 edges the fast way and the last one to three as a
// launch of their own (possible when both index arrays are given: edge i of the tail is edge head + i of the call)
template <int D, typename OT, class Part>
void launch_split(const KArgs& a, Part part) {
    const bool aligned = !a.obs || ((uintptr_t)a.obs & 15) == 0;
    const int head = a.n & ~3;
    if (aligned && head == a.n) { part(a, true); return; }
    if (!aligned || head == 0 || !a.src_index || !a.dst_index) { part(a, false); return; }
    KArgs h = a, t = a;
    h.n = head;
    t.n = a.n - head;
    t.src_index += head; t.dst_index += head;
    if (t.actions) t.actions += head;
    if (t.step_size) t.step_size += head;
    if (t.reward) t.reward += head;
    if (t.done) t.done += head;
    if (t.obs) t.obs = (char*)t.obs + (size_t)head * D * sizeof(OT);
    t.env_id_base += head;                                           // the counter RNG is keyed by the edge's index in the call
    part(h, true);
    part(t, false);                                                  // (its rows start where the head's end: 16-byte alignment is not needed here)
}

}  // namespace
