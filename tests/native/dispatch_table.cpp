// dispatch_table.cpp -- the dispatch of the env-batch entry points (snac_amd/csrc/snac_hip.hip: choose() / launch()) as a table, without a GPU.
// Built by `hipcc --offload-host-only` together with snac_hip.hip; every launch_* function of the kernel families is a stub here that
// records its name and the Choice fields it was given, and the three HIP calls snac_hip.hip makes are answered here too, so no runtime
// and no device is touched.  The real C ABI is called with descriptors and made-up, non-null pointers (aligned or misaligned on purpose:
// nothing is dereferenced on the host); after each call snac_last_kernel() and the stub's record are read.
//
// Output: one line per combination of entry point, kind, static / dynamic, row type, layout, alignment case (the addresses, and whether
// N is a multiple of 4) and plan count; the line lists the batch sizes of the grid at which the kernel, the launcher or a parameter
// changes (the format of tools/dispatch_table.py).  A list is printed once, numbered [id]; a later line with the same list says [=id].
// The grid of batch sizes: every value >= 4 that snac_tuning() prints, with +-1 and the nearest multiples of 4 and of 64 on either
// side, the LADDER of tools/dispatch_table.py, and 65 536.  `dispatch_table reduced` keeps the canonical and the ppo_plan layout and
// the aligned pointers only (the runs under a knob override: the environment is read once per process).
// tests/test_dispatch_host.py compares the sha256 of every run with tests/golden/dispatch_overrides.sha256, and the lines of the full run
// that carry a list (with the static float64 canonical aligned ones) with tests/golden/dispatch_table.txt.
#include "snac_units.h"

#include <cstdint>
#include <map>
#include <set>
#include <string>

static char g_rec[64];
#define REC(...) std::snprintf(g_rec, sizeof(g_rec), __VA_ARGS__)

extern "C" {
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "(no HIP runtime in this program)"; }
}

// ---- the stubs: the signatures of snac_units.h
namespace snac_detail {
void launch_tile1d(Op, bool, int E, int, const KArgs&, hipStream_t) { REC("tile1d E=%d", E); }
void launch_tile2d(Op, bool, int E, int, const KArgs&, hipStream_t) { REC("tile2d E=%d", E); }
void launch_tile3d(Op, bool, int E, int, const KArgs&, hipStream_t) { REC("tile3d E=%d", E); }
void launch_roll2d(const snac_env_desc*, const KArgs&, hipStream_t) { REC("roll2d"); }
void launch_roll2db(const snac_env_desc*, const KArgs&, int E, hipStream_t) { REC("roll2db E=%d", E); }
void launch_roll2dbv(const snac_env_desc*, const KArgs&, int E, hipStream_t) { REC("roll2dbv E=%d", E); }
void launch_roll2dt(const snac_env_desc*, const KArgs&, int E, hipStream_t) { REC("roll2dt E=%d", E); }
void launch_roll1dt(const snac_env_desc*, const KArgs&, int E, hipStream_t) { REC("roll1dt E=%d", E); }
void launch_roll1dl(const snac_env_desc*, const KArgs&, int form, hipStream_t) { REC("roll1dl form=%d", form); }
void launch_roll3d(const snac_env_desc*, const KArgs&, hipStream_t) { REC("roll3d"); }
void launch_roll3db(const snac_env_desc*, const KArgs&, hipStream_t) { REC("roll3db"); }
void launch_roll3dbv(const snac_env_desc*, const KArgs&, hipStream_t) { REC("roll3dbv"); }
void launch_step1d(const snac_env_desc*, const KArgs&, int form, hipStream_t) { REC("step1d form=%d", form); }
void launch_aux1d(const snac_env_desc*, const KArgs&, hipStream_t) { REC("aux1d"); }
void launch_edges1d(const snac_env_desc*, const KArgs&, hipStream_t) { REC("edges1d"); }
void launch_step2d(const snac_env_desc*, const KArgs&, int E, int form, hipStream_t) { REC("step2d E=%d form=%d", E, form); }
void launch_aux2d(const snac_env_desc*, const KArgs&, hipStream_t) { REC("aux2d"); }
void launch_step3d(const snac_env_desc*, const KArgs&, bool span, hipStream_t) { REC("step3d span=%d", span ? 1 : 0); }
void launch_step3dq(const snac_env_desc*, const KArgs&, int form, hipStream_t) { REC("step3dq form=%d", form); }
void launch_aux3d(const snac_env_desc*, const KArgs&, hipStream_t) { REC("aux3d"); }
void launch_trans2d(const snac_env_desc*, const KArgs&, int E, hipStream_t) { REC("trans2d E=%d", E); }
void launch_edges2d(const snac_env_desc*, const KArgs&, hipStream_t) { REC("edges2d"); }
void launch_trans3d(const snac_env_desc*, const KArgs&, hipStream_t) { REC("trans3d"); }
void launch_edges3d(const snac_env_desc*, const KArgs&, hipStream_t) { REC("edges3d"); }
void launch_reset(const snac_env_desc*, const KArgs&, hipStream_t) { REC("reset"); }
void launch_iou(const snac_env_desc*, const KArgs&, hipStream_t) { REC("iou"); }
}  // namespace snac_detail

// ---- the grid and the calls (nothing below knows the launchers)
namespace {

const int LADDER[] = {4, 64, 256, 1024, 2048, 3072, 3584, 4096, 8192, 12288, 16384, 20480, 24576, 28672, 32768, 36864, 40960, 45056, 49152, 57344, 65536, 81920,
                      98304, 131072, 196608, 262144, 278528, 376832, 475136, 475140, 524288, 557056, 786432, 1048576};   // tools/dispatch_table.py

struct Layout { const char* name; int frame_value, obs_scalars, obs_tail; bool not3d; };   // as BatchedDMPEnv.LAYOUTS sets the descriptor
const Layout LAYOUTS[] = {{"canonical", -1, SNAC_SCALARS_DEFAULT, 0, false},
                          {"ppo_plan", -1, SNAC_SCALARS_RAW, SNAC_TAIL_PLAN, false},
                          {"lnet1d", -1, SNAC_SCALARS_DEFAULT, SNAC_TAIL_POSITION, false},
                          {"lnet2d", 2, SNAC_SCALARS_NORM, 0, true},       // (frame_value 2: check_layout rejects it for 3D)
                          {"ppo", -1, SNAC_SCALARS_RAW, 0, false},
                          {"record", -1, SNAC_SCALARS_DEFAULT, SNAC_TAIL_RECORD, false}};

enum Entry { ROLL_NONE, ROLL_ALL, ROLL_LAST, ROLL_TILED, ROLL_RING, STEP_OBS, STEP_NOOBS, SCALAR_OBS, SCALAR_NOOBS, RESET, RESET_MASK, RESET_SCALAR, OBSERVE, IOU,
             EDGES, EDGES_END = EDGES + 8 };   // EDGES + bits: 1 = src_index, 2 = dst_index, 4 = obs
const char* const EDGE_NAMES[8] = {"trans/--", "trans/s-", "trans/-d", "trans/sd", "trans/--/obs", "trans/s-/obs", "trans/-d/obs", "trans/sd/obs"};
const char* entry_name(int e) {
    static const char* const names[] = {"rollout/NONE", "rollout/ALL", "rollout/LAST", "rollout/TILED", "rollout_ring", "step/obs", "step", "step_scalar/obs", "step_scalar",
                                        "reset", "reset(m)", "reset_scalar", "observe", "iou"};
    return e < EDGES ? names[e] : EDGE_NAMES[e - EDGES];
}
bool is_rollout(int e) { return e <= ROLL_RING; }
bool has_obs(int e) { return !(e == ROLL_NONE || e == STEP_NOOBS || e == SCALAR_NOOBS || e == IOU || (e >= EDGES && !((e - EDGES) & 4))); }

// made-up addresses; + off moves one off its 16-byte boundary
void* fake(uintptr_t base, int off = 0) { return (void*)(base + (uintptr_t)off); }

int call(int e, const snac_env_desc* d, int obs_off, int plans_off, int grid_off) {
    snac_state st = {(snac_env_hdr*)fake(0x10000000), (int32_t*)fake(0x20000000), fake(0x30000000, grid_off), fake(0x40000000, plans_off), (const int16_t*)fake(0x50000000),
                     (int64_t*)fake(0x60000000), (int64_t*)fake(0x70000000), (int64_t*)fake(0x80000000)};
    void* const obs = has_obs(e) ? fake(0x100000000ull, obs_off) : nullptr;
    float* const rew = (float*)fake(0x200000000ull);
    uint8_t* const done = (uint8_t*)fake(0x300000000ull);
    const int T = 4;
    switch (e) {
        case ROLL_NONE: return snac_rollout(d, &st, T, 0, nullptr, nullptr, SNAC_OBS_NONE, obs, rew, done, nullptr);
        case ROLL_ALL: return snac_rollout(d, &st, T, 0, nullptr, nullptr, SNAC_OBS_ALL, obs, rew, done, nullptr);
        case ROLL_LAST: return snac_rollout(d, &st, T, 0, nullptr, nullptr, SNAC_OBS_LAST, obs, rew, done, nullptr);
        case ROLL_TILED: return snac_rollout(d, &st, T, 0, nullptr, nullptr, SNAC_OBS_TILED, obs, rew, done, nullptr);
        case ROLL_RING: return snac_rollout_tiled(d, &st, T, 0, nullptr, nullptr, 2 * T, T, obs, rew, done, nullptr, nullptr);
        case STEP_OBS: case STEP_NOOBS: return snac_step(d, &st, 0, nullptr, nullptr, 1, obs, rew, done, nullptr);
        case SCALAR_OBS: case SCALAR_NOOBS: return snac_step_scalar(d, &st, 0, 1, 1, 1, obs, rew, done, nullptr);
        case RESET: return snac_reset(d, &st, nullptr, nullptr, obs, nullptr);
        case RESET_MASK: return snac_reset(d, &st, (const uint8_t*)fake(0x400000000ull), nullptr, obs, nullptr);
        case RESET_SCALAR: return snac_reset_scalar(d, &st, 0, obs, nullptr);
        case OBSERVE: return snac_observe(d, &st, obs, nullptr);
        case IOU: return snac_iou(d, &st, (double*)fake(0x500000000ull), nullptr);
        default: {                                                   // a wave of num_envs edges on a pool of num_envs rows
            const int bits = e - EDGES;
            return snac_transition(d, &st, d->num_envs, (bits & 1) ? (const int32_t*)fake(0x600000000ull) : nullptr, (bits & 2) ? (const int32_t*)fake(0x700000000ull) : nullptr, 0,
                                   (const int8_t*)fake(0x800000000ull), nullptr, obs, rew, done, nullptr);
        }
    }
}

uint64_t fnv1a64(const char* s) {
    uint64_t h = 1469598103934665603ull;
    for (; *s; ++s) h = (h ^ (unsigned char)*s) * 1099511628211ull;
    return h;
}

}  // namespace

int main(int argc, char** argv) {
    const bool reduced = argc > 1 && std::string(argv[1]) == "reduced";
    static char tuning[1 << 17];
    if (snac_tuning(tuning, (int32_t)sizeof(tuning)) != SNAC_OK) { std::fprintf(stderr, "snac_tuning: %s\n", snac_last_error()); return 1; }
    std::set<int> sizes(LADDER, LADDER + sizeof(LADDER) / sizeof(LADDER[0]));
    sizes.insert(65536);
    int knobs = 0;
    for (const char* p = tuning; *p; p = std::strchr(p, '\n') + 1, ++knobs) {   // "NAME=value  # what": the effective values
        const long long v = std::atoll(std::strchr(p, '=') + 1);
        if (v < 4) continue;
        for (long long n : {v - 1, v, v + 1, (v - 1) / 4 * 4, (v / 4 + 1) * 4, (v - 1) / 64 * 64, (v / 64 + 1) * 64})
            if (n >= 1) sizes.insert((int)n);
    }
    std::printf("# tests/native/dispatch_table.cpp%s: kernel (snac_last_kernel), launcher and the parameters it was given, by batch size: the batch sizes of the grid at which they change\n",
                reduced ? " reduced" : "");
    std::printf("# snac_tuning(): %d knobs, %zu bytes, fnv1a64 %016llx\n", knobs, std::strlen(tuning), (unsigned long long)fnv1a64(tuning));
    std::printf("# line: entry point, kind, static / dynamic, rows, layout, obs / plans / grid address mod 16 (0: aligned), num_plans, the batch sizes taken; [id] a list of changes, [=id] the same list as line [id]\n");
    std::printf("# layouts:");
    for (const Layout& l : LAYOUTS)
        if (!reduced || &l < LAYOUTS + 2) std::printf(" %s", l.name);
    std::printf("\n# grid: %zu batch sizes (trans/*: edges per call):", sizes.size());
    for (int n : sizes) std::printf(" %d", n);
    std::printf("\n");
    long calls = 0;
    std::map<std::string, int> lists;                                // a list of changes is printed once, as [id]; a line with the same list says [=id]
    for (int kind = SNAC_ENV_1D; kind <= SNAC_ENV_3D; ++kind)
        for (int dyn = 0; dyn < 2; ++dyn)
            for (int dt : {SNAC_OBS_F64, SNAC_OBS_F32})
                for (const Layout& l : LAYOUTS) {
                    if ((reduced && &l >= LAYOUTS + 2) || (l.not3d && kind == SNAC_ENV_3D)) continue;
                    for (int e = 0; e < EDGES_END; ++e)
                        // the cases: obs on 16 bytes and on 8 (where the call has one), plans on 16 and on 8 (3D rollouts and snac_iou: the
                        // calls that look), grid on 16 and on 8 (snac_iou), 400 plans and TB_MAX + 1 (3D rollouts)
                        for (int obs_off = 0; obs_off <= ((has_obs(e) && !reduced) ? 8 : 0); obs_off += 8)
                            for (int plans_off = 0; plans_off <= ((((kind == SNAC_ENV_3D && is_rollout(e)) || e == IOU) && !reduced) ? 8 : 0); plans_off += 8)
                                for (int grid_off = 0; grid_off <= ((e == IOU && !reduced) ? 8 : 0); grid_off += 8)
                                    for (int P : {400, TB_MAX + 1}) {
                                        if (P != 400 && !(kind == SNAC_ENV_3D && is_rollout(e))) continue;
                                        snac_env_desc d;
                                        std::memset(&d, 0, sizeof(d));
                                        d.kind = kind; d.dynamic = dyn; d.num_plans = P; d.obs_dtype = dt; d.seed = 1;
                                        d.frame_value = l.frame_value; d.obs_scalars = l.obs_scalars; d.obs_tail = l.obs_tail;
                                        for (int odd = 0; odd < 2; ++odd) {          // whole groups of four envs (N % 4 == 0: rows in 16-byte pieces), then the other sizes
                                            std::string list, prev;
                                            for (int n : sizes) {
                                                if (((n & 3) != 0) != (odd != 0)) continue;
                                                d.num_envs = n;
                                                g_rec[0] = 0;
                                                const int rc = call(e, &d, obs_off, plans_off, grid_off);
                                                ++calls;
                                                char now[160];
                                                if (rc != SNAC_OK) std::snprintf(now, sizeof(now), "error %d (%s)", rc, snac_last_error());
                                                else std::snprintf(now, sizeof(now), "%s %s", snac_last_kernel(), g_rec);
                                                if (prev != now) list += (prev.empty() ? "" : "  |  ") + std::to_string(n) + ": " + now;
                                                prev = now;
                                            }
                                            const auto seen = lists.emplace(list, (int)lists.size() + 1);
                                            std::printf("%-15s %dD %s %s %-9s obs%d plans%d grid%d P=%-4d %s  ", entry_name(e), kind, dyn ? "dyn" : "sta", dt == SNAC_OBS_F32 ? "f32" : "f64",
                                                        l.name, obs_off, plans_off, grid_off, P, odd ? "N%4>0" : "N%4=0");
                                            if (seen.second) std::printf("[%d] %s\n", seen.first->second, list.c_str());
                                            else std::printf("[=%d]\n", seen.first->second);
                                        }
                                    }
                }
    std::printf("# %ld calls\n", calls);
    return 0;
}
