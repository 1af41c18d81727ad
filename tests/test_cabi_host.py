"""CPU-side checks (no GPU, no compute launches): the C-ABI library loads and exports every symbol the header
declares, argument validation, the host-side plan packing, sharding arithmetic, and that the product refuses to
run without its HIP path."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import helpers


def _header_functions():
    src = open(os.path.join(helpers.ROOT, "include", "snac_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(snac_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from snac_amd import _lib

    L = _lib.lib()
    names = _header_functions()
    assert set(names) == set(_lib.EXPORTS), names
    for n in names:
        assert hasattr(L, n), n
    assert L.snac_version() == _lib.ABI_VERSION
    # EXPORTS is derived from the header, so the other direction is asked of the library itself: it defines no snac_* symbol
    # that the header does not declare
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True, timeout=60).stdout
    defined = sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("snac_"))
    assert defined == names


def test_kernel_source_header_holds_no_unit_map_and_no_host_side():
    """snac_dev.h is kernel source only (its hash stamps profiles/traffic.json): snac_units.h alone includes it, and the map of the
    translation units, the shared checks, the dispatch and the launcher declarations stay out of it."""
    csrc = os.path.join(helpers.ROOT, "snac_amd", "csrc")
    includers = sorted(f for f in os.listdir(csrc) if os.path.isfile(os.path.join(csrc, f))
                       and re.search(r'#\s*include\s*[<"]snac_dev\.h[>"]', open(os.path.join(csrc, f), errors="replace").read()))
    assert includers == ["snac_units.h"]
    dev = open(os.path.join(csrc, "snac_dev.h")).read()
    for word in ("launch_", "check_common", "nodes_check", "play_check", "choose("):
        assert word not in dev, word
    assert not re.findall(r"\bk_\w*\.hip\b", dev)


def test_traffic_profile_is_stamped_with_the_kernel_source():
    """profiles/traffic.json carries the counters of the headline kernel as it is now: a change to snac_dev.h or k_roll2d.hip takes
    the FETCH_SIZE / WRITE_SIZE passes again in the same change (bench.py reports no measured traffic otherwise)."""
    import json

    from snac_amd import _lib

    with open(os.path.join(helpers.ROOT, "profiles", "traffic.json")) as fh:
        assert json.load(fh)["source_sha16"] == _lib.kernel_source_sha16()


def test_env_sizes_match_reference_constants():
    from snac_amd import _lib

    want = {(1, 0): (7, 3, 750, 2, 1, 34, 1, 30), (1, 1): (7, 3, 750, 2, 1, 34, 1, 30),
            (2, 0): (51, 5, 600, 3, 26, 26, 20, 20), (2, 1): (51, 5, 600, 3, 26, 26, 20, 20),
            (3, 0): (51, 8, 1300, 3, 26, 26, 20, 20), (3, 1): (51, 8, 1000, 3, 26, 26, 20, 20)}
    for (k, d), w in want.items():
        s = _lib.env_sizes(k, d)
        assert (s.obs_dim, s.num_actions, s.total_step, s.half_window, s.env_height, s.env_width, s.plan_height, s.plan_width) == w
    with pytest.raises(_lib.SnacError):
        _lib.env_sizes(7, 0)


def test_argument_validation_happens_before_any_launch():
    from snac_amd import _lib

    L = _lib.lib()
    d = _lib.EnvDesc(2, 1, 16, 4, 0, 0, 1, 0, 0, 0)
    st = _lib.State(0, 0, 0, 0, 0, 0, 0, 0)   # null pointers
    assert L.snac_step(C.byref(d), C.byref(st), 0, None, None, 0, None, None, None, None) == -1
    assert b"null pointer" in L.snac_last_error()
    bad = _lib.EnvDesc(9, 1, 16, 4, 0, 0, 1, 0, 0, 0)
    assert L.snac_reset(C.byref(bad), C.byref(st), None, None, None, None) == -1
    assert b"kind" in L.snac_last_error()
    bad = _lib.EnvDesc(2, 1, 0, 4, 0, 0, 1, 0, 0, 0)
    assert L.snac_iou(C.byref(bad), C.byref(st), None, None) == -1
    assert L.snac_rollout(None, None, 1, 0, None, None, 0, None, None, None, None) == -1
    # trajectory memory: arguments first, and without a GPU the call reports an error instead of handing out host memory
    p = C.c_void_p()
    assert L.snac_traj_alloc(0, 0, C.byref(p)) == -1 and b"bytes" in L.snac_last_error()
    assert L.snac_traj_alloc(1 << 20, 0, None) == -1
    assert L.snac_traj_free(None) == 0
    assert L.snac_traj_free(C.c_void_p(0x1000)) == -1 and b"snac_traj_alloc" in L.snac_last_error()
    import torch
    if not torch.cuda.is_available():
        assert L.snac_traj_alloc(1 << 20, 0, C.byref(p)) < 0 and not p.value


# ---- the alignment of the caller's state arrays (include/snac_hip.h, "Alignment of the state arrays"): refused on entry, on the host
_ARRAYS = ("hdr", "episode", "grid", "plans", "plan_tb", "stat_episodes", "stat_return", "stat_iou_fx")   # snac_state's fields, in order
_BASE = 1 << 20                                                        # a placeholder on a 512-byte boundary (never dereferenced)
# (entry point, env kind, {argument position: value}, what refuses the call once the state has passed): a representative of every
# translation unit that takes a state -- snac_hip.hip, k_misc.hip, k_nodes.hip, k_nodes_obs.hip, k_eval.hip, k_replay.hip -- each with an
# argument check of its own BEHIND the state's, so that nothing here can reach a launch.  snac_step, snac_step_scalar and snac_reset have
# no later check and share check_common with the others; k_mailbox.hip's entry points need a mailbox, which is page-locked device memory.
_ENTRY = [
    ("snac_iou", 2, {}, b"null out"), ("snac_observe", 2, {}, b"null obs"), ("snac_reset_scalar", 2, {2: -1}, b"plan_idx out of range"),
    ("snac_rollout", 2, {2: -1}, b"T must be"), ("snac_rollout_rec", 2, {2: -1}, b"T must be"), ("snac_rollout_tiled", 2, {2: -1}, b"outside the ring"),
    ("snac_transition", 2, {2: -1}, b"m must be"),
    ("snac_export_grid", 2, {}, b"null out"), ("snac_import_state", 2, {2: -1}, b"m must be"), ("snac_make_plans", 2, {2: -1}, b"plan rows out of range"),
    ("snac_plans_from_grids", 2, {2: 2, 3: 99}, b"plan rows out of range"), ("snac_episodic_sums", 2, {2: _BASE + 4, 3: _BASE}, b"out3 and scratch"),
    ("snac_nodes2d_pack", 2, {4: _BASE, 5: 0}, b"pool_rows"), ("snac_nodes2d_unpack", 2, {1: _BASE, 2: 0}, b"pool_rows"),
    ("snac_transition_nodes2d", 2, {2: _BASE, 3: 0}, b"pool_rows"), ("snac_nodes1d_pack", 1, {4: _BASE, 5: 0}, b"pool_rows"),
    ("snac_nodes3d_unpack", 3, {1: _BASE, 2: 0}, b"pool_rows"),
    ("snac_observe_nodes2d", 2, {2: _BASE, 3: 0}, b"pool_rows"), ("snac_observe_nodes1d", 1, {2: _BASE, 3: 0}, b"pool_rows"),
    ("snac_evaluate_nodes2d", 2, {2: _BASE, 3: 0}, b"pool_rows"), ("snac_evaluate_nodes3d", 3, {2: _BASE, 3: 0}, b"pool_rows"),
    ("snac_replay_gather", 2, {2: 1}, b"cap must be"), ("snac_replay_gather_tiled", 2, {2: 1}, b"cap must be"),
    ("snac_replay_gather_nstep", 2, {2: 1}, b"cap must be"), ("snac_replay_gather_windows", 2, {2: 1}, b"cap must be"),
    ("snac_replay_gather_onpolicy", 2, {2: 1}, b"cap must be"),
]


def _header_alignments():
    """{array: bytes} as the header's block states them."""
    src = open(os.path.join(helpers.ROOT, "include", "snac_hip.h")).read()
    block = re.search(r"/\* Alignment of the state arrays\..*?\*/", src, flags=re.S).group()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^ \* {5}(\w+) +(\d+) {2,}\S", block, flags=re.M)}


def _call(name, kind, fixed, pointers):
    """The entry point with a state of these eight pointers; every other argument NULL / 0 but `fixed`.  -> (status, error text)"""
    from snac_amd import _lib

    L = _lib.lib()
    d = _lib.EnvDesc(kind, 1, 16, 4, 0, 0, 1, 0, 0, 0)
    st = _lib.State(*pointers)
    args, states = [], 0
    for i, t in enumerate(_lib.PROTOTYPES[name][1]):
        if t is C.POINTER(_lib.EnvDesc):
            args.append(C.byref(d))
        elif t is C.POINTER(_lib.State):
            args.append(None if states else C.byref(st))              # (a second state, the source of snac_plans_from_grids: absent)
            states += 1
        else:
            args.append(fixed.get(i, None if t is C.c_void_p or issubclass(t, C._Pointer) else 0))
    rc = getattr(L, name)(*args)
    return rc, L.snac_last_error()


def test_header_states_an_alignment_for_every_state_array():
    from snac_amd import _lib

    assert tuple(f for f, _ in _lib.State._fields_) == _ARRAYS
    want = _header_alignments()
    assert sorted(want) == sorted(_ARRAYS), want
    assert all(v in (4, 8, 16) for v in want.values()), want
    assert want["hdr"] == 16 and want["plan_tb"] >= 4                  # the struct's own comment; the word read of k_rollout2d / k_rollout2db


def test_the_state_check_enforces_the_numbers_of_the_header():
    """What the library enforces, found by asking it: the smallest power-of-two offset from a 512-byte boundary at which an array passes
    the state's check (the call then fails its own later check) is the number the header's block gives for that array."""
    want = _header_alignments()
    for i, name in enumerate(_ARRAYS):
        enforced = None
        for off in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            p = [_BASE] * 8
            p[i] = _BASE + off
            rc, msg = _call("snac_iou", 2, {}, p)
            assert rc == -1
            if b"null out" in msg:
                enforced = off
                break
            assert msg == b"snac_state.%s must be %d-byte aligned" % (name.encode(), want[name]), (name, off, msg)
        assert enforced == want[name], (name, enforced, want[name])


@pytest.mark.parametrize("entry", _ENTRY, ids=[e[0] for e in _ENTRY])
def test_a_misaligned_state_array_is_refused_before_anything_else_of_the_state_is_used(entry):
    """Each of the eight arrays in turn at every power-of-two offset below its requirement, the other seven aligned placeholders: -1 and
    the array's name.  The same array at exactly its requirement past a 512-byte boundary passes, and the call fails its later check."""
    fn, kind, fixed, later = entry
    want = _header_alignments()
    rc, msg = _call(fn, kind, fixed, [_BASE] * 8)
    assert rc == -1 and later in msg, (fn, msg)                        # the later check itself, with every array aligned
    for i, name in enumerate(_ARRAYS):
        for off in (1, 2, 4, 8):
            if off >= want[name]:
                continue
            p = [_BASE + 512 * (j + 1) for j in range(8)]
            p[i] += off
            rc, msg = _call(fn, kind, fixed, p)
            assert rc == -1 and msg == b"snac_state.%s must be %d-byte aligned" % (name.encode(), want[name]), (fn, name, off, msg)
        p = [_BASE + 512 * (j + 1) for j in range(8)]
        p[i] += want[name]
        rc, msg = _call(fn, kind, fixed, p)
        assert rc == -1 and later in msg and b"snac_state." not in msg, (fn, name, msg)


def test_the_source_state_of_plans_from_grids_is_held_to_the_same_alignment():
    from snac_amd import _lib

    L = _lib.lib()
    d = _lib.EnvDesc(2, 1, 16, 4, 0, 0, 1, 0, 0, 0)
    st = _lib.State(*[_BASE] * 8)
    src = _lib.State(_BASE, 0, _BASE + 8, 0, 0, 0, 0, 0)           # hdr and grid are what the call reads of it
    assert L.snac_plans_from_grids(C.byref(d), C.byref(st), 2, 0, C.byref(src), 16, None, None, None, None) == -1
    assert L.snac_last_error() == b"snac_state.grid must be 16-byte aligned"


def test_hdr_struct_is_16_bytes():
    src = open(os.path.join(helpers.ROOT, "include", "snac_hip.h")).read()
    assert "int16_t ep_return" in src and "int16_t cross" in src

    class Hdr(C.Structure):
        _fields_ = [("pos_r", C.c_int8), ("pos_c", C.c_int8), ("flags", C.c_uint8), ("reserved", C.c_uint8),
                    ("cb", C.c_int16), ("cs", C.c_int16), ("tb", C.c_int16), ("pidx", C.c_int16), ("ep", C.c_int16), ("cross", C.c_int16)]

    assert C.sizeof(Hdr) == 16


def test_static_plans_and_packing():
    from snac_amd import plans

    z = helpers.static_plans_npz()
    for pc in (0, 1, 2):
        assert np.array_equal(plans.static_plan(1, pc), z["1d_p%d" % pc])
    for pc in (0, 1):
        assert np.array_equal(plans.static_plan(2, pc), z["2d_p%d" % pc])
        assert np.array_equal(plans.static_plan(3, pc), z["3d_p%d" % pc])
    with pytest.raises(ValueError):
        plans.static_plan(2, 2)
    # 2D: bit j of row i = plan[3 + i, 3 + j]; total_brick floored at 30
    full = plans.dataset(2, "sparse", "train")
    packed, tb = plans.pack_plans(2, full)
    assert packed.shape == (400, 20) and packed.dtype == np.uint32
    for p in (0, 17, 399):
        bits = (packed[p][:, None] >> np.arange(20, dtype=np.uint32)[None, :]) & 1
        assert np.array_equal(bits, full[p, 3:23, 3:23].astype(np.uint32))
        assert tb[p] == max(int(full[p].sum()), 30)
    assert (full.reshape(400, -1).sum(1) < 30).sum() == 197
    packed, tb = plans.pack_plans(3, plans.dataset(3, "dense", "train"))
    assert packed.shape == (400, 400) and tb.min() == 306 and tb.max() == 654
    packed, tb = plans.pack_plans(1, plans.dataset(1))
    assert packed.shape == (400, 32) and tb.min() == 592 and tb.max() == 604 and np.all(packed[:, 30:] == 0)
    bad = np.zeros((1, 26, 26))
    bad[0, 0, 0] = 1
    with pytest.raises(ValueError):
        plans.pack_plans(2, bad)
    with pytest.raises(ValueError):
        plans.pack_plans(2, np.full((1, 26, 26), 0.5))


def test_shard_arithmetic():
    from snac_amd import dist

    for total, world in ((524288, 8), (10, 3), (7, 8), (65536, 1)):
        spans = [dist.shard(total, r, world) for r in range(world)]
        assert sum(n for n, _ in spans) == total
        pos = 0
        for n, base in spans:
            assert base == pos
            pos += n
    assert dist.shard(524288, 3, 8) == (65536, 3 * 65536)
    with pytest.raises(ValueError):
        dist.shard(8, 8, 8)


def test_product_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from snac_amd import SnacError
    from snac_amd.batched import BatchedDMPEnv
    from snac_amd.envs import deep_mobile_printing_2d1r_static

    with pytest.raises(SnacError):
        BatchedDMPEnv(2, True, 8)
    with pytest.raises(SnacError):
        deep_mobile_printing_2d1r_static(plan_choose=0)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(helpers.ROOT, "snac_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".hpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("no oracle", ""), os.path.join(dirpath, f)


def test_bench_gpus_flag_must_match_the_world_size():
    """bench.py --gpus N under a torch.distributed environment of another size exits non-zero before touching torch."""
    import subprocess
    import sys

    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "WORLD_SIZE=3" in r.stderr and not r.stdout.strip()


def test_dispatch_table_is_one_table_with_documented_entries():
    """snac_tuning(): every batch-size threshold / switch that selects a kernel, with its effective value and what it decides (host-only
    call: no GPU needed); the defaults the tests of both sides of each threshold rely on."""
    from snac_amd import _lib

    t = _lib.tuning()
    assert len(t) >= 62 and all(k.startswith("SNAC_") and what for k, (v, what) in t.items())
    want = {"SNAC_3D_PIPELINE": 1, "SNAC_2D_STAGE_MIN_F64": 32769, "SNAC_2D_STAGE_MIN_F32": 32768, "SNAC_2D_TP_MAX_F64": 19456, "SNAC_2D_TP_GAP_LO": 15873,
            "SNAC_2D_TP_GAP_HI": 16384, "SNAC_2D_TP_MAX_F32": 30719, "SNAC_2D_TP_VAR_MAX_PLAN": 49152, "SNAC_2D_TP_VAR_MAX_SHORT": 6144, "SNAC_2D_TILE32_MIN": 22528,
            "SNAC_1D_TP_MAX_F64": 65536, "SNAC_1D_TP_EB8_MIN": 3584, "SNAC_NODES2D_NT": 1, "SNAC_STEP3D_NTLOAD_MIN": 376832, "SNAC_STEP3D_HUGE_MIN": 557056, "SNAC_STEP3D_HUGE_FORM": 3, "SNAC_STEP3D_FORM": -1, "SNAC_STEP2D_PLAIN_LO": 20480, "SNAC_STEP2D_RES_HI": 278528, "SNAC_STEP2D_PLAIN_HI": 475136, "SNAC_STEP2D_HUGE_MIN": 475137, "SNAC_STEP2D_HUGE_FORM": 2, "SNAC_STEP2D_FORM": -1, "SNAC_1D_TP_MAX_F32": 65536, "SNAC_3D_BLOCK_MIN_F64": 4096, "SNAC_3D_BLOCK_MIN_F32": 4096,
            "SNAC_STEP3D_SPAN_MIN": 81920, "SNAC_3D_BLOCK_VAR": 1, "SNAC_3D_BLOCK_VAR_MIN": 64, "SNAC_3D_BLOCK_VAR_PLAN_F64": 10240, "SNAC_3D_BLOCK_VAR_PLAN_F32": 16384,
            "SNAC_2D_BLOCK": 1, "SNAC_2D_BLOCK_MIN_F64": 11264, "SNAC_2D_BLOCK_MAX_F64": 32768, "SNAC_2D_BLOCK_MIN_F32": 15360, "SNAC_2D_BLOCK_MAX_F32": 32768,
            "SNAC_2D_BLOCK_TWO_F64": 16384, "SNAC_2D_BLOCK_TWO_F32": 16385, "SNAC_2D_BLOCK_VAR_MIN": 6148, "SNAC_2D_BLOCK_VAR_MAX": 32768, "SNAC_2D_BLOCK_VAR_TWO": 16385, "SNAC_STEP3D_QUARTER": 1, "SNAC_STEP3D_QUARTER_MIN": 4, "SNAC_STEP3D_QUARTER_MAX": 1 << 30, "SNAC_2D_BLOCK_FOUR_MAX_F64": 38912, "SNAC_2D_BLOCK_FOUR_MAX_F32": 45056, "SNAC_STEP_VAR_MIN_SHORT": 24576, "SNAC_STEP_VAR_FULL_F64": 45056, "SNAC_STEP_VAR_FULL_F32": 32769, "SNAC_STEP_VAR3_MIN": 24576}
    import os
    for k, v in want.items():
        if k not in os.environ:
            assert t[k][0] == v, (k, t[k])


def test_round5_entry_points_validate_their_arguments_before_any_hip_call():
    from snac_amd import _lib

    L = _lib.lib()
    mb = C.c_void_p()
    big = _lib.EnvDesc(2, 1, 257, 4, 0, 0, 1, 0, 0, 0)             # a mailbox steps four wavefronts: 256 envs at most
    assert L.snac_mailbox_create(C.byref(big), 0, C.byref(mb)) != 0 and b"1 .. 256" in L.snac_last_error() and not mb.value
    assert L.snac_mailbox_create(None, 0, C.byref(mb)) != 0
    assert L.snac_mailbox_step(None, None, None, 0, 1) != 0 and b"null mailbox" in L.snac_last_error()
    assert L.snac_mailbox_touch(None) != 0
    assert L.snac_mailbox_settle(None) == 0 and L.snac_mailbox_quit(None) == 0 and L.snac_mailbox_destroy(None) == 0   # nothing to wait for / end
    assert not L.snac_mailbox_row(None) and not L.snac_mailbox_reward(None) and not L.snac_mailbox_done(None)
    d = _lib.EnvDesc(2, 1, 16, 4, 0, 0, 1, 0, 0, 0)
    st = _lib.State(*[1 << 20] * 8)                                # (aligned, never dereferenced: every call below fails its checks first)
    assert L.snac_plans_from_grids(C.byref(d), C.byref(st), 2, 3, None, 0, None, None, None, None) != 0 and b"out of range" in L.snac_last_error()
    assert L.snac_plans_from_grids(C.byref(d), C.byref(st), 2, 0, None, 0, None, None, None, None) != 0 and b"exactly one" in L.snac_last_error()
    mem = (C.c_double * (2 * 676))()
    assert L.snac_plans_from_grids(C.byref(d), C.byref(st), 2, 0, None, 0, None, mem, None, None) != 0 and b"total_brick" in L.snac_last_error()
    buf = C.create_string_buffer(8)
    assert L.snac_tuning(buf, 8) != 0 and L.snac_tuning(None, 0) != 0
