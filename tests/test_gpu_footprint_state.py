"""GPU: no priority-tree writer, node-pool mover or state writer writes outside its outputs (tests/guard.py, as tests/test_gpu_footprint.py
does for the env-batch calls and tests/test_gpu_footprint_nodes.py for the node pools' edges; default knobs, in this process).

  * snac_prio_init / snac_prio_update / snac_prio_fill: the tree's buffer carved at exactly tree.bytes, for trees whose last groups are
    ragged (1, 63, 65, 4095, 4097) and exactly full (64, 4096: no padding behind the last leaf group).  Reference: image() of
    tests/test_gpu_prio.py over the numpy leaves of tests/test_prio_host.py.  index and priority are carved inputs.
  * snac_make_plans, snac_plans_from_grids, snac_import_state, snac_nodes{1,2,3}d_unpack: the state arrays a snac_state points to --
    hdr, episode, grid, plans, plan_tb and the sums -- all carved (bind()).  References: the CPU oracle's generator and rasteriser, numpy
    for the grids, a twin env / twin pool in plain tensors for import and the movers (pinned by tests/test_gpu_mcts.py and
    tests/test_gpu_nodes*.py).  Rows outside the range a call names are byte-equal before and after.
  * snac_nodes{1,2,3}d_pack: into a pool carved 128 bytes past a 512-byte boundary.
Every case ends with arena.check()."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import guard
import helpers
from test_gpu_footprint import plan_tables
import test_prio_host as ref
from test_gpu_footprint_nodes import EDGES
from test_gpu_prio import S, SAMPLER, SEED, check_tree, make_priorities

pytestmark = pytest.mark.gpu

TREES = (1, 63, 64, 65, 4095, 4096, 4097)
TABLE_ROWS = 9                                                         # plan rows of the state cases: first 0 / 3, up to 5 rows written
FIRSTS, COUNTS = (0, 3), (1, 3, 4, 5)                                   # a wave per plan row / state, four per block
STATE = ("_hdr", "_episode", "_grid", "_plans", "_plan_tb", "_stats")


def _note(entry, sizes, where, seconds):
    line = "%-30s sizes %-36s %-44s %.2f s" % (entry, " ".join(str(n) for n in sizes), where, seconds)
    print(line)
    d = os.environ.get("SNAC_FOOTPRINT_TABLE_DIR")
    if d:
        with open(os.path.join(d, "footprint_state.txt"), "a") as f:
            f.write(line + "\n")


def _bytes(t):
    return t.cpu().numpy().tobytes() if hasattr(t, "cpu") else np.ascontiguousarray(t).tobytes()


def _same(got, want, what):
    assert _bytes(got) == _bytes(want), what


# ---- the priority tree ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entries", TREES)
def test_priority_tree_writers(entries):
    import torch
    from snac_amd import priority

    t0 = time.time()
    dev = torch.device("cuda", torch.cuda.current_device())
    nbytes = ref.layout(entries)[0]
    A = guard.Arena(nbytes + 5 * 8 * 4096 + 14 * (guard.BAND + 1024), dev)
    with guard.allocations(priority, arena=A):
        tree = priority.PriorityTree(entries, dev, scale_log2=S, seed=SEED, sampler_id=SAMPLER)
    lo = A.buf.data_ptr()
    assert tree.bytes == nbytes == tree.buffer.numel() and lo <= tree.buffer.data_ptr() < lo + A.buf.numel()
    assert [v[1] - v[0] for v in A.views] == [nbytes], "the buffer is carved at exactly tree.bytes"
    rng = np.random.default_rng(entries)
    w, mx = np.zeros(entries, np.uint32), 1 << S

    def check(what):
        check_tree(tree, w, mx, what)
        A.check()

    check("init")
    for n in (0, 1, 64, 65, 4096):
        idx = rng.integers(0, entries, n).astype(np.int32)
        if n >= 64:                                                    # out of range on both sides, and duplicates with different priorities
            idx[[3, 17, 40, 41]] = (-1, entries, -(1 << 31), (1 << 31) - 1)
            idx[50:56] = idx[20]
        p = make_priorities(rng, n)
        if n == 1:
            p[0] = 0.75
        index = A.carve((n,), torch.int32, name="index (input) n = %d" % n).copy_(torch.from_numpy(idx))
        pri = A.carve((n,), torch.float32, name="priority (input) n = %d" % n).copy_(torch.from_numpy(p))
        tree.update(index, pri)
        if n:
            mx = max(mx, ref.apply_update(w, idx.astype(np.int64), p, S))
        check("update n = %d" % n)
        _same(index, idx, "index is an input"), _same(pri, p, "priority is an input")
    # fill: the single last entry, a span across a 64- and a 4096-entry boundary (as far as the tree goes), the whole tree
    at = min(50, entries - 1)
    for first, count in ((entries - 1, 1), (at, min(4100, entries - at)), (0, entries)):
        for p, weight in ((0.25, 1 << (S - 2)), (None, mx), (1e-9, 1)):
            tree.fill(first, count, p)
            w[first:first + count] = weight
            check("fill %d + %d with %r" % (first, count, p))
    _note("snac_prio_init/_update/_fill", [entries], "buffer of exactly tree.bytes, +0", time.time() - t0)


# ---- state arrays bound through the C ABI -----------------------------------------------------------------------------------------------
def bind(env, A):
    """Re-point the env's snac_state at copies of its arrays carved from A: hdr, episode, grid, plans, plan_tb and the three sums.  Every
    call on the env then reaches the library with these addresses.  Returns {name: a clone of the array as it is now}."""
    for name in STATE:
        t = getattr(env, name)
        setattr(env, name, A.carve(tuple(t.shape), t.dtype, name=name[1:]).copy_(t))
    s = env._state
    s.hdr, s.episode, s.grid = env._hdr.data_ptr(), env._episode.data_ptr(), env._grid.data_ptr()
    s.plans, s.plan_tb = env._plans.data_ptr(), env._plan_tb.data_ptr()
    s.stat_episodes, s.stat_return, s.stat_iou_fx = (env._stats[i].data_ptr() for i in range(3))
    env._fast = None
    return snapshot(env)


def snapshot(env):
    return {name: getattr(env, name).clone() for name in STATE}


def restore(env, saved):
    for name in STATE:
        getattr(env, name).copy_(saved[name])


def _env(kind, n, seed=11, rows=TABLE_ROWS, ticks=4):
    from snac_amd import BatchedDMPEnv

    _, shaped = plan_tables(kind, True)
    env = BatchedDMPEnv(kind, True, n, plans=shaped[:rows], seed=seed, total_step=12)
    env.reset()
    env.rollout(ticks, obs=None)
    return env


def _state_bytes(kind, n):
    from snac_amd import _lib

    sz = _lib.env_sizes(kind, True)
    return n * (16 + 4 + 24 + sz.grid_elems * sz.grid_elem_bytes) + TABLE_ROWS * (sz.plan_elems * 4 + 2) + 6 * (guard.BAND + 1024)


def _unchanged_outside(env, saved, names, rows, what):
    """Rows outside `rows` of the arrays `names` are byte-equal to what they were."""
    import torch

    for name in names:
        t = getattr(env, name)
        keep = torch.ones(t.shape[0], dtype=torch.bool, device=t.device)
        keep[torch.as_tensor(np.asarray(rows, np.int64), device=t.device)] = False
        _same(t[keep], saved[name][keep], "%s: %s outside the rows written" % (what, name[1:]))


def _packed(kind, full):
    """Plan rows in the device layout from [m, 30] / [m, 26, 26] integer arrays."""
    from snac_amd import plans

    packed, _ = plans.pack_plans(kind, np.asarray(full, np.float64))
    return packed.view(np.int32) if kind == 2 else packed


def _call(fn, env, *args):
    import torch

    vp = [C.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a for a in args]
    return fn(C.byref(env._desc), C.byref(env._state), *vp, C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_make_plans_random_form(kind):
    """Rows first .. first + count - 1 of plans and plan_tb equal the oracle's generator; every other row, and every other state array, is
    what it was; area_out carved and NULL."""
    import torch
    from snac_amd import _lib

    t0 = time.time()
    L, orc = _lib.lib(), helpers.oracle()
    env = _env(kind, 4)
    A = guard.Arena(_state_bytes(kind, 4) + 40 * (guard.BAND + 1024), env.device)
    saved = bind(env, A)
    seed, base = 99, 12345
    for sparse in ((0,) if kind == 1 else (0, 1)):
        for first in FIRSTS:
            for count in COUNTS:
                table, tb = orc.make_plans(kind, sparse, seed, base + first, count)
                rows = _packed(kind, table.reshape((count, 30) if kind == 1 else (count, 26, 26)))
                cells = table.sum(1) if kind == 1 else (table != 0).sum(1)
                for with_area in (True, False):
                    restore(env, saved)
                    area = A.carve((count,), torch.int32, name="area_out") if with_area else None
                    _lib.check(_call(L.snac_make_plans, env, first, count, sparse, seed, base, None, area))
                    what = "make_plans %dD sparse %d first %d count %d" % (kind, sparse, first, count)
                    _same(env._plans[first:first + count], rows, what + ": plan rows")
                    _same(env._plan_tb[first:first + count], tb.astype(np.int16), what + ": plan_tb")
                    if with_area:
                        _same(area, cells.astype(np.int32), what + ": area_out")
                    _unchanged_outside(env, saved, ("_plans", "_plan_tb"), range(first, first + count), what)
                    for name in ("_hdr", "_episode", "_grid", "_stats"):
                        _same(getattr(env, name), saved[name], what + ": " + name)
                    A.check()
    _note("snac_make_plans %dD random" % kind, COUNTS, "first 0 3, table of 9, area_out carved / NULL", time.time() - t0)


@pytest.mark.parametrize("kind", [2, 3])
def test_make_plans_from_vertices_outside_the_board(kind):
    """int8 vertices outside 0 .. 19 next to in-range ones: the oracle's rasteriser on the clamped vertices."""
    import torch
    from snac_amd import _lib

    t0 = time.time()
    L, orc = _lib.lib(), helpers.oracle()
    env = _env(kind, 4)
    A = guard.Arena(_state_bytes(kind, 4) + 40 * (guard.BAND + 1024), env.device)
    saved = bind(env, A)
    rng = np.random.default_rng(kind)
    pool = np.int8([-128, -1, 20, 127, 0, 19, 3, 11, 16])
    for sparse in (0, 1):
        for first in FIRSTS:
            for count in COUNTS:
                v = pool[rng.integers(0, len(pool), (count, 6))]
                v[0] = (-128, 127, 20, -1, 7, 12)                      # every clamp in one triangle
                full, cells = np.zeros((count, 26, 26), np.int64), np.zeros(count, np.int64)
                for i, q in enumerate(np.clip(v.astype(np.int64), 0, 19)):
                    img, cells[i] = orc.raster_triangle(q[0::2], q[1::2], sparse)
                    full[i, 3:23, 3:23] = img * (6 if kind == 3 else 1)
                restore(env, saved)
                verts = A.carve((count, 6), torch.int8, name="vertices (input)").copy_(torch.from_numpy(v))
                area = A.carve((count,), torch.int32, name="area_out")
                _lib.check(_call(L.snac_make_plans, env, first, count, sparse, 0, 0, verts, area))
                what = "make_plans %dD vertices sparse %d first %d count %d" % (kind, sparse, first, count)
                _same(env._plans[first:first + count], _packed(kind, full), what + ": plan rows")
                _same(env._plan_tb[first:first + count], (np.maximum(cells, 30) if kind == 2 else 6 * cells).astype(np.int16), what + ": plan_tb")
                _same(area, cells.astype(np.int32), what + ": area_out")
                _same(verts, v, what + ": the vertices are an input")
                _unchanged_outside(env, saved, ("_plans", "_plan_tb"), range(first, first + count), what)
                A.check()
    _note("snac_make_plans %dD vertices" % kind, COUNTS, "first 0 3, vertices -128 -1 20 127", time.time() - t0)


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_plans_from_grids(kind):
    """Both sources -- the packed records of a source batch with src_rows out of range on both sides (clamped: include/snac_hip.h), and
    environment_memory doubles in -3 .. 40000 -- and the three total_brick forms: the caller's, the source header's, neither (with
    environment_memory the entry point refuses that, and writes nothing).  Reference: numpy -- the interior clipped to 0 .. 32767 (2D: the
    board's bits, a cell > 0), total_brick clipped to 1 .. 32767."""
    import torch
    from snac_amd import _lib

    t0 = time.time()
    L = _lib.lib()
    env, src = _env(kind, 4), _env(kind, 6, seed=5, ticks=9)
    A = guard.Arena(_state_bytes(kind, 4) + 100 * (guard.BAND + 8192), env.device)
    saved = bind(env, A)
    rng = np.random.default_rng(10 + kind)
    sgrid, shdr = src._grid.cpu().numpy(), src._hdr.cpu().numpy().view(np.int16).reshape(6, 8)
    assert sgrid.any(), "the source batch has built something"
    src_rows_all = np.int32([-7, 2, 99, 0, 5])
    tb_all = np.int32([0, 17, 40000, -5, 32767])
    for first in FIRSTS:
        for m in COUNTS:
            # -- the packed records of a source batch
            for own_tb in (True, False):
                restore(env, saved)
                sr = A.carve((m,), torch.int32, name="src_rows (input)").copy_(torch.from_numpy(src_rows_all[:m]))
                tb = A.carve((m,), torch.int32, name="total_brick (input)").copy_(torch.from_numpy(tb_all[:m])) if own_tb else None
                _lib.check(L.snac_plans_from_grids(C.byref(env._desc), C.byref(env._state), m, first, C.byref(src._state), 6, C.c_void_p(sr.data_ptr()),
                                                   None, None if tb is None else C.c_void_p(tb.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
                pick = np.clip(src_rows_all[:m], 0, 5)
                g = sgrid[pick]
                if kind == 2:
                    rows = (g.view(np.uint32) & 0xFFFFF).astype(np.uint32)
                else:
                    rows = np.clip(g, 0, 32767).astype(np.int16)
                    if kind == 1:
                        rows[:, 30:] = 0
                want_tb = np.clip(tb_all[:m] if own_tb else shdr[pick, 4].astype(np.int64), 1, 32767).astype(np.int16)
                what = "plans_from_grids %dD src first %d m %d total_brick %s" % (kind, first, m, "given" if own_tb else "of the header")
                _same(env._plans[first:first + m], rows, what + ": plan rows")
                _same(env._plan_tb[first:first + m], want_tb, what + ": plan_tb")
                _same(sr, src_rows_all[:m], what + ": src_rows is an input")
                _unchanged_outside(env, saved, ("_plans", "_plan_tb"), range(first, first + m), what)
                A.check()
            # -- environment_memory
            shape = (m, 34) if kind == 1 else (m, 26, 26)
            mem = rng.integers(-3, 8, shape).astype(np.float64)
            hot = rng.random(shape) < 0.05
            mem[hot] = rng.choice(np.float64([-3, 32766, 32767, 32768, 40000]), int(hot.sum()))
            mem[(slice(None), 5) if kind == 1 else (slice(None), 5, 7)] = 40000.0          # an interior cell above the clamp
            inner = mem[:, 2:32] if kind == 1 else mem[:, 3:23, 3:23]
            if kind == 2:
                rows = ((inner > 0).astype(np.uint64) << np.arange(20, dtype=np.uint64)[None, None, :]).sum(2).astype(np.uint32)
            else:
                rows = np.zeros((m, 32 if kind == 1 else 400), np.int16)
                rows[:, :inner[0].size] = np.clip(inner, 0, 32767).reshape(m, -1)
            dmem = A.carve(shape, torch.float64, name="environment_memory (input)").copy_(torch.from_numpy(mem))
            for own_tb in (True, False):
                restore(env, saved)
                tb = A.carve((m,), torch.int32, name="total_brick (input)").copy_(torch.from_numpy(tb_all[:m])) if own_tb else None
                rc = L.snac_plans_from_grids(C.byref(env._desc), C.byref(env._state), m, first, None, 0, None, C.c_void_p(dmem.data_ptr()),
                                             None if tb is None else C.c_void_p(tb.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
                what = "plans_from_grids %dD environment_memory first %d m %d" % (kind, first, m)
                if own_tb:
                    _lib.check(rc)
                    _same(env._plans[first:first + m], rows, what + ": plan rows")
                    _same(env._plan_tb[first:first + m], np.clip(tb_all[:m], 1, 32767).astype(np.int16), what + ": plan_tb")
                    _unchanged_outside(env, saved, ("_plans", "_plan_tb"), range(first, first + m), what)
                else:                                                  # neither total_brick: refused before any launch
                    assert rc != _lib.SNAC_OK
                    _same(env._plans, saved["_plans"], what + ": nothing written"), _same(env._plan_tb, saved["_plan_tb"], what + ": nothing written")
                _same(dmem, mem, what + ": environment_memory is an input")
                A.check()
    for name in ("_hdr", "_episode", "_grid", "_stats"):
        _same(getattr(env, name), saved[name], name)
    _note("snac_plans_from_grids %dD" % kind, COUNTS, "first 0 3; src_rows -7 99; memory -3 .. 40000", time.time() - t0)


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_import_state(kind):
    """Scattered dst_index.  Reference: a twin env's import_states() into plain tensors."""
    import torch

    t0 = time.time()
    n = 12
    env, twin = _env(kind, n), _env(kind, n)
    A = guard.Arena(_state_bytes(kind, n) + 8 * (guard.BAND + 1024), env.device)
    saved = bind(env, A)
    tsaved = snapshot(twin)
    for name in STATE:
        _same(saved[name], tsaved[name], "the twin starts as the env")
    rng = np.random.default_rng(20 + kind)
    lo, hi = (2, 31) if kind == 1 else (3, 22)
    for m in COUNTS:
        for with_plan in (True, False):
            restore(env, saved), restore(twin, tsaved)
            dst = rng.permutation(n)[:m].astype(np.int64)
            shape = (m, 34) if kind == 1 else (m, 26, 26)
            mem = rng.integers(-1, 7, shape).astype(np.float64)
            mem[(slice(None), 6) if kind == 1 else (slice(None), 6, 9)] = 40000.0          # an interior cell above the clamp
            pos = rng.integers(lo, hi + 1, (m,) if kind == 1 else (m, 2))
            cb, cs = rng.integers(0, 40, m), rng.integers(0, 12, m)
            kw = dict(plan_idx=rng.integers(0, TABLE_ROWS, m), total_brick=rng.integers(1, 300, m)) if with_plan else {}
            for e in (env, twin):
                e.import_states(pos, cb, cs, mem, dst=torch.from_numpy(dst), **kw)
            what = "import_state %dD m %d%s" % (kind, m, " with plan_idx and total_brick" if with_plan else "")
            for name in STATE:
                _same(getattr(env, name), getattr(twin, name), what + ": " + name)
            _unchanged_outside(env, saved, ("_hdr", "_episode", "_grid"), dst, what)
            assert not torch.equal(env._grid, saved["_grid"]), what + ": something was imported"
            A.check()
    _note("snac_import_state %dD" % kind, COUNTS, "scattered dst_index among 12 rows", time.time() - t0)


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_pack_and_unpack(kind):
    """snac_nodes*_pack into a pool carved 128 bytes past a 512-byte boundary, snac_nodes*_unpack into the arena-bound state.  Reference: a
    twin pool / twin env in plain tensors taking the same calls."""
    import torch
    from snac_amd import NodePool

    t0 = time.time()
    n = 132
    env, twin = _env(kind, n, rows=16, ticks=9), _env(kind, n, rows=16, ticks=9)
    rows = 2 * n
    pool, tpool = NodePool(env, rows), NodePool(twin, rows)
    A = guard.Arena(_state_bytes(kind, n) + 16 * 404 * 4 + rows * pool.WORDS * 4 + 10 * (guard.BAND + 1024), env.device)
    saved = bind(env, A)
    tsaved = snapshot(twin)
    tpool.load(rows=torch.arange(rows) % n, node_rows=torch.arange(rows).flip(0))      # every record holds a state
    master = tpool.records.clone()
    pool.records = A.carve((rows, pool.WORDS), torch.int32, offset=128, name="node records").copy_(master)
    assert pool.records.data_ptr() % 512 == 128
    rng = np.random.default_rng(30 + kind)
    for m in EDGES:
        what = "%dD m %d" % (kind, m)
        # pack: env rows (several i may name one) -> distinct records
        pool.records.copy_(master), tpool.records.copy_(master)
        restore(env, saved), restore(twin, tsaved)
        src, dst =rng.integers(0, n, m), rng.permutation(rows)[:m]
        for p in (pool, tpool):
            p.load(rows=torch.from_numpy(src), node_rows=torch.from_numpy(dst))
        assert torch.equal(pool.records, tpool.records), "pack " + what
        keep = torch.ones(rows, dtype=torch.bool, device=env.device)
        keep[torch.from_numpy(dst).to(env.device)] = False
        assert torch.equal(pool.records[keep], master[keep]), "pack %s: records outside node_rows" % what
        assert not torch.equal(pool.records, master)
        for name in STATE:
            _same(getattr(env, name), saved[name], "pack %s: %s is an input" % (what, name[1:]))
        A.check()
        # unpack: records -> distinct env rows
        pool.records.copy_(master), tpool.records.copy_(master)
        restore(env, saved), restore(twin, tsaved)
        nodes, erows = rng.integers(0, rows, m), rng.permutation(n)[:m]
        pool.store(node_rows=torch.from_numpy(nodes), rows=torch.from_numpy(erows))
        tpool.store(node_rows=torch.from_numpy(nodes), rows=torch.from_numpy(erows))
        for name in STATE:
            _same(getattr(env, name), getattr(twin, name), "unpack %s: %s" % (what, name[1:]))
        _unchanged_outside(env, saved, ("_hdr", "_episode", "_grid"), erows, "unpack " + what)
        assert torch.equal(pool.records, master), "unpack %s: the records are an input" % what
        A.check()
    _note("snac_nodes%dd_pack" % kind, EDGES, "records +128", 0)
    _note("snac_nodes%dd_unpack" % kind, EDGES, "hdr / episode / grid +0", time.time() - t0)
