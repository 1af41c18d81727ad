"""GPU: 1D and 3D node pools with one record per node (snac_nodes{1,3}d_pack / _unpack, snac_transition_nodes{1,3}d, snac_amd.NodePool1D /
NodePool3D / NodePool) against the batch-layout path (snac_transition on a BatchedDMPEnv pool -- itself oracle-checked in
tests/test_gpu_mcts.py) AND against the CPU oracle directly: search-shaped waves on all three, every wave's rows, rewards and done flags
equal to the byte, the states equal afterwards.  The head / tail seam of a wave is pinned for all three kinds (2D included)."""
import ctypes as C

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

KINDS = [(1, False), (1, True), (3, False), (3, True)]
GRID_BYTES = {1: 64, 2: 80, 3: 800}
GRID_WORDS = {1: (8, 24), 2: (8, 28), 3: (8, 208)}                  # the cells' int32 words in a record


def _tag(kind, dyn):
    return ("sin_train" if kind == 1 else "dense_train") if dyn else ("p1" if kind == 3 else "p0")


def _pools(kind, dyn, pool, seed, dtype=None, oracle=True):
    import torch
    from snac_amd import BatchedDMPEnv, NodePool

    table = helpers.plan_table(kind, dyn, _tag(kind, dyn))
    full = table.reshape((-1, 30) if kind == 1 else (-1, 26, 26))
    kw = {"obs_dtype": dtype} if dtype is not None else {}
    env = BatchedDMPEnv(kind, dyn, pool, plans=full, seed=seed, **kw)
    twin = BatchedDMPEnv(kind, dyn, pool, plans=full, seed=seed, **kw)
    env.reset(); twin.reset()
    env.rollout(37, obs=None); twin.rollout(37, obs=None)
    orc = None
    if oracle:
        orc = helpers.oracle().OracleBatch(kind, dyn, pool, table, seed=seed)
        orc.reset()
        orc.rollout(37, obs=None)
    nodes = NodePool(env, pool)
    assert nodes.load() == pool
    return env, twin, orc, nodes, torch


def _same_records(nodes, twin, rows=None):
    import torch

    kind = twin.kind
    rows = torch.arange(twin.num_envs, device=twin.device) if rows is None else torch.as_tensor(rows, device=twin.device)
    r = nodes.records[rows]
    lo, hi = GRID_WORDS[kind]
    assert torch.equal(r[:, :4].contiguous().view(torch.uint8), twin._hdr[rows].contiguous().view(torch.uint8).reshape(len(rows), 16))
    assert torch.equal(r[:, 4], twin._episode[rows].to(torch.int32))
    assert torch.equal(r[:, lo:hi].contiguous().view(torch.uint8), twin._grid[rows].contiguous().view(torch.uint8).reshape(len(rows), GRID_BYTES[kind]))
    assert int(r[:, 5:8].abs().sum()) == 0 and int(r[:, hi:].abs().sum()) == 0


@pytest.mark.parametrize("kind,dyn", KINDS)
def test_pack_unpack_round_trip_and_decoded_fields(kind, dyn):
    env, twin, orc, nodes, torch = _pools(kind, dyn, 1000, 5, oracle=False)
    from snac_amd import NodePool1D, NodePool3D

    assert type(nodes) is (NodePool1D if kind == 1 else NodePool3D)
    assert nodes.records.shape == (1000, 32 if kind == 1 else 224)
    _same_records(nodes, env)
    assert torch.equal(nodes.position, env.position.to(nodes.position.dtype)) and torch.equal(nodes.count_brick, env.count_brick.to(torch.int32))
    assert torch.equal(nodes.count_step, env.count_step.to(torch.int32)) and torch.equal(nodes.plan_idx, env.plan_idx.to(torch.int32))
    assert torch.equal(nodes.total_brick, env.total_brick.to(torch.int32)) and torch.equal(nodes.need_reset, env.need_reset)
    if kind == 1:
        assert nodes.heights.shape == (1000, 30) and torch.equal(nodes.heights, env._grid[:, :30])
    else:
        assert nodes.heights.shape == (1000, 20, 20) and torch.equal(nodes.heights, env._grid.view(1000, 20, 20))
    assert int(nodes.heights.abs().sum()) > 0                        # the rollout built something
    # gathered rows both ways
    rng = np.random.default_rng(1)
    rows = rng.permutation(1000)[:300].astype(np.int32)
    nrows = rng.permutation(1000)[:300].astype(np.int32)
    nodes.load(rows=rows, node_rows=nrows)
    rt, nt = torch.as_tensor(rows.astype(np.int64), device=env.device), torch.as_tensor(nrows.astype(np.int64), device=env.device)
    assert torch.equal(nodes.heights[nt], (env._grid[:, :30] if kind == 1 else env._grid.view(1000, 20, 20))[rt])
    back = type(env)(kind, dyn, 1000, plans=env.plans_full, seed=42)
    back.reset()
    nodes.store(node_rows=nrows, rows=rows, env=back)
    assert torch.equal(back._hdr[rt], env._hdr[rt]) and torch.equal(back._grid[rt], env._grid[rt]) and torch.equal(back._episode[rt], env._episode[rt])
    # across two envs: the records of one batch unpacked into another
    other = type(env)(kind, dyn, 1000, plans=env.plans_full, seed=99)
    other.reset()
    nodes.load()                                                     # records = env's rows again
    nodes.store(env=other)
    assert torch.equal(other._hdr, env._hdr) and torch.equal(other._grid, env._grid) and torch.equal(other._episode, env._episode)
    assert torch.equal(other.observe(), env.observe())


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("kind,dyn", KINDS)
def test_edges_on_node_records_equal_the_batch_pool_and_the_oracle(kind, dyn, f32):
    import torch
    from test_gpu_mcts import same_state

    pool, roots = 6000, 500
    env, twin, orc, nodes, torch = _pools(kind, dyn, pool, 11, torch.float32 if f32 else None)
    rng = np.random.default_rng(7 + kind)
    A, used = env.num_actions, roots
    cast = (lambda x: x.astype(np.float32)) if f32 else (lambda x: x)
    for wave, m in enumerate([256, 64, 999, 4, 3, 130, 1, 777, 2050, 510]):    # m % 4 = 0, 1, 2, 3: runs and rows value by value
        if wave % 3 == 2:                                                   # in place on distinct rows
            m = min(m, used)
            src = rng.permutation(used)[:m].astype(np.int32)
            dst = src.copy()
            acts = rng.integers(0, A, m).astype(np.int8)
        else:                                                               # random parents x all actions into fresh records
            parents = rng.integers(0, used, (m + A - 1) // A)
            src = np.repeat(parents, A)[:m].astype(np.int32)
            acts = np.tile(np.arange(A), len(parents))[:m].astype(np.int8)
            dst = (used + np.arange(m)).astype(np.int32)
            used += m
        ks = rng.integers(1, 4, m).astype(np.int8) if wave % 2 == 0 else None   # None: the counter RNG keyed by (edge, t)
        o1, r1, d1 = nodes.transition(acts, ks, src=src, dst=dst, t=wave)
        assert env._lib.snac_last_kernel() == (b"k_edges1dp" if kind == 1 else b"k_edges3dp")
        o2, r2, d2 = twin.transition(torch.from_numpy(acts), None if ks is None else torch.from_numpy(ks), src=src, dst=dst, t=wave)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2), (wave, m)
        oo, ro, do = orc.transition(acts, ks, src=src, dst=dst, t=wave)
        assert o1.cpu().numpy().tobytes() == cast(oo).tobytes() and r1.cpu().numpy().tobytes() == ro.tobytes(), (wave, m)
        assert np.array_equal(d1.cpu().numpy().astype(np.uint8), do), (wave, m)
        _same_records(nodes, twin, np.unique(dst).astype(np.int64))
    assert used <= pool
    _same_records(nodes, twin)
    # back into a batch: the unpacked rows are the oracle's states; observe works on them
    nodes.store()
    same_state(env, orc)
    assert torch.equal(env._hdr, twin._hdr) and torch.equal(env._grid, twin._grid) and torch.equal(env.observe(), twin.observe())


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_head_and_tail_launches_of_a_wave_equal_the_batch_pool(kind, dyn, f32):
    """The seam between the head of a wave (m & ~3 edges, rows as 16-byte pieces) and its tail (the last one to three, value by value, a
    launch of its own) for all three kinds: an empty head (3), an exact head (4), a head with a tail (7), a tail in the second wave
    (67) and in the third (131) of the one block.  step_size=None: the step size comes from the counter RNG, keyed by the edge's index
    in the CALL, so a tail launch that forgot its offset would draw other sizes.  The batch-row kernels are the reference: rows,
    rewards, done flags and the written records equal to the byte."""
    import torch

    pool, used = 320, 100
    env, twin, orc, nodes, torch = _pools(kind, dyn, pool, 17, torch.float32 if f32 else None, oracle=False)
    rng = np.random.default_rng(40 + kind)
    for t, m in enumerate((3, 4, 7, 67, 131), start=5):
        src = rng.integers(0, used, m).astype(np.int32)
        dst = (used + np.arange(m)).astype(np.int32)
        acts = rng.integers(0, env.num_actions, m).astype(np.int8)
        o1, r1, d1 = nodes.transition(acts, None, src=src, dst=dst, t=t)
        assert env._lib.snac_last_kernel() == b"k_edges%ddp" % kind
        o2, r2, d2 = twin.transition(torch.from_numpy(acts), None, src=src, dst=dst, t=t)
        assert o1.dtype == o2.dtype and torch.equal(o1.contiguous().view(torch.uint8), o2.contiguous().view(torch.uint8)), (t, m)
        assert torch.equal(r1, r2) and torch.equal(d1, d2), (t, m)
        _same_records(nodes, twin, dst.astype(np.int64))
        used += m
    assert used <= pool
    _same_records(nodes, twin)


@pytest.mark.parametrize("kind,dyn", KINDS)
def test_identity_in_place_unaligned_rows_and_limit_states(kind, dyn):
    import torch

    n = 512
    env, twin, orc, nodes, torch = _pools(kind, dyn, n, 3, oracle=False)
    A = env.num_actions
    g = torch.Generator(device="cuda").manual_seed(kind * 10 + dyn)
    acts = torch.randint(0, A, (n,), dtype=torch.int8, device="cuda", generator=g)
    ks = torch.randint(1, 4, (n,), dtype=torch.int8, device="cuda", generator=g)
    o1, r1, d1 = nodes.transition(acts, ks)                          # identity rows
    o2, r2, d2 = twin.transition(acts, ks)
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    _same_records(nodes, twin)
    rows = torch.randperm(n, device="cuda", generator=g)[:257].to(torch.int32)   # in place, a ragged count
    o1, r1, d1 = nodes.transition(acts[:257], None, src=rows, dst=rows, t=4)
    o2, r2, d2 = twin.transition(acts[:257], None, src=rows, dst=rows, t=4)
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    _same_records(nodes, twin)
    # an observation buffer that is not 16-byte aligned: rows value by value (raw call: the wrapper allocates aligned rows)
    L, D = env._lib, env.obs_dim
    raw = torch.zeros(n * D + 1, dtype=torch.float64, device="cuda")
    ob = raw[1:].view(n, D)
    rw, dn = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    entry = L.snac_transition_nodes1d if kind == 1 else L.snac_transition_nodes3d
    from snac_amd import _lib

    _lib.check(entry(C.byref(env._desc), C.byref(env._state), vp(nodes.records), n, n, None, None, 9, vp(acts), vp(ks), vp(ob), vp(rw), vp(dn),
                     env._stream()))
    o2, r2, d2 = twin.transition(acts, ks, t=9)
    assert ob.data_ptr() % 16 != 0 and torch.equal(ob, o2) and torch.equal(rw, r2) and torch.equal(dn.view(torch.bool), d2)
    _same_records(nodes, twin)
    # states at the time limit, at the brick limit and (3D) boxed in by bricks: done, and the -100 of the dynamic 3D rules
    m = 192
    sel = torch.arange(m, device="cuda")
    mem = twin.environment_memory()[sel]
    cs = twin.count_step[sel].to(torch.int32).clone()
    cb = twin.count_brick[sel].to(torch.int32).clone()
    tb = twin.total_brick[sel].to(torch.int32)
    cs[:64] = env.total_step - 1
    cb[64:128] = torch.clamp(tb[64:128] - 1, min=0)
    if kind == 3:
        inner = mem[128:, 3:23, 3:23]
        mem[128:, 3:23, 3:23] = torch.where(inner > 0, inner, torch.ones_like(inner))   # every interior cell built
    pos = twin.position[sel]
    pos = pos[:, 0] if kind == 1 else pos
    for e in (env, twin):
        e.import_states(pos, cb, cs, mem, plan_idx=twin.plan_idx[sel], dst=sel.to(torch.int32))
    dst = (256 + sel).to(torch.int32)
    nodes.load(rows=sel.to(torch.int32), node_rows=sel.to(torch.int32))
    build = torch.full((m,), 2 if kind == 1 else 4, dtype=torch.int8, device="cuda")
    if kind == 3:
        build += torch.randint(0, 4, (m,), dtype=torch.int8, device="cuda", generator=g)
    build[:32] = 0                                                   # a move at the time limit
    o1, r1, d1 = nodes.transition(build, None, src=sel.to(torch.int32), dst=dst, t=11)
    o2, r2, d2 = twin.transition(build, None, src=sel.to(torch.int32), dst=dst, t=11)
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    assert bool(d1[:32].all()) and bool(d1[32:128].any())             # (a successful 3D build does not test the time limit)
    if kind == 3 and dyn:
        assert bool((r1[128:] == -100).any())
    _same_records(nodes, twin, dst.to(torch.int64))


def test_python_errors_and_the_pool_of_each_kind():
    import torch
    from snac_amd import BatchedDMPEnv, NodePool, NodePool1D, NodePool2D, NodePool3D

    envs = {k: BatchedDMPEnv(k, True, 8, seed=1) for k in (1, 2, 3)}
    for e in envs.values():
        e.reset()
    for cls, k in ((NodePool1D, 1), (NodePool2D, 2), (NodePool3D, 3)):
        assert type(NodePool(envs[k], 16)) is cls
        for other in (1, 2, 3):
            if other != k:
                with pytest.raises(ValueError):
                    cls(envs[other], 16)
    for k in (1, 3):
        nodes = NodePool(envs[k], 16)
        nodes.load()
        acts = torch.zeros(4, dtype=torch.int8, device="cuda")
        with pytest.raises(ValueError):
            nodes.transition(acts, None, src=[0, 1, 2, 3], dst=[1, 9, 10, 11])   # record 1 is read by another edge
        with pytest.raises(ValueError):
            nodes.transition(acts, None, src=[0, 1, 2, 3], dst=[9, 9, 10, 11])
        with pytest.raises(ValueError):
            nodes.transition(acts, None, src=[0, 1, 2, 16], dst=[9, 8, 10, 11])
        with pytest.raises(ValueError):
            nodes.load(rows=[0, 8], node_rows=[0, 1])
        with pytest.raises(ValueError):
            nodes.store(node_rows=[0, 16], rows=[0, 1])


@pytest.mark.parametrize("kind,pool,m", [(1, 1 << 20, 524288), (3, 1 << 18, 131072)])
def test_full_size_wave_equals_the_batch_pool(kind, pool, m):
    """A full-size wave of random-parent edges into fresh records against the same wave on the batch pool (k_edges1d / k_edges3d,
    oracle-checked at small sizes): every row, reward, done flag and resulting record equal; then a second wave in place."""
    import torch
    from snac_amd import BatchedDMPEnv, NodePool

    env = BatchedDMPEnv(kind, True, pool, seed=1)
    env.reset()
    env.rollout(20, obs=None)
    twin = env.fork(torch.arange(pool, device=env.device))
    nodes = NodePool(env, pool)
    assert nodes.load() == pool
    g = torch.Generator(device="cuda").manual_seed(3)
    src = torch.randint(0, pool - m, (m,), device="cuda", dtype=torch.int32, generator=g)
    dst = (pool - m + torch.arange(m, device="cuda", dtype=torch.int32)).contiguous()
    acts = torch.randint(0, env.num_actions, (m,), device="cuda", generator=g).to(torch.int8)
    ks = torch.randint(1, 4, (m,), device="cuda", generator=g).to(torch.int8)
    o1, r1, d1 = nodes.transition(acts, ks, src=src, dst=dst, check=False)
    assert env._lib.snac_last_kernel() == (b"k_edges1dp" if kind == 1 else b"k_edges3dp")
    o2, r2, d2 = twin.transition(acts, ks, src=src, dst=dst)
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    _same_records(nodes, twin, dst.to(torch.int64))
    o1, r1, d1 = nodes.transition(acts, None, src=dst, dst=dst, t=7, check=False)
    o2, r2, d2 = twin.transition(acts, None, src=dst, dst=dst, t=7)
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    other = BatchedDMPEnv(kind, True, pool, seed=2)
    other.reset()
    assert nodes.store(env=other) == pool
    assert torch.equal(other._hdr, twin._hdr) and torch.equal(other._grid, twin._grid) and torch.equal(other._episode, twin._episode)
