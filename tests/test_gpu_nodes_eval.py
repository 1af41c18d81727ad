"""GPU: default-policy evaluation of tree leaves in place on node pools (snac_evaluate_nodes{1,2,3}d, NodePool*.evaluate) against
BatchedDMPEnv.evaluate on the same states (fork + rollout + snac_discounted_return, itself oracle-checked in tests/test_gpu_mcts.py) --
estimates equal to the byte, step counts exactly -- and against a restatement of script/MCTS/utils/mcts.py:100-110 on the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

from devmem import _tag
import helpers

pytestmark = pytest.mark.gpu

KINDS = [(1, False), (1, True), (2, False), (2, True), (3, False), (3, True)]
T0 = {1: 37, 2: 600, 3: 21}                                         # pre-rollout: some rows end on a terminal step (as test_gpu_mcts.py)
H = {1: 300, 2: 700, 3: 400}                                        # horizons long enough for most leaves to end, not all


def _env(kind, dyn, n, seed, **kw):
    from snac_amd import BatchedDMPEnv

    table = helpers.plan_table(kind, dyn, _tag(kind, dyn))
    full = table.reshape((-1, 30) if kind == 1 else (-1, 26, 26))
    env = BatchedDMPEnv(kind, dyn, n, plans=full, seed=seed, **kw)
    env.reset()
    env.rollout(T0[kind], obs=None)
    return env, table


def _pool(env, rows, seed):
    """A pool of `rows` records holding the env's rows at permuted records; returns (pool, perm: record of env row r)."""
    import torch
    from snac_amd import NodePool

    pool = NodePool(env, rows)
    g = torch.Generator(device="cpu").manual_seed(seed)
    perm = torch.randperm(rows, generator=g)[:env.num_envs].to(env.device)
    assert pool.load(rows=torch.arange(env.num_envs, device=env.device), node_rows=perm) == env.num_envs
    return pool, perm


def _state(env):
    return [t.clone() for t in (env._hdr, env._episode, env._grid, env._stats, env._plans, env._plan_tb)]


def _same_state(env, before):
    import torch

    for a, b in zip(_state(env), before):
        assert torch.equal(a, b)


def _bytes_equal(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("kind,dyn", KINDS)
def test_pool_evaluation_equals_the_batch_path_bit_for_bit(kind, dyn):
    import torch

    n, m = 600, 700
    env, _ = _env(kind, dyn, n, 11 + kind)
    env._hdr.view(torch.int8)[::17, 2] |= 1                             # (SNAC_FLAG_NEED_RESET) a few more terminal rows, whatever the pre-rollout left
    pool, perm = _pool(env, 2048, kind)
    rng = np.random.default_rng(kind * 2 + dyn)
    rows = torch.as_tensor(rng.integers(0, n, m), device=env.device)      # leaves repeat
    first = torch.as_tensor(rng.integers(-1, 11, m).astype(np.float64), device=env.device)
    records, before = pool.records.clone(), _state(env)
    est, steps = pool.evaluate(perm[rows], H[kind], 0.97, first_reward=first)
    assert torch.equal(pool.records, records)
    _same_state(env, before)
    ref, ref_steps = env.evaluate(rows, H[kind], 0.97, first_reward=first)
    assert est.dtype == torch.float64 and steps.dtype == torch.int64 and est.shape == (m,) and steps.shape == (m,)
    assert _bytes_equal(est, ref) and torch.equal(steps, ref_steps)
    term = env.need_reset[rows]
    assert bool((steps[term] == 0).all()) and _bytes_equal(est[term], first[term])
    assert int(term.sum()) > 0 and int((steps == H[kind]).sum()) < m and int(steps.max()) > 1   # terminal leaves, leaves that end


@pytest.mark.parametrize("kind,dyn", [(1, True), (2, True), (3, False), (3, True)])
def test_pool_evaluation_matches_the_reference_loop_on_the_oracle(kind, dyn):
    """script/MCTS/utils/mcts.py:100-110 restated on the oracle: tick t of leaf i is keyed by (env_id_base + i, t0 + t)."""
    import rng_spec
    import torch
    from snac_amd import BatchedDMPEnv, NodePool

    n, m, seed, base, t0, gamma = 300, 120, 7, 1000, 12345, 0.9
    Hk = {1: 80, 2: 90, 3: 60}[kind]
    table = helpers.plan_table(kind, dyn, _tag(kind, dyn))
    full = table.reshape((-1, 30) if kind == 1 else (-1, 26, 26))
    env = BatchedDMPEnv(kind, dyn, n, plans=full, seed=seed, env_id_base=base)
    orc_mod = helpers.oracle()
    orc = orc_mod.OracleBatch(kind, dyn, n, table, seed=seed, env_id_base=base)
    env.reset(); orc.reset()
    env.rollout(T0[kind], obs=None); orc.rollout(T0[kind], obs=None)
    pool = NodePool(env, 512)
    pool.load(rows=torch.arange(n, device=env.device), node_rows=torch.arange(n, device=env.device) + 100)
    rng = np.random.default_rng(kind)
    rows = rng.integers(0, n, m)
    first = rng.integers(-1, 11, m).astype(np.float64)
    est, steps = pool.evaluate(torch.as_tensor(rows + 100, device=env.device), Hk, gamma, first_reward=first, t0=t0)
    st = orc.state()
    A = env.num_actions
    for i, row in enumerate(rows):
        e = orc_mod.OracleEnv(kind, dyn)
        e.reset(table[st["plan_idx"][row]].reshape(-1), int(st["plan_idx"][row]))
        pos = st["pos"][row]
        e.set_state(st["grid"][row], int(pos[0]) if kind == 1 else pos, st["cb"][row], st["cs"][row])
        estimate, terminal, t = float(first[i]), bool(st["need_reset"][row]), 0
        while (not terminal) and t < Hk:
            w = rng_spec.words(seed, 0, np.uint64(base + i), np.uint64(t0 + t))
            a, k = int(rng_spec.action_of(w, A)), int(rng_spec.step_size_of(w))
            _, _, r, terminal = e.transition(a, k, inplace=True)
            estimate += r * (gamma ** t)
            t += 1
        assert np.float64(est[i].item()).tobytes() == np.float64(estimate).tobytes(), (kind, dyn, i)
        assert int(steps[i]) == t, (kind, dyn, i)


@pytest.mark.parametrize("kind,dyn", [(1, False), (2, True), (3, True)])
def test_pool_evaluation_with_rule_flags_and_a_time_limit(kind, dyn):
    import torch

    n, m = 400, 400
    env, _ = _env(kind, dyn, n, 3, time_gt=True, brick_gt=True, total_step={1: 90, 2: 120, 3: 80}[kind])
    pool, perm = _pool(env, 1024, 9)
    rows = torch.as_tensor(np.random.default_rng(5).integers(0, n, m), device=env.device)
    est, steps = pool.evaluate(perm[rows], 200, 0.95, first_reward=torch.ones(m, dtype=torch.float64, device=env.device))
    ref, ref_steps = env.evaluate(rows, 200, 0.95, first_reward=torch.ones(m, dtype=torch.float64, device=env.device))
    assert _bytes_equal(est, ref) and torch.equal(steps, ref_steps)


@pytest.mark.parametrize("kind,dyn", [(1, True), (2, False), (3, True)])
def test_pool_evaluation_edges(kind, dyn):
    import torch
    from snac_amd import _lib

    n = 256
    env, _ = _env(kind, dyn, n, 21)
    pool, perm = _pool(env, 512, 4)
    rows = torch.arange(n, device=env.device)
    first = torch.linspace(-3, 7, n, dtype=torch.float64, device=env.device)
    for h in (0, 1, 3):                                                    # H = 0 and 1, and 3: leaves that do not end within H
        est, steps = pool.evaluate(perm, h, 0.9, first_reward=first)
        ref, ref_steps = env.evaluate(rows, h, 0.9, first_reward=first)
        assert _bytes_equal(est, ref) and torch.equal(steps, ref_steps), h
    assert bool((steps[env.need_reset] == 0).all()) and int(steps.max()) == 3
    # H = 0 through the C entry point: est stays, steps are written as zero
    est, steps = first.clone(), torch.full((n,), -1, dtype=torch.int64, device=env.device)
    gp = torch.ones(1, dtype=torch.float64, device=env.device)
    _lib.check(getattr(env._lib, pool.EVALUATE)(C.byref(env._desc), C.byref(env._state), C.c_void_p(pool.records.data_ptr()), pool.rows, n,
                                                 C.c_void_p(perm.to(torch.int32).contiguous().data_ptr()), 0, 0, C.c_void_p(gp.data_ptr()),
                                                 C.c_void_p(est.data_ptr()), C.c_void_p(steps.data_ptr()), env._stream()))
    torch.cuda.synchronize()
    assert _bytes_equal(est, first) and int(steps.abs().sum()) == 0
    # first_reward None, node_rows None (records 0 .. m - 1), check=False
    from snac_amd import NodePool

    idn = NodePool(env, n)
    assert idn.load() == n                                                 # record i <- row i
    est, steps = idn.evaluate(None, 50, 0.99)
    ref, ref_steps = env.evaluate(rows, 50, 0.99)
    assert est.shape == (n,) and _bytes_equal(est, ref) and torch.equal(steps, ref_steps)
    est2, steps2 = pool.evaluate(perm, 50, 0.99, check=False)
    assert _bytes_equal(est2, ref) and torch.equal(steps2, ref_steps)
    # every leaf terminal: nothing rolls out
    pool.records[:, 0] |= _lib.FLAG_NEED_RESET << 16
    est, steps = pool.evaluate(perm, 50, 0.99, first_reward=first)
    assert _bytes_equal(est, first) and int(steps.abs().sum()) == 0
    # the Python errors: shape, range, a pool of another kind
    with pytest.raises(ValueError):
        pool.evaluate(perm, 10, 0.9, first_reward=first[:-1])
    with pytest.raises(ValueError):
        pool.evaluate(perm.reshape(2, -1)[:, :3], 10, 0.9, first_reward=first)
    with pytest.raises(ValueError):
        pool.evaluate(torch.tensor([0, pool.rows], device=env.device), 10, 0.9)
    with pytest.raises(ValueError):
        pool.evaluate(torch.tensor([-1, 0], device=env.device), 10, 0.9)
    from snac_amd import NodePool1D, NodePool2D, NodePool3D
    other = {1: NodePool2D, 2: NodePool3D, 3: NodePool1D}[kind]
    with pytest.raises(ValueError):
        other(env, 64)
    e0, s0 = pool.evaluate(torch.zeros(0, dtype=torch.int64, device=env.device), 10, 0.9)
    assert e0.shape == (0,) and s0.shape == (0,)


def test_pool_evaluation_float32_env():
    import torch

    env, _ = _env(2, True, 300, 8, obs_dtype=torch.float32)
    pool, perm = _pool(env, 1024, 2)
    rows = torch.arange(300, device=env.device).flip(0)
    est, steps = pool.evaluate(perm[rows], 300, 0.99)
    ref, ref_steps = env.evaluate(rows, 300, 0.99)
    assert _bytes_equal(est, ref) and torch.equal(steps, ref_steps)


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_pool_evaluation_ragged_wave_on_a_large_pool(kind):
    """m = 65 536 + 37 leaves (the last wave part-filled) on a 2^18-record pool."""
    import torch

    n, m = 4096, 65536 + 37
    env, _ = _env(kind, True, n, 17)
    pool, perm = _pool(env, 1 << 18, 6)
    rows = torch.as_tensor(np.random.default_rng(1).integers(0, n, m), device=env.device)
    first = torch.as_tensor(np.random.default_rng(2).random(m), device=env.device)
    Hk = {1: 120, 2: 150, 3: 60}[kind]
    records = pool.records.clone()
    est, steps = pool.evaluate(perm[rows], Hk, 0.98, first_reward=first)
    ref, ref_steps = env.evaluate(rows, Hk, 0.98, first_reward=first)
    assert _bytes_equal(est, ref) and torch.equal(steps, ref_steps)
    assert torch.equal(pool.records, records)
