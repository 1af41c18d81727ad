"""GPU: the observation rows of node records (pool.observe(); snac_observe_nodes1d / 2d / 3d, k_nodes_obs.hip) against their definition:
row i = what env.observe() shows for a batch row after pool.store(node_rows=[x], rows=[r]) -- byte for byte, for every record, terminal
ones (SNAC_FLAG_NEED_RESET) included.  The records come from a few hundred random pool.transition edges; the pool is read only."""
import numpy as np
import pytest

from devmem import _tag
import helpers

pytestmark = pytest.mark.gpu

KINDS = [(1, False), (1, True), (2, False), (2, True), (3, False), (3, True)]


def _make(kind, dyn, n, f32, seed):
    import torch
    from snac_amd import BatchedDMPEnv

    table = helpers.plan_table(kind, dyn, _tag(kind, dyn))
    full = table.reshape((-1, 30) if kind == 1 else (-1, 26, 26))
    kw = {"obs_dtype": torch.float32} if f32 else {}
    env = BatchedDMPEnv(kind, dyn, n, plans=full, seed=seed, **kw)
    env.reset()
    return env


def _reference(pool, twin, rows):
    """store + env.observe(), in chunks of the twin batch's size."""
    import torch

    n, out = twin.num_envs, []
    for lo in range(0, len(rows), n):
        chunk = rows[lo:lo + n]
        pool.store(node_rows=chunk, rows=np.arange(len(chunk)), env=twin)
        out.append(twin.observe()[:len(chunk)].clone())
    return torch.cat(out)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("kind,dyn", KINDS)
def test_observed_records_equal_store_and_env_observe(kind, dyn, f32):
    import torch
    from snac_amd import NodePool, _lib

    n, R = 512, 1500
    env, twin = _make(kind, dyn, n, f32, 3 + kind), _make(kind, dyn, n, f32, 99)
    env.rollout(37, obs=None)
    ts = _lib.env_sizes(kind, dyn).total_step
    cs = env._hdr.view(torch.int16).view(n, 8)[:, 3]
    cs[0::3] = ts - 1                                                # their children come back done: terminal records
    cs[1::3] = ts - 2
    pool = NodePool(env, R)
    pool.load(rows=np.arange(R) % n, node_rows=np.arange(R))        # every record holds a state
    rng = np.random.default_rng(17 + kind + 2 * dyn)
    A, used = env.num_actions, n
    for wave, m in enumerate([200, 130, 77, 250, 3]):               # a few hundred random edges into fresh records
        src = rng.integers(0, used, m).astype(np.int32)
        dst = (used + np.arange(m)).astype(np.int32)
        pool.transition(rng.integers(0, A, m).astype(np.int8), src=src, dst=dst, t=wave, want_obs=False)
        used += m
    assert bool(pool.need_reset[:used].any()) and not bool(pool.need_reset[:used].all())
    before = pool.records.clone()
    term = np.nonzero(pool.need_reset.cpu().numpy())[0]
    for m in (777, 64, 193, 3, 1):                                   # m % 64 and m % 4 of every kind; shuffled rows with repeats
        rows = rng.integers(0, used, m).astype(np.int32)
        rows[:min(m, len(term))] = term[:min(m, len(term))]          # terminal records among them
        rng.shuffle(rows)
        got = pool.observe(rows)
        assert env._lib.snac_last_kernel() == b"k_observe%ddp" % kind
        assert got.dtype == env.obs_dtype and tuple(got.shape) == (m, env.obs_dim)
        want = _reference(pool, twin, rows)
        assert helpers.same_bytes(got.cpu().numpy(), want.cpu().numpy()), (kind, dyn, f32, m)
        again = torch.full_like(got, 7)
        assert pool.observe(torch.as_tensor(rows, device=env.device), out=again, check=False) is again
        assert torch.equal(again.view(torch.uint8), got.view(torch.uint8))
    every = pool.observe()                                           # node_rows=None: record i
    assert tuple(every.shape) == (R, env.obs_dim)
    assert helpers.same_bytes(every.cpu().numpy(), _reference(pool, twin, np.arange(R, dtype=np.int32)).cpu().numpy())
    head = torch.empty((R - 5, env.obs_dim), dtype=env.obs_dtype, device=env.device)
    pool.observe(out=head)                                           # m = out's rows, not a multiple of 4: the value-by-value tail
    assert torch.equal(head.view(torch.uint8), every[:R - 5].contiguous().view(torch.uint8))
    torch.cuda.synchronize()
    assert torch.equal(pool.records, before)                         # read only
    with pytest.raises(ValueError):
        pool.observe([R])
    with pytest.raises(ValueError):
        pool.observe([0, 1], out=head)
