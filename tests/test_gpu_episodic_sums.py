"""GPU: snac_episodic_sums -- the batch's three episodic sums in one launch (G <= 64 blocks, partials and a self-resetting ticket in a
scratch the batch owns), behind stats_tensor() and episodic_stats().  The per-env arrays are filled with seeded int64 values of both
signs up to 2^40, so a float path cannot pass; the sums must equal _stats.sum(dim=1) exactly.  Batch sizes: 1, 4, 63, 64, 65 (arrays
that start in the middle of a 16-byte piece when N is odd), 257, 4099 (five blocks, a ragged last slice)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 4, 63, 64, 65, 257, 4099]


def _batch(n, seed=1, **kw):
    from snac_amd import BatchedDMPEnv

    env = BatchedDMPEnv(2, True, n, seed=seed, **kw)
    env.reset()
    return env


def _fill(env, seed):
    import torch

    rng = np.random.default_rng(seed)
    v = rng.integers(-(1 << 40), (1 << 40) + 1, size=tuple(env._stats.shape), dtype=np.int64)
    env._stats.copy_(torch.from_numpy(v).to(env.device))
    return [int(x) for x in v.sum(axis=1)]                            # numpy int64 sums: exact (|sum| < 2^53 here, no wrap)


def _check(env, want):
    import torch

    got = env.stats_tensor()
    assert got.dtype == torch.int64 and tuple(got.shape) == (3,) and got.tolist() == want
    assert torch.equal(got, env._stats.sum(dim=1))
    out = torch.full((3,), -1, dtype=torch.int64, device=env.device)
    assert env.stats_tensor(out=out) is out and out.tolist() == want
    e = env.episodic_stats()
    assert [e["episodes"], e["return_sum"], e["iou_fx_sum"]] == want


@pytest.mark.parametrize("n", SIZES)
def test_sums_equal_the_arrays_exactly(n):
    import torch

    env = _batch(n)
    want = _fill(env, n)
    _check(env, want)
    for i in range(5):                                               # five calls in a row: the ticket cleans itself
        assert env.stats_tensor().tolist() == want
    torch.cuda.synchronize()
    assert int(env._sums_scratch[-1]) == 0                           # the ticket, back at 0 for the next call
    want = _fill(env, n + 100)                                       # no totals kept between calls: the arrays are the only truth
    _check(env, want)


def test_two_batches_on_two_streams_each_with_its_own_scratch():
    import torch

    a, b = _batch(4099, 1), _batch(257, 2)
    wa, wb = _fill(a, 11), _fill(b, 12)
    assert a._sums_scratch.data_ptr() != b._sums_scratch.data_ptr()
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for i in range(6):
        with torch.cuda.stream(sa):
            outs.append((a.stats_tensor(), wa))
        with torch.cuda.stream(sb):
            outs.append((b.stats_tensor(), wb))
    sa.synchronize(); sb.synchronize()
    for got, want in outs:
        assert got.tolist() == want


def test_the_sums_follow_the_arrays_after_load_state_dict_fork_and_a_rollout():
    import torch

    env = _batch(4099, 3, total_step=5)
    snap = env.state_dict()
    want = _fill(env, 21)
    _check(env, want)
    env.load_state_dict(snap)                                        # the arrays as they were at the snapshot: zeros
    _check(env, [0, 0, 0])
    want = _fill(env, 22)
    child = env.fork(torch.arange(0, 4099, 2, device=env.device))    # a fork starts its sums at zero, with a scratch of its own
    _check(child, [0, 0, 0])
    _check(env, want)
    env.rollout(7)                                                   # time limit 5: every env finishes an episode
    after = env._stats.sum(dim=1).tolist()
    assert after[0] >= want[0] + 4099
    _check(env, after)


def test_out_must_be_an_int64_triple_on_the_device():
    import torch

    env = _batch(64)
    with pytest.raises(ValueError):
        env.stats_tensor(out=torch.zeros(3, dtype=torch.int32, device=env.device))
    with pytest.raises(ValueError):
        env.stats_tensor(out=torch.zeros(4, dtype=torch.int64, device=env.device))
    wide = torch.zeros(6, dtype=torch.int64, device=env.device)
    want = _fill(env, 5)
    assert env.stats_tensor(out=wide[::2]).tolist() == want and wide[1::2].tolist() == [0, 0, 0]   # a strided out= is written through a copy
