"""GPU: counter-RNG actions drawn from a caller-given distribution (BatchedDMPEnv(action_probs=...), snac_env_desc.action_dist).

(a) a rollout / step whose actions the device draws from p equals, byte for byte, the same call on a twin without a distribution fed
    those actions explicitly (drawn on the host from tests/rng_spec.py with p; step sizes from the counter RNG in both) -- the twin's
    explicit-action path is oracle-checked by the existing tests, so this pins the new path to the reference's rules -- on every
    rollout and step kernel of the dispatch (profiles/r06_dispatch.txt; snac_last_kernel() asserted);
(b) the uniform table draws exactly what no distribution draws;
(c) the frequencies of the 3D mix, and actions of weight zero never taken;
(d) tree search: NodePool*.evaluate == BatchedDMPEnv.evaluate == fork + explicit-action rollout + the discounted sum;
(e) shards keyed by env_id_base add up to the whole batch."""
import numpy as np
import pytest

from devmem import _kernel
import rng_spec

pytestmark = pytest.mark.gpu

MIX3D = [0.2] * 4 + [0.05] * 4
SKEW = {1: [0.6, 0.1, 0.3], 2: [0.05, 0.3, 0.1, 0.25, 0.3], 3: MIX3D}

# (kind, dynamic, float32 rows, layout, N, T, the kernel the distribution's rollout runs on)
ROLLOUTS = [
    (1, False, False, None, 256, 160, "k_rollout1dt"),
    (1, True, True, "ppo", 1024, 160, "k_rollout1dt"),
    (1, True, False, None, 45056, 40, "k_rollout1dl"),
    (1, True, False, "ppo", 28672, 40, "k_rollout1dl"),
    (2, True, False, None, 256, 160, "k_rollout2dt"),
    (2, False, True, "ppo", 512, 120, "k_rollout2dt"),
    (2, False, True, None, 16384, 40, "k_rollout2db"),
    (2, True, False, None, 40960, 24, "k_rollout2d"),
    (3, True, False, None, 64, 160, "k_rollout3d"),
    (3, False, True, None, 4096, 60, "k_rollout3db"),
    (3, True, False, "ppo", 64, 120, "k_rollout"),
]
# (kind, dynamic, float32 rows, layout, N, the kernel of the distribution's step)
STEPS = [
    (1, True, False, None, 256, "k_step1d"),
    (1, False, True, None, 64, "k_transition"),
    (2, True, False, None, 1024, "k_step2d"),
    (3, False, False, None, 1024, "k_step3dq"),
    (3, True, True, "ppo", 64, "k_transition"),
]


def _id(c):
    return "%dD-%s-%s-%s-%d" % (c[0], "dyn" if c[1] else "static", "f32" if c[2] else "f64", c[3] or "canonical", c[4])


def _env(kind, dyn, f32, layout, n, seed=7, **kw):
    import torch
    from snac_amd import BatchedDMPEnv

    return BatchedDMPEnv(kind, dyn, n, seed=seed, obs_dtype=torch.float32 if f32 else torch.float64, layout=layout, **kw)


def _host_actions(env, probs, ticks, t0, rows=None):
    """[ticks, N] int8: the actions the device draws with `probs` at ticks t0 .. t0 + ticks - 1 (include/snac_hip.h "Counter RNG")."""
    from snac_amd import _lib

    cdf = _lib.action_cdf(probs, env.num_actions).astype(np.uint64)
    ids = np.arange(env.num_envs, dtype=np.uint64) + np.uint64(env.env_id_base) if rows is None else rows
    w = rng_spec.words(env.seed, rng_spec.STREAM_STEP, ids[None, :], (np.arange(ticks, dtype=np.uint64) + np.uint64(t0))[:, None])
    u = (w >> np.uint64(16))[..., None]
    return (u >= cdf).sum(-1).astype(np.int8)


def _record(env, T):
    import torch

    shape = (T, env.num_envs)
    return {"actions": torch.empty(shape, dtype=torch.int8, device=env.device), "step_size": torch.empty(shape, dtype=torch.int8, device=env.device),
            "plan_idx": torch.empty(shape, dtype=torch.int16, device=env.device), "first": torch.empty(shape, dtype=torch.uint8, device=env.device)}


def _b(t):
    return t.cpu().numpy().tobytes()


def _same_state(a, b):
    for x, y in ((a._hdr, b._hdr), (a._grid, b._grid), (a._episode, b._episode), (a._stats, b._stats)):
        assert _b(x) == _b(y)
    assert a.episodic_stats() == b.episodic_stats()


def _advance(env, T, explicit_probs):
    """rollout(T) without outputs: the env's own draw, or the actions drawn on the host with explicit_probs."""
    import torch

    acts = None if explicit_probs is None else torch.from_numpy(_host_actions(env, explicit_probs, T, env.t)).to(env.device)
    env.rollout(T, actions=acts, obs=None)


def _run(case, probs, explicit_probs=None):
    """rollout(T) after a short first rollout, on an env with action_probs=probs; explicit_probs: the actions passed explicitly,
    drawn on the host with those weights.  Returns (env, obs, reward, done, record, kernel)."""
    import torch

    kind, dyn, f32, layout, n, T, _ = case
    env = _env(kind, dyn, f32, layout, n, action_probs=probs)
    env.reset()
    _advance(env, 7, explicit_probs)                                # some envs mid-episode, the tick counter away from 0
    acts = None if explicit_probs is None else torch.from_numpy(_host_actions(env, explicit_probs, T, env.t)).to(env.device)
    rec = _record(env, T)
    obs, rew, done = env.rollout(T, actions=acts, record=rec)
    torch.cuda.synchronize()
    return env, obs, rew, done, rec, _kernel()


def _assert_same(a, b):
    ea, oa, ra, da, reca, _ = a
    eb, ob, rb, db, recb, _ = b
    assert _b(oa) == _b(ob), "observations"
    assert _b(ra) == _b(rb), "rewards"
    assert _b(da) == _b(db), "done"
    for k in ("actions", "step_size", "plan_idx", "first"):
        assert _b(reca[k]) == _b(recb[k]), k
    _same_state(ea, eb)


@pytest.mark.parametrize("case", ROLLOUTS, ids=[_id(c) for c in ROLLOUTS])
def test_a_rollout_with_a_distribution_equals_its_actions_passed_explicitly(case):
    p = SKEW[case[0]]
    dev = _run(case, p)
    assert dev[5] == case[6]
    _assert_same(dev, _run(case, None, explicit_probs=p))
    acts = dev[4]["actions"].cpu().numpy()
    assert np.bincount(acts.reshape(-1).astype(np.int64), minlength=len(p)).min() > 0


@pytest.mark.parametrize("case", ROLLOUTS, ids=[_id(c) for c in ROLLOUTS])
def test_the_uniform_table_draws_what_no_distribution_draws(case):
    A = {1: 3, 2: 5, 3: 8}[case[0]]
    dev = _run(case, [1.0] * A)
    assert dev[0]._desc.action_dist != 0                            # the table path, not handle 0
    assert dev[5] == case[6]
    plain = _run(case, None)
    assert plain[0]._desc.action_dist == 0 and plain[5] == case[6]
    _assert_same(dev, plain)


def _step_run(case, probs, explicit_probs, ticks=6):
    import torch

    kind, dyn, f32, layout, n, _ = case
    env = _env(kind, dyn, f32, layout, n, action_probs=probs)
    env.reset()
    outs, kerns = [], []
    for i in range(ticks):
        if i == 3:
            _advance(env, 200, explicit_probs)                      # then some envs are done: the steps auto-reset them
        acts = None
        if explicit_probs is not None:
            acts = torch.from_numpy(_host_actions(env, explicit_probs, 1, env.t)[0]).to(env.device)
        obs, rew, done = env.step(acts, None, auto_reset=True)
        torch.cuda.synchronize()
        kerns.append(_kernel())
        outs.append((_b(obs), _b(rew), _b(done)))
    return env, outs, kerns


@pytest.mark.parametrize("case", STEPS, ids=[_id(c) + "-" + c[5] for c in STEPS])
def test_a_step_with_a_distribution_equals_its_actions_passed_explicitly(case):
    kind = case[0]
    p = SKEW[kind]
    e1, o1, k1 = _step_run(case, p, None)
    e2, o2, _ = _step_run(case, None, p)
    assert set(k1) == {case[5]}
    assert o1 == o2
    _same_state(e1, e2)
    A = len(p)
    e3, o3, k3 = _step_run(case, [1.0] * A, None)                   # (b) for the step kernels
    e4, o4, _ = _step_run(case, None, None)
    assert set(k3) == {case[5]}
    assert o3 == o4
    _same_state(e3, e4)


def test_the_3d_mix_has_its_frequencies_and_zero_weights_are_never_drawn():
    import torch

    n, T = 16384, 1000
    env = _env(3, True, False, None, n, action_probs=MIX3D)
    env.reset()
    rec = {"actions": torch.empty((T, n), dtype=torch.int8, device=env.device)}
    env.rollout(T, obs=None, record=rec)
    counts = torch.bincount(rec["actions"].reshape(-1).to(torch.int64), minlength=8).cpu().numpy()
    total = n * T
    assert counts.sum() == total
    p = np.diff(np.concatenate([[0], env.action_cdf.astype(np.float64), [65536]])) / 65536
    assert np.allclose(p, MIX3D, atol=2e-5)
    sigma = np.sqrt(total * p * (1 - p))
    assert np.all(np.abs(counts - total * p) < 5 * sigma), (counts, total * p)

    for kind, w in ((2, [1, 0, 1, 0, 1]), (3, [0, 1, 0, 0, 2, 0, 0, 1]), (1, [0, 0, 1])):
        e = _env(kind, True, False, None, 4096, action_probs=w)
        e.reset()
        r = {"actions": torch.empty((300, 4096), dtype=torch.int8, device=e.device)}
        e.rollout(300, record=r)
        seen = set(torch.unique(r["actions"]).cpu().tolist())
        assert seen == {j for j, x in enumerate(w) if x > 0}


@pytest.mark.parametrize("kind,dyn", [(1, False), (1, True), (2, True), (3, False), (3, True)])
def test_tree_evaluation_draws_from_the_distribution(kind, dyn):
    import torch
    from snac_amd import NodePool

    n, H, gamma = 512, {1: 300, 2: 400, 3: 300}[kind], 0.97
    p = SKEW[kind]
    env = _env(kind, dyn, False, None, n, seed=11, action_probs=p)
    env.reset()
    env.rollout({1: 37, 2: 600, 3: 21}[kind], obs=None)            # some rows end on a terminal step
    rows = torch.arange(0, n, 2, device=env.device)
    m = int(rows.numel())
    est_b, steps_b = env.evaluate(rows, H, gamma)
    pool = NodePool(env, n)
    g = torch.Generator(device="cpu").manual_seed(3)
    perm = torch.randperm(n, generator=g).to(env.device)
    assert pool.load(rows=torch.arange(n, device=env.device), node_rows=perm) == n
    est_p, steps_p = pool.evaluate(perm[rows], H, gamma)
    assert _b(est_p) == _b(est_b)
    assert torch.equal(steps_p, steps_b)

    # fork + explicit-action rollout + the discounted sum (script/MCTS/utils/mcts.py:100-110)
    terminal = env.need_reset[rows].cpu().numpy()
    from snac_amd import _lib

    leaves = env.fork(rows)
    leaves.set_action_probs(None)
    leaves.t = 0
    leaves._hdr.view(torch.int8)[:, 2] &= ~_lib.FLAG_NEED_RESET
    acts = torch.from_numpy(_host_actions(leaves, p, H, 0)).to(env.device)
    _, rew, done = leaves.rollout(H, actions=acts, obs=None)
    rew, done = rew.cpu().numpy(), done.cpu().numpy()
    est, steps = np.zeros(m), np.zeros(m, np.int64)
    for i in range(m):
        if terminal[i]:
            continue
        for t in range(H):
            est[i] = est[i] + float(rew[t, i]) * (gamma ** t)
            steps[i] += 1
            if done[t, i]:
                break
    assert est.tobytes() == est_b.cpu().numpy().tobytes()
    assert np.array_equal(steps, steps_b.cpu().numpy())

    plain = _env(kind, dyn, False, None, n, seed=11)
    plain.reset()
    plain.rollout({1: 37, 2: 600, 3: 21}[kind], obs=None)
    est_u, _ = plain.evaluate(rows, H, gamma)
    assert not torch.equal(est_u, est_b)


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_shards_keyed_by_env_id_base_add_up_to_the_batch(kind):
    import torch
    from snac_amd import dist

    N, T = 2048, 150
    p = SKEW[kind]
    whole = dist.make_sharded_env(kind, True, N, rank=0, world=1, seed=5, action_probs=p)
    parts = [dist.make_sharded_env(kind, True, N, rank=r, world=2, seed=5, action_probs=p) for r in (0, 1)]
    assert [e.env_id_base for e in parts] == [0, N // 2]
    outs = []
    for e in [whole] + parts:
        e.reset()
        outs.append(e.rollout(T))
    torch.cuda.synchronize()
    for i in range(3):
        cat = torch.cat([outs[1][i], outs[2][i]], dim=1)
        assert _b(cat) == _b(outs[0][i])
    assert whole.episodic_stats()["episodes"] == sum(e.episodic_stats()["episodes"] for e in parts)
