"""GPU: snac_policy_act, BatchedDMPEnv.sample_actions / epsilon_greedy and RolloutBuffer.act_logits.

The kernel through the C ABI on the generated score rows of tests/test_policy_act_host.py (make_scores: normal, all equal, one and several
-inf, a spread of +-50, and the three sorts of bad row; that they contain every case is asserted there, on the host), byte for byte against
policy_rule, with every output carved from a guard arena: nothing lands outside [0, N) of the outputs, `scores` keeps its bytes, a NULL
output is not written, the count of bad rows is exact.  `scores` is also taken one float into a larger tensor (a base aligned to 4 bytes
only).  Then sharding, the Python surface, RolloutBuffer.act_logits against act() fed with the rule's arrays, and the two examples."""
import ctypes as C

import numpy as np
import pytest

from devmem import _example, _vp, short_env
import guard
from test_policy_act_host import ACTIONS, CATEGORICAL, EPS_GREEDY, GREEDY, bad_rows_of, make_scores, policy_rule

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 4099)                                   # ragged waves, several blocks, a ragged last block


def _desc(kind, seed, base):
    from snac_amd import _lib

    return _lib.EnvDesc(kind, 1, 1, 1, 0, 0, seed, base, 0, 0, 0, 0, 0, 0)     # num_envs is not read: N is the number of rows


def _call(kind, N, t, mode, scores, seed=1, base=0, eps=0.0, want=("action", "logp", "entropy"), offset=False):
    """One call with its outputs in a guard arena -> dict of numpy arrays (None where not asked for) and bad_rows.  scores: numpy [N, A];
    offset: placed one float into a larger tensor.  eps: a number or a float32 [N] array."""
    import torch
    from snac_amd import _lib

    L, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    A = ACTIONS[kind]
    flat = torch.full((N * A + 9,), 7.0, dtype=torch.float32, device=dev)
    at = 1 if offset else 0
    sc = flat[at:at + N * A].view(N, A)
    sc.copy_(torch.from_numpy(scores))
    assert sc.data_ptr() % 16 == (4 if offset else 0) and sc.is_contiguous()
    before = flat.clone()
    arena = guard.Arena(N * 9 + 8 * (guard.BAND + 1024), dev)
    out = dict(action=arena.carve((N,), torch.int8, offset=1 if offset else 0, name="action"),
               logp=arena.carve((N,), torch.float32, offset=4 if offset else 0, name="logp"),
               entropy=arena.carve((N,), torch.float32, offset=4 if offset else 0, name="entropy"))
    bad = arena.carve((1,), torch.int32, name="bad_rows").zero_()
    eps_t = torch.from_numpy(np.asarray(eps, np.float32)).to(dev) if np.ndim(eps) else None
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    d = _desc(kind, seed, base)
    _lib.check(L.snac_policy_act(C.byref(d), N, t, mode, _vp(sc), 0.0 if eps_t is not None else float(eps), _vp(eps_t),
                                 *[_vp(out[k]) if k in want else None for k in ("action", "logp", "entropy")], _vp(bad), stream))
    arena.check()
    for k in out:
        if k not in want:
            guard.view_untouched(out[k], k + " (NULL in the call)")
    assert torch.equal(flat.view(torch.int32), before.view(torch.int32)), "scores were written"      # bytes: the rows hold NaNs
    res = {k: (out[k].cpu().numpy() if k in want else None) for k in out}
    res["bad_rows"] = int(bad.cpu()[0])
    return res


def _same(got, want, what):
    for k in ("action", "logp", "entropy"):
        if got[k] is not None:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)
    assert got["bad_rows"] == want["bad_rows"], what


def _shifts(N):
    return range(8) if N == 1 else (N % 8,)                         # a single row takes every sort in turn


# ---- the kernel against the rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_the_categorical_mode_equals_the_rule_byte_for_byte(kind, N):
    A = ACTIONS[kind]
    for shift in _shifts(N):
        scores = make_scores(np.random.default_rng(1000 * kind + N + shift), N, A, shift)
        for seed, base, t, offset in ((1, 0, 0, False), (1, 0, 0xFFFFFFFF, True), (0x123456789ABCDEF, (1 << 33) + 5, 77, True)):
            want = policy_rule(seed, base + np.arange(N, dtype=np.uint64), t, CATEGORICAL, scores)
            assert want["bad_rows"] == bad_rows_of(N, shift)
            got = _call(kind, N, t, CATEGORICAL, scores, seed, base, offset=offset)
            _same(got, want, (kind, N, shift, seed, t))
            assert got["action"].min() >= 0 and got["action"].max() < A
    # any subset of the outputs: the ones left out are not written, the others do not change
    for subset in (("action",), ("logp",), ("entropy",), ("action", "entropy")):
        part = _call(kind, N, 77, CATEGORICAL, scores, seed, base, want=subset, offset=True)
        _same(part, want, (kind, N, subset))


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_the_greedy_and_epsilon_greedy_modes_equal_the_rule(kind, N):
    A = ACTIONS[kind]
    rng = np.random.default_rng(2000 * kind + N)
    for shift in _shifts(N):
        scores = make_scores(rng, N, A, shift)
        ids = np.arange(N, dtype=np.uint64) + np.uint64(11)
        greedy = _call(kind, N, 5, GREEDY, scores, 3, 11, want=("action",), offset=True)
        _same(greedy, policy_rule(3, ids, 5, GREEDY, scores), (kind, N, shift, "greedy"))
        per_env = rng.choice(np.array([0.0, 0.05, 0.4, 1.0, 0.999999, 1e-6], np.float32), N)
        for t, eps in ((5, 0.0), (5, 0.25), (6, 0.25), (5, 1.0), (5, per_env)):
            got = _call(kind, N, t, EPS_GREEDY, scores, 3, 11, eps=eps, want=("action",), offset=bool(t & 1))
            _same(got, policy_rule(3, ids, t, EPS_GREEDY, scores, eps), (kind, N, shift, t, "eps"))
            assert got["action"].min() >= 0 and got["action"].max() < A
            if np.ndim(eps) == 0 and eps == 0.0:
                assert got["action"].tobytes() == greedy["action"].tobytes()      # epsilon = 0 is the greedy mode
            if np.ndim(eps) == 0 and eps == 1.0:                     # epsilon = 1 never takes the greedy branch: the uniform draw alone
                import rng_spec

                w = rng_spec.words(3, 5, ids, np.uint64(t))
                assert got["action"].tolist() == (((w & np.uint64(0xFFFF)) * np.uint64(A)) >> np.uint64(16)).tolist()


def test_ties_take_the_lowest_index_and_uniform_weights():
    for kind, A in ACTIONS.items():
        scores = np.full((257, A), -2.5, np.float32)
        assert not _call(kind, 257, 0, GREEDY, scores, want=("action",))["action"].any()
        assert not _call(kind, 257, 0, EPS_GREEDY, scores, eps=0.0, want=("action",))["action"].any()
        got = _call(kind, 257, 0, CATEGORICAL, scores)
        assert set(got["action"].tolist()) == set(range(A))
        assert np.allclose(got["logp"], -np.log(A), atol=1e-6) and np.allclose(got["entropy"], np.log(A), atol=1e-6)


def test_the_draws_do_not_depend_on_the_sharding():
    for kind, A in ACTIONS.items():
        scores = make_scores(np.random.default_rng(kind), 256, A)
        for mode, eps in ((CATEGORICAL, 0.0), (EPS_GREEDY, 0.3)):
            want = ("action", "logp", "entropy") if mode == CATEGORICAL else ("action",)
            whole = _call(kind, 256, 9, mode, scores, 7, 0, eps=eps, want=want)
            halves = [_call(kind, 128, 9, mode, scores[b:b + 128], 7, b, eps=eps, want=want) for b in (0, 128)]
            for k in want:
                assert whole[k].tobytes() == halves[0][k].tobytes() + halves[1][k].tobytes(), (kind, mode, k)
            assert whole["bad_rows"] == halves[0]["bad_rows"] + halves[1]["bad_rows"] == bad_rows_of(256)


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_sample_actions_and_epsilon_greedy_follow_env_t(kind):
    import torch

    N = 65
    env, _ = short_env(kind, N, True, seed=9, env_id_base=1000)
    A, ids = env.num_actions, 1000 + np.arange(N, dtype=np.uint64)
    scores = make_scores(np.random.default_rng(kind), N, A)
    logits = torch.from_numpy(scores).to(env.device)
    env.step()
    env.step()
    assert env.t == 2
    want = policy_rule(9, ids, 2, CATEGORICAL, scores)
    action, logp, entropy = env.sample_actions(logits, want_entropy=True)
    assert action.dtype == torch.int8 and action.cpu().numpy().tobytes() == want["action"].tobytes()
    assert logp.cpu().numpy().tobytes() == want["logp"].tobytes() and entropy.cpu().numpy().tobytes() == want["entropy"].tobytes()
    assert int(env.policy_bad_rows.cpu()[0]) == bad_rows_of(N) and env.t == 2
    a2, l2, e2 = env.sample_actions(logits.double(), t=3, want_logp=False)      # converted; another tick, other draws
    assert l2 is None and e2 is None and a2.cpu().numpy().tobytes() == policy_rule(9, ids, 3, CATEGORICAL, scores)["action"].tobytes()
    out = (torch.empty(N, dtype=torch.int8, device=env.device), torch.empty(N, device=env.device), None)
    got = env.sample_actions(logits, out=out)
    assert got[0] is out[0] and got[1] is out[1] and got[2] is None and torch.equal(got[0], action) and torch.equal(got[1], logp)
    for eps in (0.0, 0.25, 1.0):
        assert env.epsilon_greedy(logits, eps).cpu().numpy().tobytes() == policy_rule(9, ids, 2, EPS_GREEDY, scores, eps)["action"].tobytes()
    per_env = np.linspace(0.0, 1.0, N).astype(np.float32)
    assert env.epsilon_greedy(logits, torch.from_numpy(per_env), t=4).cpu().numpy().tobytes() == policy_rule(9, ids, 4, EPS_GREEDY, scores, per_env)["action"].tobytes()
    with pytest.raises(ValueError, match="logits must have shape"):
        env.sample_actions(logits[:, :-1])
    with pytest.raises(ValueError, match="q must have shape"):
        env.epsilon_greedy(logits[:-1], 0.1)
    for bad in (-0.1, 1.5, float("nan"), True, "0.1"):
        with pytest.raises(ValueError, match="epsilon must be"):
            env.epsilon_greedy(logits, bad)
    with pytest.raises(ValueError, match="one value per env"):
        env.epsilon_greedy(logits, torch.zeros(N + 1))
    with pytest.raises(ValueError, match="t must be"):
        env.sample_actions(logits, t=-1)


def test_act_logits_equals_act_with_the_rules_arrays():
    """Horizon 4 at N = 65: act_logits on one env, act(actions, value, logp) with the restatement's arrays on an identically seeded one."""
    import torch
    from snac_amd import RolloutBuffer

    N, H, kind = 65, 4, 2
    bufs = [RolloutBuffer(short_env(kind, N, True, seed=5)[0], H, 0.97, 0.9) for _ in range(2)]
    rng = np.random.default_rng(4)
    for tick in range(H):
        scores, value = make_scores(rng, N, 5, tick), rng.normal(size=N).astype(np.float32)
        assert bufs[0].env.t == bufs[1].env.t == tick
        want = policy_rule(5, np.arange(N), tick, CATEGORICAL, scores)
        got = bufs[0].act_logits(torch.from_numpy(scores).to(bufs[0].env.device), torch.from_numpy(value))
        assert got.dtype == torch.int8 and got.cpu().numpy().tobytes() == want["action"].tobytes()
        bufs[1].act(torch.from_numpy(want["action"]), torch.from_numpy(value), torch.from_numpy(want["logp"]))
    for name in ("action", "reward", "done"):
        assert getattr(bufs[0].ring, name).cpu().numpy().tobytes() == getattr(bufs[1].ring, name).cpu().numpy().tobytes(), name
    for name in ("logp", "value"):
        assert getattr(bufs[0], name).cpu().numpy().tobytes() == getattr(bufs[1], name).cpu().numpy().tobytes(), name
    boot = torch.from_numpy(rng.normal(size=N).astype(np.float32))
    for b in bufs:                                                   # finish() and minibatches() run on it unchanged
        b.finish(boot)
    assert torch.equal(bufs[0].adv, bufs[1].adv) and torch.equal(bufs[0].ret, bufs[1].ret)
    sizes = [len(mb["action"]) for mb in bufs[0].minibatches(64)]
    assert sizes == [64] * (H * N // 64) + [H * N % 64]


# ---- the examples ------------------------------------------------------------------------------------------------------------------------
def test_the_ppo_example_with_device_sampling_repeats_itself():
    mod = _example("ppo_batched")
    runs = [mod.run(envs=256, iterations=2, horizon=8, epochs=1, batch=1024, device_sampling=True, log=lambda line: None) for _ in range(2)]
    assert len(runs[0][0]) == 2 * 2 and all(np.isfinite(runs[0][0])) and runs[0][0] == runs[1][0]


def test_the_dqn_example_with_device_sampling_repeats_itself():
    mod = _example("dqn_batched")
    runs = [mod.run(envs=256, ticks=2, batch=256, prefill=8, device_sampling=True, log=lambda line: None) for _ in range(2)]
    assert len(runs[0][0]) == 2 and all(np.isfinite(runs[0][0])) and runs[0][0] == runs[1][0]
