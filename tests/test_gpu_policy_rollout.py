"""snac_policy_rollout on the GPU: T ticks of observe -> network -> draw -> step in one launch, byte for byte against rollout_rule
(tests/test_policy_rollout_host.py: the oracle's reset, rows and step, mlp_rule and policy_rule composed per tick) through the C ABI with
every output in a guard arena; against the per-tick composition of the entry points that were there before; across shards; and through
BatchedDMPEnv.rollout_policy, ReplayRing.collect_policy, RolloutBuffer.collect_policy and the two examples."""
import ctypes as C

import numpy as np
import pytest

from devmem import _example, _vp
import guard
import helpers
from test_gpu_parity import check_state
from test_policy_act_host import ACTIONS, CATEGORICAL, EPS_GREEDY, GREEDY
from test_policy_rollout_host import (CASES, OBS_ALL, OBS_LAST, OBS_NONE, PRELUDE_TICKS, TOTAL_STEP, case_id, make_net, make_rollout_case, plan_cells,
                                      plan_table, rollout_rule, start)

pytestmark = pytest.mark.gpu

OUTPUTS = ("obs", "reward", "done", "actions", "step_size", "plan_idx", "first", "value", "logp", "entropy")
MODE_NAMES = {CATEGORICAL: "categorical", GREEDY: "greedy", EPS_GREEDY: "eps_greedy"}


def _env(kind, dyn, N, f32, seed, base=0, started=True):
    import torch
    from snac_amd import BatchedDMPEnv

    table = plan_table(kind, dyn)
    full = table.reshape(len(table), 30) if kind == 1 else table.reshape(len(table), 26, 26)
    env = BatchedDMPEnv(kind, dyn, N, plans=full, seed=seed, env_id_base=base, total_step=TOTAL_STEP,
                        obs_dtype=torch.float32 if f32 else torch.float64)
    if started:
        start(env, N, base)
        assert env.t == PRELUDE_TICKS
    return env


def _oracle(kind, dyn, N, seed, base=0):
    orc = helpers.oracle().OracleBatch(kind, dyn, N, plan_table(kind, dyn), seed=seed, env_id_base=base)
    orc.set_total_step(TOTAL_STEP)
    start(orc, N, base)
    return orc


def _place(arr, offset, dev):
    """A numpy array on the device, `offset`: one element into its allocation (aligned as its element type and no wider)."""
    import torch

    flat = torch.zeros((arr.size + 5,), dtype=torch.from_numpy(arr).dtype, device=dev)
    view = flat[1:1 + arr.size] if offset else flat[:arr.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)).reshape(-1).to(dev))
    return flat, view.view(arr.shape)


def _call(case, want=OUTPUTS, offset=False):
    """One call of the entry point on a started env, every output carved from a guard arena -> (dict of numpy arrays, None where NULL;
    bad_rows; the env afterwards)."""
    import torch
    from snac_amd import _lib

    kind, dyn, f32, dims, N, T, mode, eps, t0, obs_mode, head = case
    c = make_rollout_case(case)
    A, D = ACTIONS[kind], 7 if kind == 1 else 51
    env = _env(kind, dyn, N, f32, c["seed"])
    L, dev = _lib.lib(), env.device
    placed = [(_place(w, offset, dev), _place(b, offset, dev)) for w, b in zip(c["weights"], c["biases"])]
    net = _lib.Mlp()
    net.layers = len(dims) - 1
    for l, d in enumerate(dims):
        net.dim[l] = d
    for l, ((_, w), (_, b)) in enumerate(placed):
        net.w[l], net.b[l] = w.data_ptr(), b.data_ptr()
    before = [(fw.clone(), fb.clone()) for (fw, _), (fb, _) in placed]
    eps_flat, eps_env = _place(c["eps"], offset, dev) if np.ndim(c["eps"]) else (None, None)
    eps_before = None if eps_flat is None else eps_flat.clone()
    has_value = dims[-1] == A + 1
    odt = torch.float32 if f32 else torch.float64
    shapes = dict(obs=((T, N, D) if obs_mode == OBS_ALL else (N, D), odt), reward=((T, N), torch.float32), done=((T, N), torch.uint8),
                  actions=((T, N), torch.int8), step_size=((T, N), torch.int8), plan_idx=((T, N), torch.int16), first=((T, N), torch.uint8),
                  value=((T, N), torch.float32), logp=((T, N), torch.float32), entropy=((T, N), torch.float32))
    arena = guard.Arena(T * N * (D * 8 + 24) + 13 * (guard.BAND + 1024), dev)
    out = {}
    for name in OUTPUTS:
        shape, dt = shapes[name]
        size = torch.empty((), dtype=dt).element_size()
        out[name] = arena.carve(shape, dt, offset=size if offset else 0, name=name)
    bad = arena.carve((1,), torch.int32, name="bad_rows").zero_()
    if "obs" not in want:                                            # no rows asked for: SNAC_OBS_NONE (a mode with a null obs is refused)
        obs_mode = OBS_NONE
    defined = set(OUTPUTS) - ({"obs"} if obs_mode == OBS_NONE else set()) - (set() if has_value else {"value"})
    defined -= set() if mode == CATEGORICAL else {"logp", "entropy"}
    given = {k: (out[k] if k in want and k in defined else None) for k in OUTPUTS}
    rec = _lib.RolloutRecord(*[None if given[k] is None else given[k].data_ptr() for k in ("actions", "step_size", "plan_idx", "first")])
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        _lib.check(L.snac_policy_rollout(C.byref(env._desc), C.byref(env._state), C.byref(net), T, t0, mode,
                                         0.0 if eps_env is not None else float(c["eps"]), _vp(eps_env), obs_mode, _vp(given["obs"]),
                                         _vp(given["reward"]), _vp(given["done"]), C.byref(rec), _vp(given["value"]), _vp(given["logp"]),
                                         _vp(given["entropy"]), _vp(bad), stream))
    assert L.snac_last_kernel() == b"k_policy_rollout"
    arena.check()                                                    # nothing lands outside the outputs
    for k in OUTPUTS:
        if given[k] is None:
            guard.view_untouched(out[k], k + " (NULL in the call)")
    for ((fw, _), (fb, _)), (w0, b0) in zip(placed, before):         # bytes: the biases hold NaNs
        assert torch.equal(fw.view(torch.int32), w0.view(torch.int32)) and torch.equal(fb.view(torch.int32), b0.view(torch.int32)), "weights written"
    assert eps_flat is None or torch.equal(eps_flat, eps_before), "epsilon_per_env written"
    return {k: (None if given[k] is None else given[k].cpu().numpy()) for k in OUTPUTS}, int(bad.cpu()[0]), env


def _same(got, c, case, names=OUTPUTS):
    kind, dyn, f32, dims, N, T, mode, eps, t0, obs_mode, head = case
    w = c["want"]
    for k in names:
        if got.get(k) is None:
            continue
        ref = w[k]
        if k == "obs":
            ref = (ref if obs_mode == OBS_ALL else ref[-1]).astype(np.float32 if f32 else np.float64)
        if k == "done" and got[k].dtype == bool:
            ref = ref.astype(bool)
        assert got[k].dtype == ref.dtype and got[k].shape == ref.shape, (k, got[k].dtype, ref.dtype, got[k].shape, ref.shape)
        if got[k].tobytes() != ref.tobytes():
            ne = np.flatnonzero(np.frombuffer(got[k].tobytes(), np.uint8) != np.frombuffer(ref.tobytes(), np.uint8)) // got[k].itemsize
            at = np.unravel_index(int(ne[0]), got[k].shape)
            raise AssertionError((case_id(case), k, "first difference at", at, "got", got[k][at], "want", ref[at], "differing bytes", ne.size))


# ---- the launch against the rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_launch_equals_the_rule_byte_for_byte_and_writes_nothing_else(case):
    c = make_rollout_case(case)
    got, bad, env = _call(case, offset=CASES.index(case) % 2 == 1)
    _same(got, c, case)
    assert bad == c["want"]["bad_rows"]
    assert env.t == PRELUDE_TICKS                                    # the entry point knows nothing of env.t
    check_state(env, c["orc"])                                       # headers, grids, episode counters, episodic sums: the rule's


def test_each_optional_output_may_be_null():
    for case in (CASES[0], CASES[5]):
        c = make_rollout_case(case)
        for left_out in OUTPUTS:
            got, bad, env = _call(case, want=tuple(k for k in OUTPUTS if k != left_out), offset=True)
            assert got[left_out] is None
            _same(got, c, case)
            assert bad == c["want"]["bad_rows"]
        got, bad, env = _call(case, want=())                         # nothing but the state and bad_rows
        assert all(v is None for v in got.values())
        check_state(env, c["orc"])


# ---- through BatchedDMPEnv.rollout_policy ------------------------------------------------------------------------------------------------
def _module(weights, biases, dev):
    import torch

    mods = []
    for l, (w, b) in enumerate(zip(weights, biases)):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
        mods += [lin] + ([torch.nn.ReLU()] if l < len(weights) - 1 else [])
    return torch.nn.Sequential(*mods).to(dev)


def _mlp(c, env):
    from snac_amd import DeviceMLP

    A = env.num_actions
    return DeviceMLP(_module(c["weights"], c["biases"], env.device), env if c["weights"][-1].shape[0] == A + 1 else None)


def _eps(c, env):
    import torch

    return torch.from_numpy(c["eps"]).to(env.device) if np.ndim(c["eps"]) else c["eps"]


def _run(case, base=0, net_of=None):
    """rollout_policy on a started env of the case -> (its dict, the env).  net_of: the case whose network acts (default: the case's own;
    a shard runs the whole batch's network)."""
    kind, dyn, f32, dims, N, T, mode, eps, t0, obs_mode, head = case
    c = make_rollout_case(case, base)
    env = _env(kind, dyn, N, f32, c["seed"], base)
    res = env.rollout_policy(_mlp(make_rollout_case(net_of) if net_of else c, env), T, mode=MODE_NAMES[mode], epsilon=_eps(c, env),
                             obs={OBS_ALL: "all", OBS_LAST: "last", OBS_NONE: None}[obs_mode], want_entropy=mode == CATEGORICAL, record=True)
    return res, env


def _state_bytes(env):
    return b"".join(t.cpu().numpy().tobytes() for t in (env._hdr, env._episode, env._grid, env._stats))


def _py_case(case, t0=PRELUDE_TICKS, **kw):
    """A case as the Python methods run it: env.t is the tick, so t0 is the prelude's end."""
    kind, dyn, f32, dims, N, T, mode, eps, _, obs_mode, head = case
    new = dict(kind=kind, dyn=dyn, f32=f32, dims=dims, N=N, T=T, mode=mode, eps=eps, t0=t0, obs_mode=obs_mode, head=head)
    new.update(kw)
    return tuple(new[k] for k in ("kind", "dyn", "f32", "dims", "N", "T", "mode", "eps", "t0", "obs_mode", "head"))


PY_CASES = tuple(_py_case(CASES[i]) for i in (2, 4, 8, 11))


@pytest.mark.parametrize("case", PY_CASES, ids=case_id)
def test_rollout_policy_equals_the_rule_and_the_composition_of_the_existing_entry_points(case):
    import torch

    kind, dyn, f32, dims, N, T, mode, eps, t0, obs_mode, head = case
    c = make_rollout_case(case)
    res, env = _run(case)
    assert env.t == PRELUDE_TICKS + T and res["done"].dtype == torch.bool
    _same({k: v.cpu().numpy() for k, v in res.items()}, c, case)
    assert int(env.policy_bad_rows.cpu()[0]) == c["want"]["bad_rows"]
    check_state(env, c["orc"])
    # per tick, with the entry points that were there before: masked reset, observe, forward, draw, step
    twin = _env(kind, dyn, N, f32, c["seed"])
    mlp, A = _mlp(c, twin), twin.num_actions
    ticks = dict(obs=[], reward=[], done=[], actions=[], logp=[], entropy=[], value=[])
    for j in range(T):
        rows = twin.reset(mask=twin.need_reset)
        x = rows.float()
        if dims[0] != twin.obs_dim:
            x = torch.cat([x, twin.input_plan().float().flatten(1)], 1)
        y = mlp.forward(x.contiguous())
        scores = y[:, :A].contiguous()
        if mode == CATEGORICAL:
            a, lp, en = twin.sample_actions(scores, want_entropy=True)
            ticks["logp"].append(lp)
            ticks["entropy"].append(en)
        else:
            a = twin.epsilon_greedy(scores, _eps(c, twin) if mode == EPS_GREEDY else 0.0)
        if dims[-1] == A + 1:
            ticks["value"].append(y[:, A].clone())
        o, r, d = twin.step(a, auto_reset=False)
        for k, v in (("obs", o), ("reward", r), ("done", d), ("actions", a)):
            ticks[k].append(v.clone())
    for k, rows in ticks.items():
        if k in res and rows:
            whole = torch.stack(rows) if (k != "obs" or obs_mode == OBS_ALL) else rows[-1]
            assert whole.dtype == res[k].dtype and whole.cpu().numpy().tobytes() == res[k].cpu().numpy().tobytes(), k
    assert _state_bytes(twin) == _state_bytes(env) and twin.t == env.t
    assert int(twin.policy_bad_rows.cpu()[0]) == int(env.policy_bad_rows.cpu()[0])


def test_a_batch_in_shards_gives_the_same_bytes():
    case = _py_case(CASES[4], N=33, mode=EPS_GREEDY, eps="per_env")
    whole, env = _run(case)
    parts = [_run(_py_case(case, N=n), base=b, net_of=case) for b, n in ((0, 16), (16, 17))]
    for k, v in whole.items():
        joined = np.concatenate([p[0][k].cpu().numpy() for p in parts], axis=1 if v.dim() > 1 else 0)
        assert joined.tobytes() == v.cpu().numpy().tobytes(), k
    for t in ("_hdr", "_episode", "_grid"):
        assert np.concatenate([getattr(p[1], t).cpu().numpy() for p in parts]).tobytes() == getattr(env, t).cpu().numpy().tobytes(), t
    assert np.concatenate([p[1]._stats.cpu().numpy() for p in parts], axis=1).tobytes() == env._stats.cpu().numpy().tobytes()
    _same({k: v.cpu().numpy() for k, v in whole.items()}, make_rollout_case(case), case)


def test_two_runs_give_the_same_bytes():
    for case in (PY_CASES[1], PY_CASES[3]):
        runs = [_run(case) for _ in range(2)]
        for k in runs[0][0]:
            assert runs[0][0][k].cpu().numpy().tobytes() == runs[1][0][k].cpu().numpy().tobytes(), k
        assert _state_bytes(runs[0][1]) == _state_bytes(runs[1][1])


def test_the_weights_are_read_in_place_at_every_call():
    import torch

    case = _py_case(CASES[5], T=4)
    kind, dyn, f32, dims, N, T, mode, eps, t0, obs_mode, head = case
    c = make_rollout_case(case)
    env = _env(kind, dyn, N, f32, c["seed"])
    mlp = _mlp(c, env)
    kw = dict(mode="greedy", obs="all", record=True)
    first = env.rollout_policy(mlp, T, **kw)
    with torch.no_grad():
        for w, b in mlp._params:                                     # an optimiser's in-place step
            w.mul_(-1.0)
            b.add_(0.25)
    second = env.rollout_policy(mlp, T, **kw)
    # the rule with the first weights for T ticks, then with the changed ones
    orc = _oracle(kind, dyn, N, c["seed"])
    cells = plan_cells(kind, plan_table(kind, dyn))
    w1 = rollout_rule(orc, cells, c["weights"], c["biases"], T, PRELUDE_TICKS, GREEDY, 0.0, c["seed"])
    changed = [-w for w in c["weights"]], [b + np.float32(0.25) for b in c["biases"]]
    w2 = rollout_rule(orc, cells, changed[0], changed[1], T, PRELUDE_TICKS + T, GREEDY, 0.0, c["seed"])
    for got, want in ((first, w1), (second, w2)):
        for k in ("actions", "reward", "value", "plan_idx"):
            assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
        assert got["obs"].cpu().numpy().tobytes() == want["obs"].astype(np.float32 if f32 else np.float64).tobytes()
    stale = rollout_rule(_oracle_after(kind, dyn, N, c, T), cells, c["weights"], c["biases"], T, PRELUDE_TICKS + T, GREEDY, 0.0, c["seed"])
    assert stale["actions"].tobytes() != w2["actions"].tobytes()     # the old weights would have acted otherwise
    check_state(env, orc)


def _oracle_after(kind, dyn, N, c, T):
    orc = _oracle(kind, dyn, N, c["seed"])
    rollout_rule(orc, c["cells"], c["weights"], c["biases"], T, PRELUDE_TICKS, GREEDY, 0.0, c["seed"])
    return orc


# ---- the ring and the buffer -------------------------------------------------------------------------------------------------------------
def test_collect_policy_across_a_ring_wrap_equals_appending_the_rules_actions():
    import torch
    from snac_amd import ReplayRing

    case = _py_case(CASES[5], N=33, T=12, dims=(451, 16, 5), eps=0.3)
    kind, dyn, f32, dims, N, T, mode, eps, t0, obs_mode, head = case
    c = make_rollout_case(case)
    envs = [_env(kind, dyn, N, f32, c["seed"]) for _ in range(2)]
    rings = [ReplayRing(e, 8, prioritized=True) for e in envs]
    mlp = _mlp(c, envs[0])
    rings[0].collect_policy(mlp, 5, mode="eps_greedy", epsilon=eps)
    rings[0].collect_policy(mlp, 7, mode="eps_greedy", epsilon=eps)   # slots 5, 6, 7, then 0 .. 3: two launches
    for j in range(T):
        rings[1].append(torch.from_numpy(c["want"]["actions"][j]))
    assert rings[0].head == rings[1].head == 4 and rings[0].ticks == rings[1].ticks == T and envs[0].t == envs[1].t == PRELUDE_TICKS + T
    for name in ("obs", "reward", "done", "action", "step_size", "plan_idx", "first"):
        assert getattr(rings[0], name).cpu().numpy().tobytes() == getattr(rings[1], name).cpu().numpy().tobytes(), name
    assert torch.equal(rings[0].tree.weights(), rings[1].tree.weights())
    assert _state_bytes(envs[0]) == _state_bytes(envs[1])
    check_state(envs[0], c["orc"])
    with pytest.raises(ValueError, match="layout='ticks'"):
        ReplayRing(envs[1], 8, layout="tiled").collect_policy(mlp, 2)


def test_the_buffers_collect_policy_equals_act_logits_tick_by_tick():
    import torch
    from snac_amd import DeviceMLP, RolloutBuffer

    case = _py_case(CASES[4], N=65, T=6, dims=(451, 32, 6), mode=CATEGORICAL, head="plain")
    kind, dyn, f32, dims, N, T, mode, eps, t0, obs_mode, head = case
    c = make_rollout_case(case)
    envs = [_env(kind, dyn, N, f32, c["seed"]) for _ in range(2)]
    bufs = [RolloutBuffer(e, 4, 0.97, 0.9) for e in envs]             # a ring of five slots: six ticks wrap it
    mlps = [_mlp(c, e) for e in envs]
    bufs[0].collect_policy(mlps[0], 2)
    bufs[0].collect_policy(mlps[0], 4)
    A = envs[1].num_actions
    for j in range(T):
        e = envs[1]
        rows = e.reset(mask=e.need_reset)                            # the rule's order: a finished env starts over before it is observed
        y = mlps[1].forward(torch.cat([rows.float(), e.input_plan().float().flatten(1)], 1))
        bufs[1].act_logits(y[:, :A].contiguous(), y[:, A])
    assert bufs[0].collected == bufs[1].collected == T and bufs[0].ring.head == bufs[1].ring.head
    for name in ("obs", "reward", "done", "action", "step_size", "plan_idx", "first"):
        assert getattr(bufs[0].ring, name).cpu().numpy().tobytes() == getattr(bufs[1].ring, name).cpu().numpy().tobytes(), name
    for name in ("value", "logp"):
        assert getattr(bufs[0], name).cpu().numpy().tobytes() == getattr(bufs[1], name).cpu().numpy().tobytes(), name
    want = c["want"]                                                 # and the rule's, slot by slot (the ring of 5 holds the newest 5 ticks)
    for j in range(1, T):
        assert bufs[0].logp[j % 5].cpu().numpy().tobytes() == want["logp"][j].tobytes() and bufs[0].value[j % 5].cpu().numpy().tobytes() == want["value"][j].tobytes()
    boot = torch.from_numpy(np.random.default_rng(1).normal(size=N).astype(np.float32))
    for b in bufs:
        b.finish(boot)
    assert torch.equal(bufs[0].adv, bufs[1].adv) and torch.equal(bufs[0].ret, bufs[1].ret)
    with pytest.raises(ValueError, match="actor-critic"):
        bufs[0].collect_policy(DeviceMLP(_module(*make_net(np.random.default_rng(2), (451, 5), 5), envs[0].device), None), 1)


# ---- the examples ------------------------------------------------------------------------------------------------------------------------
def test_the_ppo_example_with_the_device_rollout_finishes_with_finite_losses():
    losses, returns = _example("ppo_batched").run(envs=256, iterations=2, horizon=8, epochs=1, batch=1024, device_rollout=True, log=lambda line: None)
    assert len(losses) == 2 * 2 and all(np.isfinite(losses)) and len(returns) == 2


def test_the_dqn_example_with_the_device_rollout_finishes_with_finite_losses():
    losses, returns = _example("dqn_batched").run(envs=256, ticks=2, batch=256, prefill=8, device_rollout=4, log=lambda line: None)
    assert len(losses) == 2 and all(np.isfinite(losses))
