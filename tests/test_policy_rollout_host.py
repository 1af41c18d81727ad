"""snac_policy_rollout on the host: the entry point's export and argument checks (they run before any HIP call, so they run without a
GPU), the refusals of the Python methods, and the reference of tests/test_gpu_policy_rollout.py -- rollout_rule(), the rule of
include/snac_hip.h, "Acting with the device network over a rollout", in numpy: per tick the oracle's masked reset and observation rows,
mlp_rule (tests/test_mlp_host.py), policy_rule (tests/test_policy_act_host.py) and the oracle's step, composed in the header's order --
with make_rollout_case(), the generated inputs of the GPU tests, and the assertion that they contain every sort of tick."""
import ctypes as C

import numpy as np
import pytest

from cabi_checks import PH, _err_code as _err, _net
import helpers
import rng_spec
from snac_amd import _lib
from test_mlp_host import mlp_rule
from test_policy_act_host import ACTIONS, CATEGORICAL, EPS_GREEDY, GREEDY, eps_fx_of, policy_rule

OBS_NONE, OBS_ALL, OBS_LAST, OBS_TILED = 0, 1, 2, 3
OBS_DIM = {1: 7, 2: 51, 3: 51}
PLAN_CELLS = {1: 30, 2: 400, 3: 400}
TOTAL_STEP = 5                                                       # episodes end within a dozen ticks
PRELUDE_TICKS = 5                                                    # the ticks start() spends: a case's own t0 is free of them


# ---- the rule, in numpy ------------------------------------------------------------------------------------------------------------------
def plan_table(kind, dyn):
    return helpers.plan_table(kind, True, "sin_train" if kind == 1 else "dense_train")[:16] if dyn else helpers.plan_table(kind, False, "p0")


def plan_cells(kind, table):
    """float32 [P, 30 / 400]: input_plan of every row of the table, row-major"""
    return (table if kind == 1 else table.reshape(len(table), 26, 26)[:, 3:23, 3:23].reshape(len(table), -1)).astype(np.float32)


def rollout_rule(orc, cells, weights, biases, T, t0, mode, eps=0.0, seed=1, base=0):
    """T ticks on the OracleBatch `orc` (advanced in place; its state afterwards is the rule's) -> dict of [T, N] arrays (obs float64
    [T, N, D]: a float32 output is its astype(float32)), bad_rows, and what the sorts test looks at (reset bool [T, N], explore bool
    [T, N] or None, scores float32 [T, N, A])."""
    N, A, D = orc.n, orc.num_actions, orc.obs_dim
    ids = np.uint64(base) + np.arange(N, dtype=np.uint64)
    plan_in, has_value = weights[0].shape[1] != D, weights[-1].shape[0] == A + 1
    assert weights[0].shape[1] in (D, D + cells.shape[1]) and weights[-1].shape[0] in (A, A + 1)
    out = dict(obs=np.zeros((T, N, D)), reward=np.zeros((T, N), np.float32), done=np.zeros((T, N), np.uint8), actions=np.zeros((T, N), np.int8),
               step_size=np.zeros((T, N), np.int8), plan_idx=np.zeros((T, N), np.int16), first=np.zeros((T, N), np.uint8),
               value=np.zeros((T, N), np.float32) if has_value else None, logp=np.zeros((T, N), np.float32) if mode == CATEGORICAL else None,
               entropy=np.zeros((T, N), np.float32) if mode == CATEGORICAL else None, bad_rows=0, reset=np.zeros((T, N), bool),
               explore=np.zeros((T, N), bool) if mode == EPS_GREEDY else None, scores=np.zeros((T, N, A), np.float32))
    for j in range(T):
        tau = (t0 + j) & 0xFFFFFFFF
        need = orc.state()["need_reset"]
        rows = orc.reset(mask=need)                                  # 1. the reset of snac_reset(mask = need_reset); 2. the rows of snac_observe
        x = rows.astype(np.float32)
        if plan_in:
            x = np.concatenate([x, cells[orc.state()["plan_idx"]]], axis=1)
        y = mlp_rule(weights, biases, x)["y"]                        # 3. the network
        p = policy_rule(seed, ids, tau, mode, y[:, :A], eps)         # 4. the draw
        out["bad_rows"] += p["bad_rows"]
        o, r, d = orc.step(tau, actions=p["action"], step_size=None, auto_reset=False)   # 5. the step: the step size of stream 0
        st = orc.state()
        out["obs"][j], out["reward"][j], out["done"][j], out["actions"][j] = o, r, d, p["action"]
        out["step_size"][j] = rng_spec.step_size_of(rng_spec.words(seed, 0, ids, np.uint64(tau)))
        out["plan_idx"][j], out["first"][j], out["reset"][j], out["scores"][j] = st["plan_idx"], st["cs"] == 1, need != 0, y[:, :A]
        for k in ("logp", "entropy"):
            if out[k] is not None:
                out[k][j] = p[k]
        if has_value:
            out["value"][j] = y[:, A]
        if mode == EPS_GREEDY:
            w = rng_spec.words(seed, 5, ids, np.uint64(tau))
            e = eps_fx_of(np.float32(eps) if np.ndim(eps) else np.float64(eps))
            out["explore"][j] = (w >> np.uint64(16)) < e
    return out


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------------
HEADS = ("plain", "masked", "bad_nan", "bad_inf", "value_inf")


def make_net(rng, dims, A, head="plain"):
    """(weights, biases) float32.  N(0, 1 / K) weights; the last layer's ten times that, so that the scores spread and the greedy action
    changes from env to env.  head: "masked": the bias of one score is -inf; "bad_nan" / "bad_inf": of one score NaN / +inf (every row
    is bad); "value_inf": the bias of the value output is +inf (needs dims[-1] == A + 1)."""
    L = len(dims) - 1
    weights = [(rng.normal(size=(dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32) for l in range(L)]
    biases = [(0.1 * rng.normal(size=dims[l + 1])).astype(np.float32) for l in range(L)]
    weights[-1] *= np.float32(10.0)
    a = int(rng.integers(A))
    if head == "masked":
        biases[-1][a] = -np.inf
    elif head == "bad_nan":
        biases[-1][a] = np.nan
    elif head == "bad_inf":
        biases[-1][a] = np.inf
    elif head == "value_inf":
        assert dims[-1] == A + 1
        biases[-1][A] = np.inf
    else:
        assert head == "plain"
    return weights, biases


def start(batch, N, base=0):
    """The start state of every case, on an OracleBatch or a BatchedDMPEnv alike (the calls they share): episodes staggered by global env
    id, so that at the first tick the envs with (id % 3 != 0) carry SNAC_FLAG_NEED_RESET and the others are two ticks from their
    time limit.  Spends PRELUDE_TICKS ticks of the counter RNG."""
    ids = base + np.arange(N)
    oracle = hasattr(batch, "b")

    def tick(t):
        if oracle:
            batch.step(t, auto_reset=True)
        else:
            assert batch.t == t
            batch.step(auto_reset=True, want_obs=False)

    batch.reset()
    tick(0)
    tick(1)
    batch.reset(mask=(ids % 3 == 0).astype(np.uint8))
    for t in (2, 3, 4):
        tick(t)


# kind, dynamic, float32 rows, dims, N, T, mode, eps ("per_env" or a number), t0, obs_mode, head
WRAP = (1 << 32) - 3
CASES = (
    (1, True, False, (7, 4), 17, 24, CATEGORICAL, 0.0, 0, OBS_ALL, "plain"),
    (1, False, True, (7, 4), 1, 24, CATEGORICAL, 0.0, WRAP, OBS_ALL, "value_inf"),
    (1, True, True, (37, 8, 3), 33, 24, EPS_GREEDY, "per_env", 0, OBS_LAST, "plain"),
    (1, False, False, (37, 8, 3), 16, 2, GREEDY, 0.0, 7, OBS_NONE, "masked"),
    (2, True, True, (51, 64, 6), 260, 24, CATEGORICAL, 0.0, 0, OBS_ALL, "plain"),
    (2, True, False, (51, 64, 6), 15, 24, EPS_GREEDY, 0.3, WRAP, OBS_ALL, "plain"),
    (2, False, False, (51, 64, 6), 16, 1, CATEGORICAL, 0.0, 5, OBS_LAST, "bad_nan"),
    (2, False, True, (51, 64, 6), 17, 2, GREEDY, 0.0, 5, OBS_ALL, "bad_inf"),
    (2, True, True, (51, 65, 1, 5), 33, 24, EPS_GREEDY, "per_env", WRAP, OBS_NONE, "masked"),
    (2, False, False, (51, 65, 1, 5), 1, 24, GREEDY, 0.0, 0, OBS_ALL, "plain"),
    (2, True, False, (451, 256, 255, 6), 17, 3, CATEGORICAL, 0.0, WRAP, OBS_ALL, "masked"),
    (3, True, False, (51, 16, 9), 33, 24, CATEGORICAL, 0.0, WRAP, OBS_ALL, "plain"),
    (3, False, True, (51, 16, 9), 17, 24, EPS_GREEDY, 0.3, 0, OBS_LAST, "value_inf"),
    (3, True, True, (51, 16, 9), 15, 2, GREEDY, 0.0, 9, OBS_ALL, "masked"),
    (3, False, False, (51, 16, 9), 260, 1, CATEGORICAL, 0.0, 11, OBS_ALL, "plain"),
)


def case_id(case):
    kind, dyn, f32, dims, N, T, mode, eps, t0, obs_mode, head = case
    return "%dd_%s_%s_%s_N%d_T%d_m%d_%s_t%d_o%d_%s" % (kind, "dyn" if dyn else "sta", "f32" if f32 else "f64", "x".join(map(str, dims)), N, T, mode,
                                                        eps, t0 & 0xFF, obs_mode, head)


def case_seed(case):
    kind, dyn, f32, dims, N, T, mode, eps, t0, obs_mode, head = case
    return 7000 * kind + 100 * sum(dims) + 13 * N + T + 3 * mode + HEADS.index(head) + (t0 & 0xFF)


_made = {}


def make_rollout_case(case, base=0):
    """dict(weights, biases, eps (a number or float32 [N]), table, cells, seed, want: rollout_rule's result from the start state, state:
    the oracle afterwards) of a case, made once and left unchanged."""
    key = (case, base)
    if key in _made:
        return _made[key]
    kind, dyn, f32, dims, N, T, mode, eps, t0, obs_mode, head = case
    rng = np.random.default_rng(case_seed(case))
    weights, biases = make_net(rng, dims, ACTIONS[kind], head)
    if isinstance(eps, str):                                         # per env, by global id
        eps = np.array([0.0, 0.05, 0.4, 1.0], np.float32)[(base + np.arange(N)) % 4]
    table = plan_table(kind, dyn)
    seed = 3 + kind
    orc = helpers.oracle().OracleBatch(kind, dyn, N, table, seed=seed, env_id_base=base)
    orc.set_total_step(TOTAL_STEP)
    start(orc, N, base)
    cells = plan_cells(kind, table)
    want = rollout_rule(orc, cells, weights, biases, T, t0, mode, eps, seed, base)
    _made[key] = dict(weights=weights, biases=biases, eps=eps, table=table, cells=cells, seed=seed, want=want, orc=orc)
    return _made[key]


def test_the_generated_cases_contain_every_sort_of_tick():
    reset_first = reset_later = masked = bad = explore = greedy = value_inf = plan_in = False
    drawn = {1: set(), 2: set(), 3: set()}
    for case in CASES:
        kind, dyn, f32, dims, N, T, mode, eps, t0, obs_mode, head = case
        A = ACTIONS[kind]
        c = make_rollout_case(case)
        w = c["want"]
        assert w["actions"].min() >= 0 and w["actions"].max() < A
        drawn[kind] |= set(w["actions"].ravel().tolist())
        reset_first |= bool(w["reset"][0].any()) and not bool(w["reset"][0].all())
        reset_later |= bool(w["reset"][1:].any())
        plan_in |= dims[0] != OBS_DIM[kind]
        if head == "masked":
            a = int(np.flatnonzero(np.isneginf(c["biases"][-1][:A]))[0])
            assert np.isneginf(w["scores"][:, :, a]).all()
            chosen = w["actions"] == a                               # a masked action is never the policy's choice: only exploration draws it
            assert not (chosen[~w["explore"]] if mode == EPS_GREEDY else chosen).any()
            masked = True
        if head in ("bad_nan", "bad_inf"):
            assert w["bad_rows"] == T * N                            # counted, and drawn as all-zero scores
            zero = policy_rule(c["seed"], np.arange(N, dtype=np.uint64), t0, mode, np.zeros((N, A), np.float32), 0.0)
            assert w["actions"][0].tobytes() == zero["action"].tobytes()
            if mode == CATEGORICAL:
                assert w["logp"][0].tobytes() == zero["logp"].tobytes() and np.allclose(w["entropy"], np.log(A), atol=1e-6)
            bad = True
        else:
            assert w["bad_rows"] == 0
        if head == "value_inf":
            assert np.isposinf(w["value"]).all() and w["bad_rows"] == 0
            value_inf = True
        elif w["value"] is not None:
            assert np.isfinite(w["value"]).all()
        if mode == EPS_GREEDY:
            explore |= bool(w["explore"].any())
            greedy |= bool((~w["explore"]).any())
        assert (w["first"] != 0)[w["reset"]].all()                   # a reset tick is the first step of its episode
        assert w["done"].any() or T < 3
    assert reset_first and reset_later and masked and bad and explore and greedy and value_inf and plan_in
    assert all(drawn[kind] == set(range(ACTIONS[kind])) for kind in drawn), drawn


def test_the_rule_is_the_composition_it_states_and_repeats_itself():
    """One case by hand: a tick of rollout_rule is a masked reset, the rows, the network, the draw and a step with that action."""
    case = CASES[5]
    kind, dyn, f32, dims, N, T, mode, eps, t0, obs_mode, head = case
    c = make_rollout_case(case)
    orc = helpers.oracle().OracleBatch(kind, dyn, N, c["table"], seed=c["seed"])
    orc.set_total_step(TOTAL_STEP)
    start(orc, N)
    assert orc.state()["need_reset"].tolist() == [int(i % 3 != 0) for i in range(N)]
    again = rollout_rule(orc, c["cells"], c["weights"], c["biases"], T, t0, mode, c["eps"], c["seed"])
    for k, v in c["want"].items():
        assert (v == again[k]) if not isinstance(v, np.ndarray) else v.tobytes() == again[k].tobytes(), k
    for k, v in c["orc"].state().items():
        assert np.array_equal(v, orc.state()[k]), k
    w = c["want"]
    assert (w["step_size"] >= 1).all() and (w["step_size"] <= 3).all()
    assert (w["reset"][1:] == (w["done"][:-1] != 0)).all()           # an env that finished resets at the next tick


# ---- the C entry point -------------------------------------------------------------------------------------------------------------------
def _desc(kind=2, dynamic=1, N=16, obs_dtype=0, **kw):
    d = _lib.EnvDesc(kind, dynamic, N, 4, obs_dtype, 0, 1, 0, 0, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _state(**kw):
    s = _lib.State(*([1 << 20] * 8))
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _roll(L, desc=None, st=None, net=None, T=4, t0=0, mode=CATEGORICAL, epsilon=0.0, eps_env=None, obs_mode=OBS_ALL, obs=PH, reward=PH, done=PH,
          rec=None, value=PH, logp=PH, entropy=PH, bad=PH, no_desc=False, no_net=False):
    d = desc if desc is not None else _desc()
    s = st if st is not None else _state()
    n = net if net is not None else _net((51, 64, 6))
    return L.snac_policy_rollout(None if no_desc else C.byref(d), C.byref(s), None if no_net else C.byref(n), T, t0, mode, epsilon, eps_env,
                                 obs_mode, obs, reward, done, C.byref(rec) if rec is not None else None, value, logp, entropy, bad, None)


def test_the_library_exports_the_entry_point():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    vp = C.c_void_p
    want = [C.POINTER(_lib.EnvDesc), C.POINTER(_lib.State), C.POINTER(_lib.Mlp), C.c_int32, C.c_uint32, C.c_int32, C.c_double, vp, C.c_int, vp, vp,
            vp, C.POINTER(_lib.RolloutRecord), vp, vp, vp, vp, vp]
    assert "snac_policy_rollout" in _lib.EXPORTS and _lib.PROTOTYPES["snac_policy_rollout"] == (C.c_int, want)
    assert L.snac_policy_rollout.argtypes == want
    assert C.sizeof(_lib.Mlp) == 88                                  # snac_mlp keeps its layout


def test_policy_rollout_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    odd2, odd4, odd8 = C.c_void_p((1 << 20) + 1), C.c_void_p((1 << 20) + 2), C.c_void_p((1 << 20) + 4)
    _err(L, _roll(L, no_desc=True), -1, b"null desc/state")
    for kind in (0, 4):
        _err(L, _roll(L, _desc(kind=kind)), -1, b"unknown env kind")
    _err(L, _roll(L, _desc(N=0)), -1, b"num_envs must be positive")
    _err(L, _roll(L, st=_state(grid=0)), -1, b"null pointer in snac_state")
    _err(L, _roll(L, st=_state(hdr=(1 << 20) + 8)), -1, b"snac_state.hdr must be 16-byte aligned")
    # the network: mlp_check's pieces
    _err(L, _roll(L, no_net=True), -1, b"null net")
    _err(L, _roll(L, net=_net(layers=5)), -1, b"layers must be 1 .. 4")
    _err(L, _roll(L, net=_net((51, 257, 6))), -1, b"a hidden width must be 1 .. 256")
    _err(L, _roll(L, net=_net(w=[1 << 20, 0])), -1, b"null weights / bias")
    _err(L, _roll(L, net=_net(b=[(1 << 20) + 2, 1 << 20])), -1, b"4-byte aligned")
    for T in (0, -1, -(1 << 31)):
        _err(L, _roll(L, T=T), -1, b"T must be >= 1")
    # mode and epsilon as snac_policy_act
    for mode in (-1, 3, 100):
        _err(L, _roll(L, mode=mode), -1, b"mode must be")
    for eps in (float("nan"), float("inf"), -0.001, 1.001):
        for mode in (CATEGORICAL, GREEDY, EPS_GREEDY):
            _err(L, _roll(L, mode=mode, epsilon=eps, logp=None, entropy=None), -1, b"epsilon must be finite and in [0, 1]")
    for mode in (CATEGORICAL, GREEDY):
        _err(L, _roll(L, mode=mode, eps_env=PH, logp=None, entropy=None), -1, b"epsilon_per_env belongs to")
    for mode in (GREEDY, EPS_GREEDY):
        _err(L, _roll(L, mode=mode, entropy=None), -1, b"categorical mode only")
        _err(L, _roll(L, mode=mode, logp=None), -1, b"categorical mode only")
    # the rows
    _err(L, _roll(L, obs_mode=OBS_TILED), -3, b"SNAC_OBS_TILED")
    for m in (-1, 4):
        _err(L, _roll(L, obs_mode=m), -1, b"unknown obs_mode")
    for m in (OBS_ALL, OBS_LAST):
        _err(L, _roll(L, obs_mode=m, obs=None), -1, b"obs_mode set but obs is null")
    for kw in (dict(obs_tail=_lib.TAIL_PLAN), dict(obs_tail=_lib.TAIL_POSITION), dict(obs_tail=_lib.TAIL_RECORD), dict(frame_value=2),
               dict(obs_scalars=_lib.SCALARS_RAW)):
        _err(L, _roll(L, _desc(**kw)), -3, b"canonical observation layout only")
    _err(L, _roll(L, _desc(dynamic=0, obs_scalars=_lib.SCALARS_NORM)), -3, b"canonical observation layout only")
    # the network's ends against the kind
    for kind, dims in ((2, (50, 64, 6)), (2, (52, 6)), (2, (450, 64, 6)), (1, (51, 4)), (1, (36, 4)), (3, (37, 9)), (3, (452, 9))):
        _err(L, _roll(L, _desc(kind=kind), net=_net(dims)), -1, b"dim[0] must be obs_dim")
    for kind, dims in ((2, (51, 64, 4)), (2, (51, 7)), (1, (7, 5)), (1, (37, 2)), (3, (51, 7)), (3, (451, 10))):
        _err(L, _roll(L, _desc(kind=kind), net=_net(dims)), -1, b"dim[layers] must be num_actions")
    for kind, dims in ((2, (51, 64, 5)), (1, (37, 3)), (3, (451, 8, 8))):
        _err(L, _roll(L, _desc(kind=kind), net=_net(dims)), -1, b"value needs dim[layers] == num_actions + 1")
    # alignment: every array as its element type
    _err(L, _roll(L, obs=odd4), -1, b"obs must be aligned")           # float64 rows
    _err(L, _roll(L, _desc(obs_dtype=1), obs=odd2), -1, b"obs must be aligned")
    _err(L, _roll(L, mode=EPS_GREEDY, eps_env=odd4, logp=None, entropy=None), -1, b"epsilon_per_env must be 4-byte aligned")
    for k in ("reward", "value", "logp", "entropy", "bad"):
        _err(L, _roll(L, **{k: odd4}), -1, b"must be 4-byte aligned")
    _err(L, _roll(L, rec=_lib.RolloutRecord(None, None, (1 << 20) + 1, None)), -1, b"rec->plan_idx must be 2-byte aligned")
    # the checks come in the stated order whatever else is wrong
    _err(L, _roll(L, T=0, mode=9, obs=None), -1, b"T must be >= 1")


# ---- the Python methods ------------------------------------------------------------------------------------------------------------------
def _bare_env(kind=2, N=8, **kw):
    """A BatchedDMPEnv that never saw a device: the fields the argument checks read."""
    import torch
    from snac_amd import BatchedDMPEnv

    env = object.__new__(BatchedDMPEnv)
    env.kind, env.num_envs, env.num_actions, env.base_obs_dim, env.obs_dim = kind, N, ACTIONS[kind], OBS_DIM[kind], OBS_DIM[kind]
    env.frame_value, env.obs_scalars, env.obs_tail, env.device, env._was_reset = -1, None, 0, torch.device("cuda", 0), False
    for k, v in kw.items():
        setattr(env, k, v)
    return env


def _bare_mlp(dims, device="cuda:0"):
    import torch
    from snac_amd import DeviceMLP

    net = object.__new__(DeviceMLP)
    net.dims, net.device, net.num_actions = tuple(dims), torch.device(device), None
    return net


def test_rollout_policy_refuses_bad_arguments_before_it_touches_a_device():
    import torch

    env, net = _bare_env(), _bare_mlp((51, 64, 6))
    plan = lambda **kw: env._rollout_policy_plan(*[kw.get(k, v) for k, v in (("net", net), ("T", 4), ("mode", "categorical"), ("epsilon", 0.0), ("obs", "all"),
                                                                          ("want_value", None), ("want_logp", None), ("want_entropy", False),
                                                                          ("record", False), ("out", None))])
    T, mode, eps, eps_env, obs_mode, names = plan()
    assert (T, mode, eps, eps_env, obs_mode) == (4, CATEGORICAL, 0.0, None, OBS_ALL) and names == {"obs", "reward", "done", "value", "logp"}
    assert plan(net=_bare_mlp((451, 8, 5)), mode="greedy", obs=None, record=True)[5] == {"reward", "done", "actions", "step_size", "plan_idx", "first"}
    per_env = torch.zeros(8)
    assert plan(mode="eps_greedy", epsilon=per_env)[2:4] == (0.0, per_env) and plan(mode="eps_greedy", epsilon=0.25)[1:3] == (EPS_GREEDY, 0.25)
    for kw, words in ((dict(net=torch.nn.Linear(51, 6)), "net must be a DeviceMLP"), (dict(T=0), "T must be an integer >= 1"),
                      (dict(T=2.0), "T must be"), (dict(T=True), "T must be"), (dict(mode="softmax"), "mode must be"),
                      (dict(net=_bare_mlp((52, 6))), "input width must be obs_dim = 51"), (dict(net=_bare_mlp((51, 4))), "num_actions = 5 outputs"),
                      (dict(net=_bare_mlp((51, 6), "cuda:1")), "on the env's device"), (dict(epsilon=1.5), "epsilon must be a number in"),
                      (dict(epsilon=True), "epsilon must be"), (dict(epsilon=per_env), "per-env epsilons belong to"),
                      (dict(mode="eps_greedy", epsilon=torch.zeros(9)), "one value per env"), (dict(obs="tiled"), "obs must be"),
                      (dict(want_value=1), "want_value must be None or a bool"), (dict(want_entropy=None), "must be bools"),
                      (dict(net=_bare_mlp((51, 5)), want_value=True), "want_value needs a network"),
                      (dict(mode="greedy", want_logp=True), "categorical"), (dict(mode="eps_greedy", want_entropy=True), "categorical"),
                      (dict(out=[1]), "out must be a dict"), (dict(out=dict(rewards=None)), "out must be a dict"),
                      (dict(obs=None, out=dict(obs=None)), "needs obs="), (dict(mode="greedy", out=dict(logp=None)), "does not define")):
        with pytest.raises(ValueError, match=words):
            plan(**kw)
    for bad in (dict(obs_dim=451), dict(frame_value=2), dict(obs_scalars="raw")):
        with pytest.raises(ValueError, match="canonical observation layout only"):
            _bare_env(**bad)._rollout_policy_plan(net, 4, "categorical", 0.0, "all", None, None, False, False, None)
    with pytest.raises(_lib.SnacError, match="before reset"):
        env.rollout_policy(net, 4)


def test_collect_policy_refuses_bad_arguments_before_it_touches_a_device():
    from snac_amd import ReplayRing, RolloutBuffer

    ring = object.__new__(ReplayRing)
    ring.tiled, ring.cap, ring.env, ring._env_t = True, 8, _bare_env(t=3), 3
    net = _bare_mlp((51, 64, 5))
    with pytest.raises(ValueError, match="layout='ticks'"):
        ring.collect_policy(net, 4)
    ring.tiled = False
    for T, words in ((0, "T must be"), (2.5, "T must be"), (9, "exceeds the ring capacity")):
        with pytest.raises(ValueError, match=words):
            ring.collect_policy(net, T)
    ring._env_t = 2
    with pytest.raises(_lib.SnacError, match="stepped outside the ring"):
        ring.collect_policy(net, 4)
    buf = object.__new__(RolloutBuffer)
    buf.env, buf.ring = ring.env, ring
    for bad in (net, "net", None):
        with pytest.raises(ValueError, match="actor-critic"):
            buf.collect_policy(bad, 4)
