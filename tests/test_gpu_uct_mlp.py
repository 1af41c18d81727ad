"""GPU: the PUCT search with its network on the device.

UCTSearch(evaluator=DeviceMLP) values its leaves in one fused launch (snac_mlp_uct_value_leaves); UCTSearch(evaluator=lambda o:
mlp.policy_value(o)) is the generic path on the same network -- the evaluator's launch, then the torch operations of _value_leaves().
On twin envs both must leave the same bytes: the statistics rows, the node records, the roots' visits, q and priors and the network
values, after run() and after an advance(); for the three kinds, 3 and 65 trees of 64 nodes, 1 and 4 paths, plain PUCT, normalised q,
the Gumbel root search and the Gumbel rule below the root.  Then the fused entry point alone through the C ABI on constructed slots --
terminal and non-terminal leaves of both kinds, indices outside their ranges, bad rows -- against numpy (leaves_rule of
tests/test_mlp_host.py) in a guard arena, and the example with --device-evaluator."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from devmem import _env, _vp
import guard
import helpers
from specmath import _same
from test_gpu_mlp import PlacedNet
from test_mlp_host import bad_rows_of, case_seed, leaves_rule, make_leaves, make_mlp_case, rule_of

pytestmark = pytest.mark.gpu

GAMMA, CPUCT, VL, CAP, ITERS = 0.99, 1.25, 0.5, 64, 6
MODES = dict(puct=dict(), norm=dict(q_normalise=True), gumbel=dict(q_normalise=True, gumbel=2),
             interior=dict(q_normalise=True, gumbel=2, gumbel_interior=True))


def _net(env, seed):
    import torch

    torch.manual_seed(seed)
    A = env.num_actions
    return torch.nn.Sequential(torch.nn.Linear(env.obs_dim, 32), torch.nn.ReLU(), torch.nn.Linear(32, A + 1)).to(env.device)


def _run(search, n):
    if search.gumbel is None:
        search.run(n)
        return
    search.gumbel_begin(search.gumbel_scores(noise=False))
    search.gumbel_run(n)


def _same_search(a, b, what):
    import torch

    torch.cuda.synchronize()
    assert torch.equal(a.stats, b.stats), (what, "stats")            # int32 words: equal values are equal bytes
    assert torch.equal(a.pool.records, b.pool.records), (what, "node records")
    assert torch.equal(a.root_visits(), b.root_visits()) and torch.equal(a.tree_sizes(), b.tree_sizes()), (what, "visits")
    for name, x, y in (("root_q", a.root_q(), b.root_q()), ("root_priors", a.root_priors(), b.root_priors()), ("net_values", a.net_values, b.net_values),
                       ("est", a._est, b._est), ("value", a._value, b._value), ("priors", a._priors, b._priors)):
        assert x.contiguous().cpu().numpy().tobytes() == y.contiguous().cpu().numpy().tobytes(), (what, name)
    if a.q_bounds is not None:
        assert a.q_bounds.cpu().numpy().tobytes() == b.q_bounds.cpu().numpy().tobytes(), (what, "q_bounds")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B,K", [(3, 1), (3, 4), (65, 1), (65, 4)])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_the_fused_search_equals_the_generic_path_on_twin_envs(kind, B, K, mode):
    import torch
    from snac_amd import DeviceMLP, UCTSearch, _lib

    envs = [_env(kind, True, B, seed=5) for _ in range(2)]
    net = _net(envs[0], 10 * kind + K)
    mlp = [DeviceMLP(net, e) for e in envs]
    kw = dict(c=CPUCT, max_iterations=4 * ITERS, paths=K, virtual_loss=VL if K > 1 else 0.0, **MODES[mode])
    fused = UCTSearch(envs[0], CAP, 0, GAMMA, evaluator=mlp[0], **kw)
    generic = UCTSearch(envs[1], CAP, 0, GAMMA, evaluator=lambda o: mlp[1].policy_value(o), **kw)
    assert fused._mlp is mlp[0] and generic._mlp is None
    for s in (fused, generic):
        s.reset()
        _run(s, ITERS)
    assert _lib.lib().snac_last_kernel() in (b"k_uct_set_priors", b"k_uct_set_priors_value")
    _same_search(fused, generic, (kind, B, K, mode, "run"))
    assert int(fused.root_visits().sum()) > 0 and float(fused._value.abs().sum()) > 0
    moves = fused.best_actions()
    ra, da = fused.advance(moves)
    rb, db = generic.advance(moves)
    assert torch.equal(ra, rb) and torch.equal(da, db)
    _same_search(fused, generic, (kind, B, K, mode, "advance"))
    for s in (fused, generic):
        _run(s, ITERS)
    _same_search(fused, generic, (kind, B, K, mode, "run after advance"))
    assert int(mlp[0].bad_rows.cpu()[0]) == int(mlp[1].bad_rows.cpu()[0]) == 0


def test_the_fused_launch_is_what_values_the_leaves():
    """Without the feature UCTSearch has no fused path: the launch behind _value_leaves() is snac_mlp_uct_value_leaves's."""
    from snac_amd import DeviceMLP, UCTSearch, _lib

    env = _env(2, True, 5, seed=2)
    mlp = DeviceMLP(_net(env, 1), env)
    search = UCTSearch(env, CAP, 0, GAMMA, c=CPUCT, max_iterations=8, evaluator=mlp)
    search.reset()
    search._select()
    search._edges()
    search._first_reward()
    search._observe_leaves()
    search._value_leaves()
    assert _lib.lib().snac_last_kernel() == b"k_mlp_value_leaves"
    with pytest.raises(ValueError, match="the DeviceMLP must be on"):
        UCTSearch(_env(1, True, 5, seed=2), CAP, 0, GAMMA, evaluator=mlp)


# ---- the fused entry point alone ---------------------------------------------------------------------------------------------------------
OUTPUTS = ("priors", "value", "est", "bad_rows")


def _leaves(case, lv, f64, offset, want=OUTPUTS):
    import torch
    from snac_amd import _lib

    p = PlacedNet(case, f64, offset)
    A, S = case["A"], p.rows
    dev = p.dev
    ins = {k: torch.from_numpy(np.ascontiguousarray(lv[k])).to(dev) for k in ("first_has", "first_idx", "done", "stats", "leaf")}
    before = {k: v.clone() for k, v in ins.items()}
    arena = guard.Arena(S * (4 * A + 16) + 64 + 6 * (guard.BAND + 1024), dev)
    off4, off8 = (4, 8) if offset else (0, 0)
    out = dict(priors=arena.carve((S, A), torch.float32, offset=off4, name="priors"), value=arena.carve((S,), torch.float64, offset=off8, name="value"),
               est=arena.carve((S,), torch.float64, offset=off8, name="est"), bad_rows=arena.carve((1,), torch.int32, offset=off4, name="bad_rows"))
    if "est" in want:
        out["est"].copy_(torch.from_numpy(lv["est"]))
    if "bad_rows" in want:
        out["bad_rows"].zero_()
    o = {k: _vp(out[k]) if k in want else None for k in OUTPUTS}
    L = _lib.lib()
    _lib.check(L.snac_mlp_uct_value_leaves(C.byref(p.net), A, _vp(p.x), p.f64, S, _vp(ins["first_has"]), _vp(ins["first_idx"]), _vp(ins["done"]),
                                           _vp(ins["stats"]), len(lv["stats"]), _vp(ins["leaf"]), o["priors"], o["value"], o["est"], o["bad_rows"],
                                           p.stream))
    if want:
        assert L.snac_last_kernel() == b"k_mlp_value_leaves"
    arena.check()
    for k in OUTPUTS:
        if k not in want:
            guard.view_untouched(out[k], k + " (NULL in the call)")
    p.unchanged()
    for k, v in ins.items():
        assert torch.equal(v, before[k]), k + " was written"
    return {k: (out[k].cpu().numpy() if k in want else None) for k in OUTPUTS}


@pytest.mark.parametrize("S", [1, 65, 257])
@pytest.mark.parametrize("dims,A", [((7, 4), 3), ((51, 64, 6), 5), ((51, 65, 1, 9), 8)], ids=["7x4", "51x64x6", "51x65x1x9"])
def test_the_fused_entry_point_equals_numpy_and_writes_nothing_else(dims, A, S):
    for shift in ((0, 4, 5) if S == 1 else (S % 8,)):                # a single slot: a good row and two bad ones
        rng = np.random.default_rng(case_seed(dims, S, shift) + 1)
        case = make_mlp_case(rng, dims, S, A, shift)
        want = rule_of(case)
        assert want["bad_rows"] == bad_rows_of(S, shift)
        lv = make_leaves(rng, S, 9)
        value, est = leaves_rule(want, **lv)
        if S > 1:                                                    # both kinds of leaf, terminal and not, and indices outside their ranges
            term = value == 0
            assert (term & ~want["bad"]).any() and (~term).any() and lv["first_has"].any() and not lv["first_has"].all()
            assert (lv["leaf"] < 0).any() and (lv["leaf"] >= 9).any() and want["bad"].any()
        first = None
        for f64, offset in ((0, False), (1, True)):
            got = _leaves(case, lv, f64, offset)
            _same(got["priors"], want["priors"], (dims, S, shift, "priors"))
            assert got["value"].tobytes() == value.tobytes() and got["est"].tobytes() == est.tobytes(), (dims, S, shift, f64)
            assert int(got["bad_rows"][0]) == want["bad_rows"]
            if first is not None:
                assert all(got[k].tobytes() == first[k].tobytes() for k in OUTPUTS)
            first = got
    for n, subset in enumerate([(), ("est",), ("value",), ("priors", "bad_rows"), ("value", "est")]):
        got = _leaves(case, lv, n % 2, bool(n % 2), want=subset)
        if "value" in subset:
            assert got["value"].tobytes() == value.tobytes()
        if "est" in subset:
            assert got["est"].tobytes() == est.tobytes()
        if "bad_rows" in subset:
            assert int(got["bad_rows"][0]) == want["bad_rows"]


# ---- the example -------------------------------------------------------------------------------------------------------------------------
def test_the_selfplay_example_trains_with_the_device_evaluator():
    spec = importlib.util.spec_from_file_location("alphazero_selfplay", os.path.join(helpers.ROOT, "examples", "alphazero_selfplay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    info = {}
    losses, play = mod.train(envs=16, steps=3, moves=2, iterations=4, device_evaluator=True, info=info)
    assert len(losses) == 3 and np.isfinite(losses).all() and info["evaluator_bad_rows"] == 0 and len(play) > 0
