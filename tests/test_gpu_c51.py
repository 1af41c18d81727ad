"""GPU: snac_c51_expect / snac_c51_project, CategoricalSupport and the distributional path of examples/dqn_batched.py.

Both kernels through the C ABI on the generated inputs of tests/test_c51_host.py (make_case: both ends exactly, beyond both ends, discounts
0, 1, 0.95^3 and 1.5, a tie at the top, a NaN in a p_select row, the three sorts of bad sample; that they contain every case is asserted
there, on the host), byte for byte against c51_rule, at batch sizes with a ragged wave and a ragged block, the three action counts and five
supports (K = 64 a full wave of atoms, K = 2 the smallest).  Every output is carved from a guard arena: nothing lands outside the outputs,
the inputs keep their bytes, a NULL output is not written and the others do not change; the inputs are also taken one float into a larger
tensor (a base aligned to 4 bytes only).  Where the rule gives a NaN (the expected value of a row that holds one) the kernel must give a
NaN too; which NaN is not part of the rule, so those four bytes are not compared.  Then repeatability, the Python surface and the example."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from devmem import _place_floats, _shifts, _vp, short_env
import guard
import helpers
from test_c51_host import ACTIONS, SORTS, SUPPORTS, bad_rows_of, c51_expect_rule, c51_rule, make_case

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257, 1031)                                # a wave takes 4 samples and a block 16: ragged waves and blocks, many blocks
OUTPUTS = ("a_star", "q_star", "bad_rows")


def _call(K, vmin, vmax, case, select=True, want=OUTPUTS, offset=False):
    """One snac_c51_project and two snac_c51_expect calls (of p_next and of p_select) with their outputs in a guard arena -> dict of numpy
    arrays (None where not asked for)."""
    import torch
    from snac_amd import _lib

    L, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    B, A, _ = case["p_next"].shape
    ins = {k: _place_floats(case[k], offset, dev) for k in ("p_next", "p_select", "ret", "discount")}
    before = {k: flat.clone() for k, (flat, _) in ins.items()}
    arena = guard.Arena(B * (4 * K + 5 + 8 * A) + 4 + 8 * (guard.BAND + 1024), dev)
    off4, off1 = (4, 1) if offset else (0, 0)
    out = dict(m=arena.carve((B, K), torch.float32, offset=off4, name="m"), a_star=arena.carve((B,), torch.int8, offset=off1, name="a_star"),
               q_star=arena.carve((B,), torch.float32, offset=off4, name="q_star"), bad_rows=arena.carve((1,), torch.int32, name="bad_rows"),
               q=arena.carve((B, A), torch.float32, offset=off4, name="q"), q_select=arena.carve((B, A), torch.float32, offset=off4, name="q_select"))
    if "bad_rows" in want:
        out["bad_rows"].zero_()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    v = {k: _vp(view) for k, (_, view) in ins.items()}
    _lib.check(L.snac_c51_project(B, A, K, vmin, vmax, v["p_next"], v["p_select"] if select else None, v["ret"], v["discount"], _vp(out["m"]),
                                  *[_vp(out[k]) if k in want else None for k in OUTPUTS], stream))
    assert L.snac_last_kernel() == b"k_c51_project"
    _lib.check(L.snac_c51_expect(B, A, K, vmin, vmax, v["p_next"], _vp(out["q"]), stream))
    _lib.check(L.snac_c51_expect(B, A, K, vmin, vmax, v["p_select"], _vp(out["q_select"]), stream))
    assert L.snac_last_kernel() == b"k_c51_expect"
    arena.check()
    for k in OUTPUTS:
        if k not in want:
            guard.view_untouched(out[k], k + " (NULL in the call)")
    for k, (flat, _) in ins.items():
        assert torch.equal(flat.view(torch.int32), before[k].view(torch.int32)), k + " was written"      # bytes: the rows hold NaNs
    return {k: (t.cpu().numpy() if k not in OUTPUTS or k in want else None) for k, t in out.items()}


def _same(got, want, what):
    """Byte for byte, but a NaN of the rule is any NaN."""
    for k, w in want.items():
        g = got[k]
        if g is None:
            continue
        if k == "bad_rows":
            assert int(g[0]) == w, (what, k, int(g[0]), w)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        if w.dtype == np.float32:
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan), (what, k, "NaNs")
            g, w = np.where(nan, np.float32(0), g), np.where(nan, np.float32(0), w)
        diff = np.nonzero((g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1)).any(axis=1))[0]
        assert diff.size == 0, (what, k, "first sample that differs", int(diff[0]), g[diff[0]], w[diff[0]])


def _want(case, vmin, vmax, select):
    w = c51_rule(case["p_next"], case["ret"], case["discount"], vmin, vmax, case["p_select"] if select else None)
    w["q_select"] = c51_expect_rule(case["p_select"], vmin, vmax).astype(np.float32)
    return w


# ---- the kernels against the rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("A", ACTIONS)
def test_both_kernels_equal_the_rule_byte_for_byte_and_write_nothing_else(A, B):
    for n, (K, vmin, vmax) in enumerate(SUPPORTS):
        for shift in _shifts(B, SORTS):
            case = make_case(np.random.default_rng(10000 * n + 100 * A + B + shift), B, A, K, vmin, vmax, shift)
            for select, offset in ((True, False), (True, True), (False, True)):
                want = _want(case, vmin, vmax, select)
                assert want["bad_rows"] == bad_rows_of(B, shift)
                got = _call(K, vmin, vmax, case, select, offset=offset)
                _same(got, want, (A, B, K, shift, select, offset))
                assert got["a_star"].min() >= 0 and got["a_star"].max() < A
        # any subset of the optional outputs: the ones left out are not written, the others do not change
        for subset in ((), ("a_star",), ("q_star",), ("bad_rows",), ("a_star", "bad_rows")):
            _same(_call(K, vmin, vmax, case, False, want=subset, offset=True), want, (A, B, K, subset))


def test_two_calls_on_the_same_inputs_give_the_same_bytes():
    for n, (K, vmin, vmax) in enumerate(SUPPORTS):
        case = make_case(np.random.default_rng(n), 1031, 8, K, vmin, vmax)
        first, second = (_call(K, vmin, vmax, case, offset=bool(j)) for j in range(2))
        for k in first:
            assert first[k].tobytes() == second[k].tobytes(), (K, k)


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", ACTIONS)
def test_categorical_support_follows_the_rule(A):
    import torch
    from snac_amd import CategoricalSupport

    from test_c51_host import support as support_of

    B, (K, vmin, vmax) = 257, SUPPORTS[0]
    dev = torch.device("cuda", torch.cuda.current_device())
    cs = CategoricalSupport(A, atoms=K, vmin=vmin, vmax=vmax, device=dev)
    assert cs.z.dtype == torch.float32 and cs.z.cpu().numpy().tobytes() == support_of(K, vmin, vmax)[1].astype(np.float32).tobytes()
    case = make_case(np.random.default_rng(A), B, A, K, vmin, vmax)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("p_next", "p_select", "ret", "discount")}
    want = _want(case, vmin, vmax, True)
    q = cs.expected(t["p_next"])
    _same(dict(q=q.cpu().numpy()), dict(q=want["q"]), "expected")
    q_out = torch.empty((B, A), dtype=torch.float32, device=dev)
    assert cs.expected(t["p_next"], out=q_out) is q_out and torch.equal(q_out, q)
    m, a_star, q_star = cs.project(t["p_next"], t["ret"], t["discount"], p_select=t["p_select"], want_q=True)
    got = dict(m=m.cpu().numpy(), a_star=a_star.cpu().numpy(), q_star=q_star.cpu().numpy(), bad_rows=cs.bad_rows.cpu().numpy())
    _same(got, {k: want[k] for k in got}, "project")
    m2, a2, q2 = cs.project(t["p_next"], t["ret"], t["discount"], want_action=False)          # the choice by p_next itself; no a_star, no q_star
    own = c51_rule(case["p_next"], case["ret"], case["discount"], vmin, vmax)
    assert a2 is None and q2 is None and m2.cpu().numpy().tobytes() == own["m"].tobytes()
    assert int(cs.bad_rows.cpu()[0]) == 2 * bad_rows_of(B)                                    # a counter: it adds up over the calls
    out = (torch.empty((B, K), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int8, device=dev), None)
    res = cs.project(t["p_next"], t["ret"], t["discount"], p_select=t["p_select"], out=out)
    assert res[0] is out[0] and res[1] is out[1] and res[2] is None and torch.equal(res[0], m) and torch.equal(res[1], a_star)
    with pytest.raises(ValueError, match="p_select must have shape"):
        cs.project(t["p_next"], t["ret"], t["discount"], p_select=t["p_select"][:-1])
    with pytest.raises(ValueError, match="ret must have shape"):
        cs.project(t["p_next"], t["ret"][:-1], t["discount"])
    with pytest.raises(ValueError, match="discount must be a contiguous torch.float32 tensor"):
        cs.project(t["p_next"], t["ret"], t["discount"].double())
    with pytest.raises(ValueError, match=r"out\[0\] must have shape"):
        cs.project(t["p_next"], t["ret"], t["discount"], out=(out[0][:-1], None, None))
    with pytest.raises(ValueError, match="p must be on"):
        cs.expected(t["p_next"].cpu())


def test_categorical_support_takes_an_envs_actions_device_and_stream():
    import torch
    from snac_amd import CategoricalSupport

    for kind, A in ((1, 3), (2, 5), (3, 8)):
        env, _ = short_env(kind, 65, True, seed=3)
        cs = CategoricalSupport(env, atoms=33, vmin=-100.0, vmax=300.0)
        assert cs.num_actions == env.num_actions == A and cs.device == env.device and cs.env is env
        case = make_case(np.random.default_rng(kind), 65, A, 33, -100.0, 300.0)
        q = cs.expected(torch.from_numpy(case["p_next"]).to(env.device))
        assert q.cpu().numpy().tobytes() == c51_expect_rule(case["p_next"], -100.0, 300.0).astype(np.float32).tobytes()
        action = env.epsilon_greedy(q, 0.0)                          # what the expected values are for
        assert action.cpu().numpy().tolist() == np.argmax(q.cpu().numpy(), axis=1).tolist()
        with pytest.raises(ValueError, match="device is the env's"):
            CategoricalSupport(env, device=env.device)


# ---- the example -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", [dict(), dict(prioritized=True), dict(n_step=3)], ids=["plain", "prioritized", "n_step"])
def test_the_dqn_example_trains_on_distributional_targets(how):
    spec = importlib.util.spec_from_file_location("dqn_batched", os.path.join(helpers.ROOT, "examples", "dqn_batched.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    info = {}
    losses, _ = mod.run(envs=256, ticks=6, batch=256, distributional=True, info=info, log=lambda line: None, **how)
    assert len(losses) == 6 and all(np.isfinite(losses)) and all(x > 0 for x in losses)
    assert info["bad_rows"] == 0
