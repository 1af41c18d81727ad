"""Host: snac_policy_act is exported and checks every argument before any HIP call -- each failing call below fails its checks first, so the
placeholder pointers are never dereferenced, and a call with no output returns 0 although no device exists to launch on.  Then the rule as
include/snac_hip.h states it ("Acting from a policy"), in numpy, independently of the kernel (tests/test_gpu_policy_act.py compares the
kernel with it byte for byte): EXP and LOG as the header's sequences of float64 operations against math.exp / math.log, the integer
weights, and the draws of the categorical and the epsilon-greedy mode against their exact probabilities."""
import ctypes as C
import math

import numpy as np
import pytest

from cabi_checks import PH, _err
import rng_spec
from snac_amd import _lib
from specmath import spec_exp, spec_log

CATEGORICAL, GREEDY, EPS_GREEDY = 0, 1, 2
STREAM_POLICY = 5
ACTIONS = {1: 3, 2: 5, 3: 8}                                         # num_actions of the three kinds
# the fixed seed of the two statistical checks below: both statistics stay below their 99.9 % quantiles for it (the draws are a pure
# function of the seed, so the checks are deterministic; about one seed in a thousand would miss each)
STAT_SEED = 20261020


# ---- the rule, in numpy: every ufunc call below is one float64 operation, rounded on its own --------------------------------------------
def weights_of(scores):
    """(bad [N] bool, greedy [N], x [N, A] float64, e [N, A] float64, w [N, A] uint64) of float32 rows, bad rows taken as all zeros."""
    s = np.array(scores, np.float32, ndmin=2)
    m = s[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for a in range(1, s.shape[1]):
            m = np.where(s[:, a] > m, s[:, a], m)
        bad = np.isnan(s).any(axis=1) | (s == np.inf).any(axis=1) | (m == -np.inf)
        s[bad], m[bad] = 0.0, 0.0
        greedy = np.argmax(s == m[:, None], axis=1)                  # the lowest index of the largest score
        x = s.astype(np.float64) - m.astype(np.float64)[:, None]
    e = spec_exp(x)
    return bad, greedy, x, e, np.floor(e * 268435456.0).astype(np.uint64)


def eps_fx_of(eps):
    with np.errstate(invalid="ignore"):
        v = np.floor(np.asarray(eps).astype(np.float64) * 65536.0)
        return np.where(v >= 65536.0, 65536, np.where(v > 0.0, v, 0.0)).astype(np.uint64)


def policy_rule(seed, env_ids, t, mode, scores, eps=0.0):
    """-> dict(action int8 [N], logp / entropy float32 [N] (categorical only, else None), bad_rows int).  eps: a number, or float32 [N]."""
    env_ids = np.asarray(env_ids, np.uint64)
    w = rng_spec.words(seed, STREAM_POLICY, env_ids, np.uint64(int(t) & 0xFFFFFFFF))
    bad, greedy, x, e, wt = weights_of(scores)
    N, A = x.shape
    assert env_ids.shape == (N,)
    out = dict(logp=None, entropy=None, bad_rows=int(bad.sum()))
    if mode == GREEDY:
        action = greedy
    elif mode == EPS_GREEDY:
        eps_fx = eps_fx_of(np.float32(eps) if np.ndim(eps) else np.float64(eps))
        explore = (w >> np.uint64(16)) < eps_fx
        action = np.where(explore, ((w & np.uint64(0xFFFF)) * np.uint64(A)) >> np.uint64(16), greedy)
    else:
        total = wt.sum(axis=1)
        assert total.max() <= 1 << 31
        u = (w * total) >> np.uint64(32)
        action = (np.cumsum(wt, axis=1) > u[:, None]).argmax(axis=1)     # the lowest a whose running sum passes u
        S, T = np.zeros(N), np.zeros(N)
        with np.errstate(invalid="ignore"):
            for a in range(A):
                S = S + e[:, a]
                T = T + np.where(e[:, a] == 0.0, 0.0, e[:, a] * x[:, a])
        L = spec_log(S)
        out["logp"] = (x[np.arange(N), action] - L).astype(np.float32)
        out["entropy"] = (L - T / S).astype(np.float32)
    out["action"] = np.asarray(action).astype(np.int8)
    return out


# the score rows of tests/test_gpu_policy_act.py: eight sorts of row taking turns, row i of sort (i + shift) % 8
SORTS = ("normal", "equal", "one_masked", "several_masked", "spread", "nan", "plus_inf", "all_masked")


def make_scores(rng, N, A, shift=0):
    s = (3.0 * rng.normal(size=(N, A))).astype(np.float32)
    for i in range(N):
        sort = SORTS[(i + shift) % 8]
        if sort == "equal":
            s[i] = s[i, 0]
        elif sort == "one_masked":
            s[i, rng.integers(A)] = -np.inf
        elif sort == "several_masked":
            s[i, rng.choice(A, size=2 if A == 3 else A - 2, replace=False)] = -np.inf
        elif sort == "spread":
            s[i] = rng.uniform(-50.0, 50.0, size=A).astype(np.float32)
        elif sort == "nan":
            s[i, rng.integers(A)] = np.nan
        elif sort == "plus_inf":
            s[i, rng.integers(A)] = np.inf
        elif sort == "all_masked":
            s[i] = -np.inf
    return s


def bad_rows_of(N, shift=0):
    return sum(SORTS[(i + shift) % 8] in ("nan", "plus_inf", "all_masked") for i in range(N))


# ---- EXP, LOG and the weights ------------------------------------------------------------------------------------------------------------
def test_exp_and_log_stay_within_1e_12_of_the_exact_functions():
    x = np.concatenate([np.linspace(-45.0, 0.0, 200001), -np.logspace(-300, 1.65, 4001), [0.0, -0.0, -45.0, -math.log(2.0) / 2, -19.4]])
    got = spec_exp(x)
    assert max(abs(float(g) - math.exp(float(v))) for g, v in zip(got, x)) <= 1e-12
    assert np.all(got[x == 0.0] == 1.0) and np.all(got <= 1.0) and np.all(got > 0.0)
    assert np.array_equal(spec_exp([-45.000001, -100.0, -np.inf]), [0.0, 0.0, 0.0])
    s = np.concatenate([np.linspace(1.0, 8.0, 200001), [1.0, 2.0, 4.0, 8.0, math.sqrt(2.0), np.nextafter(math.sqrt(2.0), 0.0), 2.0 * math.sqrt(2.0)]])
    got = spec_log(s)
    assert max(abs(float(g) - math.log(float(v))) for g, v in zip(got, s)) <= 1e-12
    assert spec_log(1.0) == 0.0


def test_the_largest_score_weighs_exactly_2_to_the_28_and_a_far_or_masked_one_nothing():
    rows = np.array([[0.5, -np.inf, 0.5 - 20.0, 0.5, 0.25], [-3.0, -3.0, -3.0, -3.0, -3.0], [7.0, 7.0 - 19.0, -50.0, 50.0, 0.0]], np.float32)
    bad, greedy, x, e, w = weights_of(rows)
    assert not bad.any() and greedy.tolist() == [0, 0, 3]
    assert w[0].tolist()[:4] == [1 << 28, 0, 0, 1 << 28] and 0 < w[0, 4] < 1 << 28
    assert w[1].tolist() == [1 << 28] * 5
    assert w[2, 3] == 1 << 28 and w[2].sum() == 1 << 28              # 43, 62, 100 and 50 below the largest: nothing
    assert weights_of(np.array([[0.0, -19.0]], np.float32))[4][0, 1] > 0      # 19 below still has a weight
    for A in ACTIONS.values():                                       # never past 2^31, reached by A = 8 equal scores
        assert weights_of(np.zeros((1, A), np.float32))[4].sum() == A << 28 <= 1 << 31
    # bad rows are drawn as all zeros: uniform weights, greedy action 0
    bad, greedy, x, e, w = weights_of(np.array([[1.0, np.nan, 0.0], [np.inf, 0.0, 0.0], [-np.inf] * 3, [-np.inf, 2.0, -np.inf]], np.float32))
    assert bad.tolist() == [True, True, True, False] and greedy.tolist() == [0, 0, 0, 1]
    assert w[:3].tolist() == [[1 << 28] * 3] * 3 and w[3].tolist() == [0, 1 << 28, 0]


def test_the_rows_of_the_gpu_test_contain_every_sort():
    for A in ACTIONS.values():
        s = make_scores(np.random.default_rng(A), 64, A)
        bad, greedy, x, e, w = weights_of(s)
        assert bad.sum() == bad_rows_of(64) == 24 and bad_rows_of(1, 5) == 1 and bad_rows_of(1, 0) == 0
        assert (w[~bad] == 0).any() and ((w[~bad] > 0) & (w[~bad] < 1 << 28)).any() and np.isneginf(s[~bad]).any()
        ties = ((s == s.max(axis=1, keepdims=True)).sum(axis=1) > 1) & ~bad
        assert ties.any() and (greedy[ties] == 0).all()
        out = policy_rule(1, np.arange(64), 0, CATEGORICAL, s)
        assert np.isfinite(out["logp"]).all() and np.isfinite(out["entropy"]).all() and (out["entropy"] >= 0).all()
        assert (w[np.arange(64), out["action"]] > 0).all()           # an action of weight 0 is never drawn
        assert np.allclose(out["entropy"][bad], math.log(A)) and np.allclose(out["logp"][bad], -math.log(A))


# ---- the draws against their exact probabilities -----------------------------------------------------------------------------------------
def test_categorical_draws_follow_the_weight_ratios():
    row = np.array([0.3, -1.2, 2.0, 0.0, -4.0, 1.1, -0.5, 0.7], np.float32)
    n = 65536
    out = policy_rule(STAT_SEED, np.arange(n), 7, CATEGORICAL, np.tile(row, (n, 1)))
    w = weights_of(row)[4][0].astype(np.float64)
    expect = n * w / w.sum()
    count = np.bincount(out["action"], minlength=8)
    chi2 = float(((count - expect) ** 2 / expect).sum())
    assert chi2 < 24.322, (chi2, count.tolist())                     # the 99.9 % quantile of chi-square with 7 degrees of freedom
    p = w / w.sum()
    assert np.allclose(out["logp"], np.log(p)[out["action"]], atol=1e-6) and np.allclose(out["entropy"], -(p * np.log(p)).sum(), atol=1e-6)


@pytest.mark.parametrize("eps", [0.25, 0.0123])
def test_epsilon_greedy_explores_its_share(eps):
    n, A = 65536, 5
    q = np.tile(np.array([0.0, 1.0, 5.0, 5.0, -1.0], np.float32), (n, 1))
    out = policy_rule(STAT_SEED, np.arange(n), 3, EPS_GREEDY, q, eps)
    w = rng_spec.words(STAT_SEED, STREAM_POLICY, np.arange(n, dtype=np.uint64), np.uint64(3))
    p = int(eps_fx_of(eps)) / 65536.0
    assert int(eps_fx_of(eps)) == math.floor(eps * 65536)
    explored = int(((w >> np.uint64(16)) < eps_fx_of(eps)).sum())
    chi2 = (explored - n * p) ** 2 / (n * p) + ((n - explored) - n * (1 - p)) ** 2 / (n * (1 - p))
    assert chi2 < 10.828, (chi2, explored)                           # the 99.9 % quantile of chi-square with 1 degree of freedom
    assert set(np.unique(out["action"])) == set(range(A)) and (out["action"] == 2).sum() >= n - explored   # greedy: the lowest of the tie
    assert (policy_rule(STAT_SEED, np.arange(n), 3, EPS_GREEDY, q, 0.0)["action"] == 2).all()
    if eps == 0.25:                                                  # exact in float32: the per-env form draws the same actions
        assert np.array_equal(policy_rule(STAT_SEED, np.arange(n), 3, EPS_GREEDY, q, np.full(n, eps, np.float32))["action"], out["action"])
    assert eps_fx_of(np.array([np.nan, -1.0, 2.0, 1.0], np.float32)).tolist() == [0, 0, 65536, 65536]


# ---- the C entry point -------------------------------------------------------------------------------------------------------------------
def _desc(kind=2, seed=1, base=0):
    return _lib.EnvDesc(kind, 1, 16, 4, 0, 0, seed, base, 0, 0, 0, 0, 0, 0)


def _act(L, desc=True, kind=2, N=4, t=0, mode=CATEGORICAL, scores=PH, epsilon=0.0, eps_env=None, action=PH, logp=None, entropy=None, bad=PH):
    d = _desc(kind)
    return L.snac_policy_act(C.byref(d) if desc else None, N, t, mode, scores, epsilon, eps_env, action, logp, entropy, bad, None)


def test_the_library_exports_the_entry_point():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    assert "snac_policy_act" in _lib.EXPORTS and len(L.snac_policy_act.argtypes) == 12
    assert _lib.PROTOTYPES["snac_policy_act"][1][2:4] == [C.c_uint32, C.c_int32] and _lib.PROTOTYPES["snac_policy_act"][1][5] == C.c_double
    assert (_lib.POLICY_CATEGORICAL, _lib.POLICY_GREEDY, _lib.POLICY_EPS_GREEDY) == (CATEGORICAL, GREEDY, EPS_GREEDY)


def test_policy_act_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _err(L, _act(L, desc=False), b"null desc/scores")
    _err(L, _act(L, scores=None), b"null desc/scores")
    for kind in (0, 4, -1):
        _err(L, _act(L, kind=kind), b"unknown env kind")
    for N in (0, -1):
        _err(L, _act(L, N=N), b"N must be")
    for mode in (-1, 3, 100):
        _err(L, _act(L, mode=mode), b"mode must be")
    for eps in (float("nan"), float("inf"), float("-inf"), -0.001, 1.001):
        for mode in (CATEGORICAL, GREEDY, EPS_GREEDY):
            _err(L, _act(L, mode=mode, epsilon=eps), b"epsilon must be finite and in [0, 1]")
    for mode in (CATEGORICAL, GREEDY):
        _err(L, _act(L, mode=mode, eps_env=PH), b"epsilon_per_env belongs to")
    for mode in (GREEDY, EPS_GREEDY):
        _err(L, _act(L, mode=mode, logp=PH), b"categorical mode only")
        _err(L, _act(L, mode=mode, entropy=PH), b"categorical mode only")
    # no output: no launch -- but the checks come first
    for mode in (CATEGORICAL, GREEDY, EPS_GREEDY):
        for kind in (1, 2, 3):
            assert _act(L, kind=kind, mode=mode, action=None, epsilon=1.0 if mode == EPS_GREEDY else 0.0) == 0
    assert _act(L, mode=EPS_GREEDY, action=None, eps_env=PH, bad=None, t=0xFFFFFFFF) == 0
    _err(L, _act(L, action=None, N=0), b"N must be")
    _err(L, _act(L, action=None, scores=None), b"null desc/scores")
