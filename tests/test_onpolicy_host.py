"""Host: snac_gae and snac_replay_gather_onpolicy are exported and check every argument before any HIP call -- each failing call below
fails its checks first, so the placeholder pointers are never dereferenced, and an empty span or batch returns 0 although no device exists
to launch on -- and RolloutBuffer rejects bad arguments on an object that was never built on a device.  Last, the two rules as
include/snac_hip.h states them ("On-policy rollouts"), in numpy, independently of the kernels (tests/test_gpu_onpolicy.py compares the
kernels with them): the spans that the GPU test uses contain every case that can go wrong, and the rule has its exact identities."""
import ctypes as C

import numpy as np
import pytest

from cabi_checks import ODD, PH, _err, _NoDevice
from snac_amd import _lib
from test_replay_nstep_host import gather_rule, ring_desc


def _gae(L, N=4, cap=8, first=0, count=8, gamma=0.97, lam=0.95, reward=PH, done=PH, value=PH, boot=PH, adv=PH, ret=PH):
    return L.snac_gae(N, cap, first, count, gamma, lam, reward, done, value, boot, adv, ret, None)


def _gather(L, desc=True, st=True, kind=2, tail=0, cap=8, tiled=0, obs=PH, first=PH, plan_idx=PH, action=PH, value=PH, logp=PH, adv=PH, ret=PH,
            norm=PH, tick=PH, env=PH, batch=4, s=PH, plan=PH, action_out=PH, value_out=PH, logp_out=PH, adv_out=PH, ret_out=PH):
    d, state = ring_desc(kind, tail), _lib.State(*[1 << 20] * 8)  # never dereferenced
    return L.snac_replay_gather_onpolicy(C.byref(d) if desc else None, C.byref(state) if st else None, cap, tiled, obs, first, plan_idx, action,
                                         value, logp, adv, ret, norm, tick, env, batch, s, plan, action_out, value_out, logp_out, adv_out,
                                         ret_out, None)


def test_the_library_exports_the_two_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    for n, k in (("snac_gae", 13), ("snac_replay_gather_onpolicy", 24)):
        assert n in _lib.EXPORTS
        assert getattr(L, n) is not None
        assert len(getattr(L, n).argtypes) == k
    assert _lib.PROTOTYPES["snac_gae"][1][4:6] == [C.c_double, C.c_double]
    assert _lib.GAE_CHUNK >= 2


def test_gae_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    for N in (0, -1):
        _err(L, _gae(L, N=N), b"N must be")
    for cap in (0, -4):
        _err(L, _gae(L, cap=cap, count=0), b"cap must be")
    for first in (-1, 8, 100):
        _err(L, _gae(L, first=first), b"first must be in [0, cap)")
    for count in (-1, 9, 1 << 20):
        _err(L, _gae(L, count=count), b"count must be in [0, cap]")
    for bad in (float("nan"), float("inf"), float("-inf")):
        _err(L, _gae(L, gamma=bad), b"finite")
        _err(L, _gae(L, lam=bad), b"finite")
        _err(L, _gae(L, gamma=bad, count=0), b"finite")
    for name in ("reward", "done", "value", "adv", "ret"):
        _err(L, _gae(L, **{name: None}), b"null ring array")
        _err(L, _gae(L, count=0, **{name: None}), b"null ring array")    # the checks come before the empty span
    # an empty span: no launch
    assert _gae(L, count=0) == 0
    assert _gae(L, count=0, boot=None, first=7, gamma=0.0, lam=0.0) == 0
    assert _gae(L, count=0, cap=1, N=1) == 0


def test_gather_onpolicy_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _err(L, _gather(L, desc=False), b"null desc/state")
    _err(L, _gather(L, st=False), b"null desc/state")
    for cap in (1, 0, -4):
        _err(L, _gather(L, cap=cap), b"cap must be")
    _err(L, _gather(L, batch=-1), b"batch >= 0")
    for name in ("obs", "first", "action", "value", "logp", "adv", "ret"):
        _err(L, _gather(L, **{name: None}), b"null ring array")
    for name in ("tick", "env"):
        _err(L, _gather(L, **{name: None}), b"null index array")
    _err(L, _gather(L, plan_idx=None), b"plan_out needs plan_idx_ring")
    for kind in (2, 3):
        _err(L, _gather(L, kind=kind, plan=C.c_void_p((1 << 20) + 8)), b"16-byte")
    for tail in (2, 4, 3):                                           # the plan tail, the record tail, position + plan
        rc = _gather(L, tail=tail)
        assert rc == -3 and b"position tail only" in L.snac_last_error(), (rc, L.snac_last_error())   # SNAC_ERR_UNSUPPORTED
    for name in ("s", "action_out", "value_out", "logp_out", "adv_out", "ret_out"):
        _err(L, _gather(L, **{name: None}), b"null output")
    # an empty batch: no launch -- but the checks come first
    assert _gather(L, batch=0) == 0
    assert _gather(L, batch=0, plan=None, plan_idx=None, norm=None) == 0
    assert _gather(L, batch=0, kind=1, tail=1, plan=C.c_void_p((1 << 20) + 4)) == 0    # 1D: plan_out needs no alignment; the position tail
    assert _gather(L, batch=0, tiled=1, plan=ODD) == 0
    _err(L, _gather(L, batch=0, obs=None), b"null ring array")
    _err(L, _gather(L, batch=0, adv_out=None), b"null output")


# ---- the python layer -----------------------------------------------------------------------------------------------------------------
def _buffer(**have):
    """A RolloutBuffer that was never built on a device: touching anything is the failure the tests look for."""
    from snac_amd import RolloutBuffer

    b = object.__new__(RolloutBuffer)
    b.env = b.ring = _NoDevice()
    b.__dict__.update(have)
    return b


@pytest.mark.parametrize("horizon", [0, -1, 2.0, True, "3", None])
def test_rollout_buffer_rejects_a_bad_horizon_before_touching_a_device(horizon):
    from snac_amd import RolloutBuffer

    with pytest.raises(ValueError, match="horizon must be an integer >= 1"):
        RolloutBuffer(_NoDevice(), horizon, 0.99, 0.95)


@pytest.mark.parametrize("bad", [None, float("nan"), float("inf"), float("-inf"), "0.9", True])
def test_rollout_buffer_rejects_a_non_finite_gamma_or_lambda_before_touching_a_device(bad):
    from snac_amd import RolloutBuffer

    with pytest.raises(ValueError, match="gamma must be a finite number"):
        RolloutBuffer(_NoDevice(), 8, bad, 0.95)
    with pytest.raises(ValueError, match="lam must be a finite number"):
        RolloutBuffer(_NoDevice(), 8, 0.99, bad)
    with pytest.raises(ValueError, match="layout"):
        RolloutBuffer(_NoDevice(), 8, 0.99, 0.95, layout="rows")


def test_rollout_buffer_calls_reject_bad_arguments_before_touching_a_device():
    with pytest.raises(ValueError, match="needs 4 ticks"):
        _buffer(horizon=4, collected=3).finish(None)
    for batch in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="batch must be an integer >= 1"):
            _buffer(horizon=4, first=0).minibatches(batch)
    for epochs in (0, 1.0, True):
        with pytest.raises(ValueError, match="epochs must be an integer >= 1"):
            _buffer(horizon=4, first=0).minibatches(8, epochs=epochs)
    for normalise in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="normalise must be a bool"):
            _buffer(horizon=4, first=0).minibatches(8, normalise=normalise)
        with pytest.raises(ValueError, match="normalise must be a bool"):
            _buffer(horizon=4, first=0).gather([0], [0], normalise=normalise)
    with pytest.raises(ValueError, match="call finish"):
        _buffer(horizon=4, first=None).minibatches(8)


# ---- the two rules, in numpy --------------------------------------------------------------------------------------------------------
# A span is a dict: reward float32 / done uint8 / value float32 [cap, N], bootstrap float32 [N], first, count.
def make_span(rng, cap, N, first, count):
    """Generated contents: rewards that are integers plus fractions and values of both signs, done with probability 0.25 everywhere in
    the ring (also outside the span).  With four envs or more the first four columns are set by hand inside the span: no done; done at
    the newest slot; done at the oldest slot; done in the two newest slots (the oldest and the newest are one slot when count == 1)."""
    S = dict(reward=(rng.integers(-100, 11, size=(cap, N)) + rng.random((cap, N))).astype(np.float32), done=(rng.random((cap, N)) < 0.25).astype(np.uint8),
             value=(30.0 * rng.normal(size=(cap, N))).astype(np.float32), bootstrap=(30.0 * rng.normal(size=N)).astype(np.float32) + np.float32(0.5),
             first=first, count=count)
    if N >= 4:
        slots = span_slots(S)
        S["done"][slots, 0:4] = 0
        S["done"][slots[-1], 1] = 1
        S["done"][slots[0], 2] = 1
        S["done"][slots[-2:], 3] = 1
    return S


def span_slots(S):
    """The span's slots, oldest first."""
    return (S["first"] + np.arange(S["count"])) % S["reward"].shape[0]


def gae_rule(S, gamma, lam, bootstrap=True, adv=None, ret=None):
    """adv, ret [cap, N] float32 as the header states them, written into copies of the given arrays (zeros when None) at the span's slots only."""
    cap, N = S["reward"].shape
    adv = np.zeros((cap, N), np.float32) if adv is None else adv.copy()
    ret = np.zeros((cap, N), np.float32) if ret is None else ret.copy()
    gamma = np.float64(gamma)
    c = gamma * np.float64(lam)                                      # rounded once, before the loop
    nv = S["bootstrap"].astype(np.float64) if bootstrap else np.zeros(N, np.float64)
    a = np.zeros(N, np.float64)
    for slot in span_slots(S)[::-1]:                                 # numpy rounds every product, sum and difference on its own
        r, v, d = S["reward"][slot].astype(np.float64), S["value"][slot].astype(np.float64), S["done"][slot] != 0
        delta = (r + np.where(d, 0.0, gamma * nv)) - v
        a = delta + np.where(d, 0.0, c * a)
        adv[slot] = a.astype(np.float32)
        ret[slot] = (a + v).astype(np.float32)
        nv = v
    return adv, ret


def onpolicy_rule(R, V, t, i, norm=None):
    """The PPO sample (t, i): R a ring of tests/test_replay_nstep_host.py (make_ring), V the four [cap, N] float32 arrays value / logp /
    adv / ret, norm None or the float32 pair {mean, rstd}."""
    step = gather_rule(R, t, i)
    adv = V["adv"][t, i]
    if norm is not None:                                             # float32: the difference and the product each rounded
        adv = (np.float32(adv) - np.float32(norm[0])) * np.float32(norm[1])
    return dict(s=step["s"], plan=step["plan"], action=step["action"], value=V["value"][t, i], logp=V["logp"][t, i], adv=np.float32(adv), ret=V["ret"][t, i])


# the spans of tests/test_gpu_onpolicy.py: per cap the counts 1, K - 1, K, K + 1, 2 K + 3 and cap (clipped to cap), K the kernel's chunk; each
# from the ring's last slot (wraps whenever count >= 2) and from its middle
K = _lib.GAE_CHUNK
SIZES = (1, 63, 64, 65, 200)
CAPS = (2, 8, 37)
GAMMA, LAM = 0.97, 0.9


def span_cases():
    out = []
    for cap in CAPS:
        for count in sorted({min(c, cap) for c in (1, K - 1, K, K + 1, 2 * K + 3, cap)}):
            for first in sorted({cap - 1, cap // 2}):
                out.append((cap, first, count))
    return out


def span_seed(N, cap, first, count):
    return ((N * 100 + cap) * 100 + first) * 100 + count


def test_the_spans_contain_every_case_that_can_go_wrong():
    met = dict(no_done=0, done_newest=0, done_oldest=0, adjacent=0, wraps=0, count_1=0, count_cap=0, negative_value=0, negative_reward=0,
               positive_reward=0, chunk_boundary=0, several_chunks=0, wraps_inside_a_chunk=0)
    assert (37, 36, 2 * K + 3) in span_cases() and (2, 1, 2) in span_cases()
    for N in SIZES:
        for cap, first, count in span_cases():
            S = make_span(np.random.default_rng(span_seed(N, cap, first, count)), cap, N, first, count)
            slots = span_slots(S)
            assert len(slots) == count and len(set(slots.tolist())) == count
            d = S["done"][slots] != 0                                # [count, N], oldest first
            met["no_done"] += int((~d.any(axis=0)).sum())
            met["done_newest"] += int(d[-1].sum())
            met["done_oldest"] += int(d[0].sum())
            met["adjacent"] += int((d[1:] & d[:-1]).sum())
            met["wraps"] += first + count > cap
            met["count_1"] += count == 1
            met["count_cap"] += count == cap
            met["negative_value"] += int((S["value"][slots] < 0).sum())
            met["negative_reward"] += int((S["reward"][slots] < 0).sum())
            met["positive_reward"] += int((S["reward"][slots] > 0).sum())
            met["chunk_boundary"] += count in (K - 1, K, K + 1)
            met["several_chunks"] += count > 2 * K
            for p0 in range(count - 1, -1, -K):                      # a chunk holds K slots back from the newest: one that crosses slot 0
                chunk = [(first + p) % cap for p in range(p0, max(p0 - K, -1), -1)]
                met["wraps_inside_a_chunk"] += any(b > a for a, b in zip(chunk, chunk[1:]))
            if N >= 4:                                               # the four columns set by hand, in every span
                assert not d[:, 0].any() and d[-1, 1] and d[0, 2] and d[-1, 3] and (count < 2 or d[-2, 3])
    assert all(v > 0 for v in met.values()), met


@pytest.mark.parametrize("cap,first,count", [(8, 7, 8), (37, 18, 19), (2, 1, 1)])
def test_with_lambda_zero_the_advantage_is_the_td_error(cap, first, count):
    S = make_span(np.random.default_rng(cap), cap, 9, first, count)
    adv, ret = gae_rule(S, GAMMA, 0.0)
    slots = span_slots(S)
    for j, slot in enumerate(slots):
        nv = S["bootstrap"] if j == count - 1 else S["value"][slots[j + 1]]
        r, v, d = S["reward"][slot].astype(np.float64), S["value"][slot].astype(np.float64), S["done"][slot] != 0
        delta = (r + np.where(d, 0.0, np.float64(GAMMA) * nv.astype(np.float64))) - v
        assert np.array_equal(adv[slot], delta.astype(np.float32))
        assert np.array_equal(ret[slot], (delta + v).astype(np.float32))
    outside = np.setdiff1d(np.arange(cap), slots)
    assert not adv[outside].any() and not ret[outside].any()         # slots outside the span are not written


def test_with_done_everywhere_the_advantage_is_reward_minus_value():
    S = make_span(np.random.default_rng(3), 8, 9, 5, 6)
    S["done"][:] = 1
    for lam in (0.0, LAM, 1.0):
        adv, ret = gae_rule(S, GAMMA, lam)
        slots = span_slots(S)
        want = S["reward"][slots].astype(np.float64) - S["value"][slots]
        assert np.array_equal(adv[slots], want.astype(np.float32))
        assert np.array_equal(adv, gae_rule(S, GAMMA, lam, bootstrap=False)[0])      # the bootstrap is ignored behind a done
    S["done"][:] = 0
    S["done"][span_slots(S)[-1]] = 1                                 # done at the newest slot only: the bootstrap is ignored, the trace runs
    assert np.array_equal(gae_rule(S, GAMMA, LAM)[0], gae_rule(S, GAMMA, LAM, bootstrap=False)[0])
    S["done"][:] = 0
    assert not np.array_equal(gae_rule(S, GAMMA, LAM)[0], gae_rule(S, GAMMA, LAM, bootstrap=False)[0])


def test_the_normalised_advantage_is_rounded_twice_in_float32():
    rng = np.random.default_rng(11)
    from test_replay_nstep_host import make_ring

    R = make_ring(rng, 7, 5, 7, 3, 10, np.float64, cells=30)
    V = {k: (10.0 * rng.normal(size=(7, 5))).astype(np.float32) for k in ("value", "logp", "adv", "ret")}
    norm = np.array([V["adv"].mean(), 1.0 / (V["adv"].std() + 1e-8)], np.float32)
    plain, normed = onpolicy_rule(R, V, 4, 2), onpolicy_rule(R, V, 4, 2, norm)
    assert plain["adv"] == V["adv"][4, 2] and normed["adv"].dtype == np.float32
    assert normed["adv"] == np.float32(np.float32(V["adv"][4, 2] - norm[0]) * norm[1])
    for key in ("s", "plan", "action", "value", "logp", "ret"):
        assert np.asarray(plain[key]).tobytes() == np.asarray(normed[key]).tobytes()
    assert plain["s"].tobytes() == gather_rule(R, 4, 2)["s"].tobytes() and "s_next" not in plain
