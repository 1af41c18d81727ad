"""Host: snac_replay_gather_nstep and snac_replay_gather_windows are exported and check every argument before any HIP call -- each failing
call below fails its checks first, so the placeholder pointers are never dereferenced, and an empty batch returns 0 although no device
exists to launch on (so do snac_replay_gather and snac_replay_gather_tiled, the plain gather beside them) -- and ReplayRing.sample(n_step=) / gather_nstep() / gather_windows() / sample_windows() reject bad arguments on an
object that was never built on a device.  Last, the two rules as include/snac_hip.h states them ("n-step transitions and episode
windows"), in numpy, independently of the kernels (tests/test_gpu_replay_nstep.py compares the kernels with them): n = 1 and L = 1 are the
tuple of snac_replay_gather, and the constructed rings that the GPU test uses meet every stop of both walks."""
import ctypes as C

import numpy as np
import pytest

from cabi_checks import ODD, PH, _err, _NoDevice
from snac_amd import _lib


def ring_desc(kind=2, tail=0):
    return _lib.EnvDesc(kind, 1, 16, 4, 0, 0, 1, 0, 0, 0, 0, 0, tail, 0)


def _nstep(L, desc=True, st=True, kind=2, tail=0, cap=8, tiled=0, obs=PH, first=PH, done=PH, reward=PH, action=PH, plan_idx=PH, newest=3, tick=PH,
           env=PH, batch=4, n=3, gamma=0.97, s=PH, s_next=PH, plan=PH, action_out=PH, ret=PH, disc=PH, done_out=PH, steps=PH):
    d, state = ring_desc(kind, tail), _lib.State(*[1 << 20] * 8)  # never dereferenced
    return L.snac_replay_gather_nstep(C.byref(d) if desc else None, C.byref(state) if st else None, cap, tiled, obs, first, done, reward, action,
                                      plan_idx, newest, tick, env, batch, n, gamma, s, s_next, plan, action_out, ret, disc, done_out, steps, None)


def _windows(L, desc=True, st=True, kind=2, tail=0, cap=8, tiled=0, obs=PH, first=PH, done=PH, reward=PH, action=PH, plan_idx=PH, oldest=3, tick=PH,
             env=PH, batch=4, length=5, s=PH, s_next=PH, plan=PH, action_out=PH, reward_out=PH, done_out=PH, mask=PH, length_out=PH):
    d, state = ring_desc(kind, tail), _lib.State(*[1 << 20] * 8)
    return L.snac_replay_gather_windows(C.byref(d) if desc else None, C.byref(state) if st else None, cap, tiled, obs, first, done, reward, action,
                                        plan_idx, oldest, tick, env, batch, length, s, s_next, plan, action_out, reward_out, done_out, mask,
                                        length_out, None)


def test_the_library_exports_the_two_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    for n, k in (("snac_replay_gather_nstep", 25), ("snac_replay_gather_windows", 24)):
        assert n in _lib.EXPORTS
        assert getattr(L, n) is not None
        assert len(getattr(L, n).argtypes) == k


def _shared_checks(L, call, end, steps):
    _err(L, call(L, desc=False), b"null desc/state")
    _err(L, call(L, st=False), b"null desc/state")
    for cap in (1, 0, -4):
        _err(L, call(L, cap=cap, **{end: 0}), b"cap must be")
    _err(L, call(L, batch=-1), b"batch >= 0")
    for v in (0, -1, 65, 1 << 20):
        _err(L, call(L, **{steps: v}), b"in [1, 64]")
    for v in (-1, 8, 100):
        _err(L, call(L, **{end: v}), b"in [0, cap)")
    for name in ("obs", "first", "done", "reward", "action"):
        _err(L, call(L, **{name: None}), b"null ring array")
    for name in ("tick", "env"):
        _err(L, call(L, **{name: None}), b"null index array")
    _err(L, call(L, plan_idx=None), b"plan_out needs plan_idx_ring")
    for kind in (2, 3):
        _err(L, call(L, kind=kind, plan=C.c_void_p((1 << 20) + 8)), b"16-byte")
    for tail in (2, 4, 3):                                           # the plan tail, the record tail, position + plan
        rc = call(L, tail=tail)
        assert rc == -3 and b"position tail only" in L.snac_last_error(), (rc, L.snac_last_error())   # SNAC_ERR_UNSUPPORTED
    for name in ("s", "s_next", "action_out", "done_out"):
        _err(L, call(L, **{name: None}), b"null output")
    # an empty batch: no launch -- but the checks come first
    assert call(L, batch=0) == 0
    assert call(L, batch=0, plan=None, plan_idx=None) == 0
    assert call(L, batch=0, kind=1, tail=1, plan=C.c_void_p((1 << 20) + 4)) == 0    # 1D: plan_out needs no alignment; the position tail
    assert call(L, batch=0, tiled=1) == 0
    _err(L, call(L, batch=0, obs=None), b"null ring array")
    _err(L, call(L, batch=0, **{steps: 0}), b"in [1, 64]")
    _err(L, call(L, batch=0, s=None), b"null output")


def test_gather_nstep_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _shared_checks(L, _nstep, "newest", "n")
    for g in (float("nan"), float("inf"), float("-inf")):
        _err(L, _nstep(L, gamma=g), b"gamma must be finite")
        _err(L, _nstep(L, gamma=g, batch=0), b"gamma must be finite")
    for name in ("ret", "disc", "steps"):
        _err(L, _nstep(L, **{name: None}), b"null output")
    assert _nstep(L, batch=0, n=64, gamma=0.0, newest=7) == 0
    assert ODD.value % 128 == 64                                     # (an aligned-enough plan_out: 16-byte is all that is asked)
    assert _nstep(L, batch=0, plan=ODD) == 0


def test_gather_windows_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _shared_checks(L, _windows, "oldest", "length")
    for name in ("reward_out", "mask", "length_out"):
        _err(L, _windows(L, **{name: None}), b"null output")
    assert _windows(L, batch=0, length=64, oldest=7) == 0


def _plain(L, fn="snac_replay_gather", desc=True, st=True, kind=2, tail=0, cap=8, obs=PH, first=PH, plan_idx=PH, tick=PH, env=PH, batch=4, s=PH,
           s_next=PH, plan=PH):
    d, state = ring_desc(kind, tail), _lib.State(*[1 << 20] * 8)  # never dereferenced
    return getattr(L, fn)(C.byref(d) if desc else None, C.byref(state) if st else None, cap, obs, first, plan_idx, tick, env, batch, s, s_next,
                          plan, None)


@pytest.mark.parametrize("fn", ["snac_replay_gather", "snac_replay_gather_tiled"])
def test_the_plain_gather_validates_its_arguments_before_any_hip_call(fn):
    L = _lib.lib()
    assert len(getattr(L, fn).argtypes) == 13
    call = lambda **kw: _plain(L, fn, **kw)  # noqa: E731
    _err(L, call(desc=False), b"null desc/state")
    _err(L, call(st=False), b"null desc/state")
    _err(L, call(cap=1), b"cap must be")
    _err(L, call(batch=-1), b"batch >= 0")
    for name in ("obs", "first", "tick", "env", "s", "s_next"):
        _err(L, call(**{name: None}), b"null pointer")
        _err(L, call(batch=0, **{name: None}), b"null pointer")      # the checks come before the empty batch
    _err(L, call(plan_idx=None), b"plan_out needs plan_idx_ring")
    for kind in (2, 3):
        _err(L, call(kind=kind, plan=C.c_void_p((1 << 20) + 4)), b"16-byte")
    for tail in (2, 4, 3):                                           # the plan tail, the record tail, position + plan
        rc = call(tail=tail)
        assert rc == -3 and b"position tail only" in L.snac_last_error(), (rc, L.snac_last_error())   # SNAC_ERR_UNSUPPORTED
    # the order: cap and batch before the null tests, those before the plan checks, those before the tail
    _err(L, call(cap=1, obs=None), b"cap must be")
    _err(L, call(obs=None, plan_idx=None), b"null pointer")
    _err(L, call(plan_idx=None, tail=2), b"plan_out needs plan_idx_ring")
    # an empty batch: no launch -- but the checks come first
    assert call(batch=0) == 0
    assert call(batch=0, plan=None, plan_idx=None) == 0
    assert call(batch=0, kind=1, tail=1, plan=C.c_void_p((1 << 20) + 4)) == 0    # 1D: plan_out needs no alignment; the position tail
    assert call(batch=0, plan=ODD) == 0


# ---- the python layer -----------------------------------------------------------------------------------------------------------------
def _ring():
    """A ReplayRing that was never built on a device: touching anything is the failure the tests look for."""
    from snac_amd import ReplayRing

    r = object.__new__(ReplayRing)
    r.env = _NoDevice()
    return r


@pytest.mark.parametrize("n", [0, -1, 65, 2.0, 1.5, True, "3", None])
def test_gather_nstep_rejects_a_bad_n_before_touching_a_device(n):
    with pytest.raises(ValueError, match=r"n must be an integer in \[1, 64\]"):
        _ring().gather_nstep([0], [0], n, 0.9)
    if n is not None:                                                # sample(): None is the one-step path
        with pytest.raises(ValueError, match=r"n_step must be an integer in \[1, 64\]"):
            _ring().sample(8, n_step=n, gamma=0.9)


@pytest.mark.parametrize("gamma", [None, float("nan"), float("inf"), float("-inf"), "0.9", True])
def test_n_step_rejects_a_missing_or_non_finite_gamma_before_touching_a_device(gamma):
    with pytest.raises(ValueError, match="gamma"):
        _ring().sample(8, n_step=3, gamma=gamma)
    with pytest.raises(ValueError, match="gamma"):
        _ring().gather_nstep([0], [0], 3, gamma)


@pytest.mark.parametrize("length", [0, -1, 65, 2.0, True, None])
def test_windows_reject_a_bad_length_before_touching_a_device(length):
    with pytest.raises(ValueError, match=r"length must be an integer in \[1, 64\]"):
        _ring().gather_windows([0], [0], length)
    with pytest.raises(ValueError, match=r"length must be an integer in \[1, 64\]"):
        _ring().sample_windows(8, length)


# ---- the two rules, in numpy --------------------------------------------------------------------------------------------------------
# A ring is a dict: obs [cap, N, D] (the ring's dtype; either layout holds these rows), reward float32 / done uint8 / first uint8 /
# action int8 / plan_idx int16 [cap, N], head, ticks, reset [D] float32 (the reset observation), plans [P, cells] float32.
def make_ring(rng, cap, N, D, head, ticks, dtype, num_plans=16, cells=400):
    """Generated contents: done with probability 0.3, first[t + 1] = done[t] plus a few first flags without a done, rewards that are
    integers plus fractions."""
    done = (rng.random((cap, N)) < 0.3).astype(np.uint8)
    first = (np.roll(done, 1, axis=0) | (rng.random((cap, N)) < 0.06)).astype(np.uint8)
    return dict(obs=rng.normal(size=(cap, N, D)).astype(dtype), reward=(rng.integers(-100, 11, size=(cap, N)) + rng.random((cap, N))).astype(np.float32),
                done=done, first=first, action=rng.integers(0, 5, size=(cap, N)).astype(np.int8),
                plan_idx=rng.integers(0, num_plans, size=(cap, N)).astype(np.int16), head=head, ticks=ticks,
                reset=rng.normal(size=D).astype(np.float32), plans=rng.integers(0, 2, size=(num_plans, cells)).astype(np.float32))


def valid_ticks(R):
    cap = R["reward"].shape[0]
    return R["ticks"] if R["ticks"] < cap else cap - 1


def addressable(R):
    """(slot, env) of every addressable transition, oldest slot first."""
    cap, N = R["reward"].shape
    v = valid_ticks(R)
    return [((R["head"] - v + j) % cap, i) for j in range(v) for i in range(N)]


def gather_rule(R, t, i):
    """The tuple of step (t, i), as snac_replay_gather defines it."""
    cap = R["reward"].shape[0]
    s = R["reset"] if R["first"][t, i] else R["obs"][(t - 1) % cap, i].astype(np.float32)
    return dict(s=s, s_next=R["obs"][t, i].astype(np.float32), action=np.int64(R["action"][t, i]), reward=R["reward"][t, i],
                done=bool(R["done"][t, i]), plan=R["plans"][R["plan_idx"][t, i]])


def nstep_rule(R, t, i, n, gamma):
    cap = R["reward"].shape[0]
    newest = (R["head"] - 1) % cap
    slot = lambda k: (t + k) % cap  # noqa: E731
    k = 0
    while True:
        why = dict(done=R["done"][slot(k), i] != 0, n=k + 1 == n, newest=slot(k) == newest, first=R["first"][slot(k + 1), i] != 0)
        if any(why.values()):
            break
        k += 1
    m = k + 1
    g = 0.0                                                          # python floats are doubles: product and sum each rounded
    for k in range(m - 1, -1, -1):
        g = float(R["reward"][slot(k), i]) + float(gamma) * g
    d = 1.0
    for _ in range(m):
        d = d * float(gamma)
    done = bool(R["done"][slot(m - 1), i])
    first = gather_rule(R, t, i)
    out = dict(s=first["s"], action=first["action"], plan=first["plan"], s_next=R["obs"][slot(m - 1), i].astype(np.float32), done=done,
               steps=np.int32(m), discount=np.float32(0.0) if done else np.float32(d), why=why)
    out["return"] = np.float32(g)
    return out


def window_rule(R, t, i, L):
    cap, D = R["reward"].shape[0], R["obs"].shape[2]
    oldest = (R["head"] - valid_ticks(R)) % cap
    n = 1
    while True:
        e = (t - n + 1) % cap                                        # the window's earliest step
        why = dict(L=n >= L, oldest=e == oldest, first=R["first"][e, i] != 0, done=R["done"][(e - 1) % cap, i] != 0)
        if any(why.values()):
            break
        n += 1
    out = dict(s=np.zeros((L, D), np.float32), s_next=np.zeros((L, D), np.float32), action=np.zeros(L, np.int64), reward=np.zeros(L, np.float32),
               done=np.zeros(L, bool), mask=np.arange(L) < n, length=np.int32(n), plan=R["plans"][R["plan_idx"][t, i]], why=why)
    for j in range(n):
        step = gather_rule(R, (t - n + 1 + j) % cap, i)
        for key in ("s", "s_next", "action", "reward", "done"):
            out[key][j] = step[key]
    return out


# the rings of tests/test_gpu_replay_nstep.py: cap = 7 and 12, wrapped (head in the middle) and not yet full (ticks < cap)
FILLS = [(7, 3, 7 + 3), (7, 5, 5), (12, 8, 2 * 12 + 8), (12, 9, 9)]      # cap, head, ticks
NSTEPS = lambda cap: (1, 2, 3, cap - 1, 64)  # noqa: E731
LENGTHS = (1, 2, 5, 64)
GAMMA = 0.9


def ring_seed(kind, f32, N, cap, head):
    return ((kind * 2 + int(f32)) * 100 + N) * 1000 + cap * 20 + head


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("cap,head,ticks", FILLS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_step_and_a_window_of_one_are_the_gather_tuple(cap, head, ticks, dtype):
    R = make_ring(np.random.default_rng(cap * 100 + head), cap, 9, 7, head, ticks, dtype, cells=30)
    pairs = addressable(R)
    assert len(pairs) == valid_ticks(R) * 9
    for t, i in pairs:
        want = gather_rule(R, t, i)
        one = nstep_rule(R, t, i, 1, GAMMA)
        assert one["steps"] == 1 and _same(one["return"], want["reward"]) and one["done"] == want["done"]
        assert _same(one["discount"], np.float32(0.0) if want["done"] else np.float32(GAMMA))
        for key in ("s", "s_next", "action", "plan"):
            assert _same(one[key], want[key]), key
        win = window_rule(R, t, i, 1)
        assert win["length"] == 1 and win["mask"].tolist() == [True] and _same(win["plan"], want["plan"])
        for key in ("s", "s_next", "action", "reward", "done"):
            assert _same(win[key][0], want[key]), key
        # and a longer window chains: s[j + 1] == s_next[j], zeros past its length
        long = window_rule(R, t, i, 5)
        n = int(long["length"])
        assert _same(long["s"][1:n], long["s_next"][:n - 1]) and not long["s"][n:].any() and not long["reward"][n:].any()
        assert _same(long["s_next"][n - 1], want["s_next"]) and not long["done"][:n - 1].any()


def test_the_n_step_return_is_the_discounted_sum_up_to_the_first_stop():
    R = make_ring(np.random.default_rng(5), 12, 4, 7, 8, 32, np.float32, cells=30)
    R["done"][:] = 0
    R["first"][:] = 0
    R["reward"][:] = 1.0
    t = (R["head"] - 6) % 12                                         # six steps up to the newest slot
    a = nstep_rule(R, t, 0, 4, 0.5)
    assert a["steps"] == 4 and a["return"] == np.float32(1.875) and a["discount"] == np.float32(0.0625) and a["why"]["n"]
    b = nstep_rule(R, t, 0, 64, 0.5)
    assert b["steps"] == 6 and b["why"]["newest"] and not b["why"]["n"] and _same(b["s_next"], R["obs"][(R["head"] - 1) % 12, 0])
    R["done"][(t + 2) % 12, 0] = 1
    c = nstep_rule(R, t, 0, 64, 0.5)
    assert c["steps"] == 3 and c["done"] and c["discount"] == 0 and c["return"] == np.float32(1.75)
    R["done"][:] = 0
    R["first"][(t + 2) % 12, 0] = 1                                  # an episode that ended without a done
    d = nstep_rule(R, t, 0, 64, 0.5)
    assert d["steps"] == 2 and not d["done"] and d["discount"] == np.float32(0.25) and d["why"]["first"]


def test_the_constructed_rings_meet_every_stop_of_both_walks():
    """What tests/test_gpu_replay_nstep.py compares the kernels with: each of the four n-step stops and of the four window stops ends
    some walk, alone where it can (a `first` without a `done` before it; the newest slot before n steps)."""
    met = dict(done=0, n=0, newest=0, first_without_done=0, newest_alone=0)
    wmet = dict(L=0, oldest=0, first=0, done=0, oldest_alone=0, shorter=0)
    for N in (5, 70):
        for cap, head, ticks in FILLS:
            R = make_ring(np.random.default_rng(ring_seed(2, False, N, cap, head)), cap, N, 51, head, ticks, np.float64)
            for t, i in addressable(R):
                for n in NSTEPS(cap):
                    why = nstep_rule(R, t, i, n, GAMMA)["why"]
                    met["done"] += bool(why["done"]); met["n"] += bool(why["n"]); met["newest"] += bool(why["newest"])
                    met["first_without_done"] += bool(why["first"] and not why["done"])
                    met["newest_alone"] += bool(why["newest"] and not (why["done"] or why["n"] or why["first"]))
                for L in LENGTHS:
                    w = window_rule(R, t, i, L)
                    for key in ("L", "oldest", "first", "done"):
                        wmet[key] += bool(w["why"][key])
                    wmet["oldest_alone"] += bool(w["why"]["oldest"] and not (w["why"]["L"] or w["why"]["first"] or w["why"]["done"]))
                    wmet["shorter"] += int(w["length"]) < L
    assert all(v > 0 for v in met.values()), met
    assert all(v > 0 for v in wmet.values()), wmet
