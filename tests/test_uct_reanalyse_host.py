"""Host: the Reanalyse entry points (snac_uct_save_roots, snac_uct_load_roots, snac_uct_store_targets, snac_uct_returns_nstep) are exported
and check every argument before any HIP call -- each failing call below fails its checks first, so the placeholder pointers are never
dereferenced, and an empty job returns 0 although no device exists to launch on -- and SelfPlay(keep_states=) / reanalyse() /
targets(td_steps=) / UCTSearch.load_roots() reject bad arguments before they touch a device.  Last, the n-step rule as include/snac_hip.h
states it ("Reanalyse"), in numpy, independently of the kernel: n = 1 is r + (done ? 0 : gamma * v_next), and n >= count is the
Monte-Carlo recurrence of snac_uct_returns bit for bit."""
import ctypes as C

import numpy as np
import pytest

from cabi_checks import ODD, PH, _err, _NoDevice
from snac_amd import _lib
from test_uct_selfplay_host import hostless_search, tree_checks

PH2 = C.c_void_p(1 << 24)                                            # a second placeholder, far from PH: src beside records


def _save(L, B=4, cap=8, records=PH, rb=128, rrows=100, out=PH2):
    return L.snac_uct_save_roots(B, cap, records, rb, rrows, out, None)


def _load(L, A=5, stats=PH, rows=100, B=4, cap=8, records=PH, rb=128, rrows=100, src=PH2, srows=4, index=PH, used=PH):
    return L.snac_uct_load_roots(A, stats, rows, B, cap, records, rb, rrows, src, srows, index, used, None)


def _store(L, A=5, stats=PH, rows=100, B=4, cap=8, index=PH, entries=64, policy=PH, pi=PH, value=PH, refreshed=PH):
    return L.snac_uct_store_targets(A, stats, rows, B, cap, index, entries, policy, pi, value, refreshed, None)


def _nstep(L, B=4, capm=8, first=0, count=8, n=3, gamma=0.97, reward=PH, done=PH, value=PH, boot=PH, z=PH):
    return L.snac_uct_returns_nstep(B, capm, first, count, n, gamma, reward, done, value, boot, z, None)


def test_the_library_exports_the_reanalyse_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    for n, k in (("snac_uct_save_roots", 7), ("snac_uct_load_roots", 13), ("snac_uct_store_targets", 12), ("snac_uct_returns_nstep", 12)):
        assert n in _lib.EXPORTS
        assert getattr(L, n) is not None
        assert len(getattr(L, n).argtypes) == k


def _record_checks(L, call):
    _err(L, call(L, records=None), b"null records")
    _err(L, call(L, records=ODD), b"records must be 128-byte")
    for rb in (0, 64, 256, 512, 895, 1024):
        _err(L, call(L, rb=rb), b"record_bytes")
    _err(L, call(L, rrows=35), b"exceed record_rows")                # B * (cap + 1) = 36 rows needed
    _err(L, call(L, rb=896, rrows=35), b"exceed record_rows")


def test_save_roots_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _err(L, _save(L, B=0), b"B must be")
    _err(L, _save(L, B=-3), b"B must be")
    _err(L, _save(L, cap=0), b"cap must be")
    _err(L, _save(L, B=1 << 16, cap=1 << 15, rrows=0x7FFFFFFF), b"exceed int32")
    _record_checks(L, _save)
    _err(L, _save(L, out=None), b"null out")
    _err(L, _save(L, out=ODD), b"out must be 128-byte")


def test_load_roots_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    tree_checks(L, _load)
    _record_checks(L, _load)
    _err(L, _load(L, src=None), b"null src")
    _err(L, _load(L, src=C.c_void_p((1 << 24) + 64)), b"src must be 128-byte")
    _err(L, _load(L, srows=0), b"src_rows must be")
    _err(L, _load(L, srows=-1), b"src_rows must be")
    _err(L, _load(L, srows=3, index=None), b"without an index")      # src[b] for every b < B
    _err(L, _load(L, used=None), b"null used")
    # records occupy [PH, PH + 100 * 128): src inside, across either end, and around them
    for src, srows in ((PH, 4), (C.c_void_p((1 << 20) + 99 * 128), 1), (C.c_void_p((1 << 20) - 128), 2), (C.c_void_p((1 << 20) - 1280), 500)):
        _err(L, _load(L, src=src, srows=srows), b"overlap")
    _err(L, _load(L, src=C.c_void_p((1 << 20) + 99 * 896), srows=1, rb=896), b"overlap")
    _err(L, _load(L, src=C.c_void_p((1 << 20) - 128), srows=1, stats=None), b"null stats")       # apart: the other checks decide
    _err(L, _load(L, src=C.c_void_p((1 << 20) + 100 * 128), srows=1, stats=None), b"null stats")


def test_store_targets_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    tree_checks(L, _store)
    _err(L, _store(L, index=None), b"null index")
    _err(L, _store(L, entries=-1), b"entries must be")
    _err(L, _store(L, pi=None), b"null ring array")
    _err(L, _store(L, value=None), b"null ring array")
    _err(L, _store(L, refreshed=None), b"null ring array")
    assert _store(L, entries=0) == 0                                 # no entry to write: no launch
    assert _store(L, entries=0, policy=None, rows=36) == 0
    _err(L, _store(L, entries=0, rows=35), b"exceed stats_rows")     # the checks come first
    _err(L, _store(L, entries=0, pi=None), b"null ring array")


def test_returns_nstep_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _err(L, _nstep(L, B=0), b"B must be")
    _err(L, _nstep(L, B=-1), b"B must be")
    _err(L, _nstep(L, capm=0, count=0), b"cap_moves must be")
    _err(L, _nstep(L, B=1 << 16, capm=1 << 16, count=1), b"exceed int32")
    _err(L, _nstep(L, first=-1), b"first must be")
    _err(L, _nstep(L, first=8), b"first must be")
    _err(L, _nstep(L, count=-1), b"count must be")
    _err(L, _nstep(L, count=9), b"count must be")
    _err(L, _nstep(L, n=0), b"n must be")
    _err(L, _nstep(L, n=-5), b"n must be")
    for g in (float("nan"), float("inf"), float("-inf")):
        _err(L, _nstep(L, gamma=g), b"gamma")
    _err(L, _nstep(L, reward=None), b"null ring array")
    _err(L, _nstep(L, done=None), b"null ring array")
    _err(L, _nstep(L, z=None), b"null ring array")
    _err(L, _nstep(L, value=None), b"null value")
    assert _nstep(L, count=0) == 0                                   # no slot to fill: no launch
    assert _nstep(L, count=0, boot=None, first=7, n=0x7FFFFFFF) == 0
    _err(L, _nstep(L, count=0, value=None), b"null value")           # the checks come first
    _err(L, _nstep(L, count=0, n=0), b"n must be")


# ---- the python layer -----------------------------------------------------------------------------------------------------------------
def hostless_play(keep_states=True, trees=4, cap=8, moves=8):
    """A SelfPlay that was never constructed on a device: the attributes reanalyse() and targets() check, nothing else."""
    from snac_amd import SelfPlay

    s = hostless_search(trees=trees, num_envs=trees)
    p = object.__new__(SelfPlay)
    p.search, p.env, p.keep_states, p.cap, p.moves, p.head = s, s.env, keep_states, cap, moves, moves % cap
    return p


def _second(p, trees=4, evaluator=len, max_iterations=16, num_actions=5):
    s = hostless_search(trees=trees)
    s.env, s.evaluator, s.max_iterations, s.num_actions = p.env, evaluator, max_iterations, num_actions
    return s


def test_selfplay_rejects_a_keep_states_that_is_no_bool_before_touching_a_device():
    from snac_amd import SelfPlay

    for k in (3, 1, 0, None, "yes"):
        with pytest.raises(ValueError, match="keep_states"):
            SelfPlay(hostless_search(), 8, keep_states=k)


def test_reanalyse_rejects_bad_arguments_before_touching_a_device():
    p = hostless_play()
    with pytest.raises(ValueError, match="keep_states=True"):
        hostless_play(keep_states=False).reanalyse(_second(p), 4)
    with pytest.raises(ValueError, match="second UCTSearch"):
        p.search.evaluator = len
        p.reanalyse(p.search, 4)                                     # the playing search itself
    other = _second(p)
    other.env = _NoDevice()
    with pytest.raises(ValueError, match="env of the playing search"):
        p.reanalyse(other, 4)
    with pytest.raises(ValueError, match="needs an evaluator"):
        p.reanalyse(_second(p, evaluator=None), 4)
    with pytest.raises(ValueError, match="actions"):
        p.reanalyse(_second(p, num_actions=3), 4)
    assert len(p) == 32
    with pytest.raises(ValueError, match="33 trees to reanalyse, 32 entries"):
        p.reanalyse(_second(p, trees=33), 4)                         # R > len(play)
    few = hostless_play(moves=2)
    assert len(few) == 8
    with pytest.raises(ValueError, match="9 trees to reanalyse, 8 entries"):
        few.reanalyse(_second(few, trees=9), 4)
    for its in (17, -1, 2.5):
        with pytest.raises(ValueError, match="iterations"):
            p.reanalyse(_second(p, max_iterations=16), its)          # the budget: iterations <= max_iterations


def test_targets_rejects_bad_td_steps_before_touching_a_device():
    p = hostless_play()
    for n in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="td_steps"):
            p.targets(td_steps=n)


def test_load_roots_rejects_wrong_shapes_before_touching_a_device():
    import torch

    class Pool:
        WORDS, KIND = 32, 2

    s = hostless_search()
    s.pool = Pool()
    ok = torch.zeros((6, 128), dtype=torch.uint8)
    for rec in (torch.zeros((6, 127), dtype=torch.uint8), torch.zeros((6, 896), dtype=torch.uint8), torch.zeros(6 * 128, dtype=torch.uint8),
                torch.zeros((6, 1, 128), dtype=torch.uint8), torch.zeros((6, 128), dtype=torch.int8), torch.zeros((6, 32), dtype=torch.int32),
                torch.zeros((0, 128), dtype=torch.uint8), torch.zeros((3, 128), dtype=torch.uint8), np.zeros((6, 128), np.uint8)):
        with pytest.raises(ValueError, match="records"):
            s.load_roots(rec)                                        # the last but one: 3 records, 4 trees, no index
    for idx in (torch.zeros(3, dtype=torch.int64), torch.zeros(5, dtype=torch.int32), torch.zeros(4), torch.zeros(4, dtype=torch.bool), [0, 1, 2, 3]):
        with pytest.raises(ValueError, match="index"):
            s.load_roots(ok, idx)
    s.env = _NoDevice(num_envs=4, device=torch.device("cuda", 0))    # the right shapes on the wrong device
    with pytest.raises(ValueError, match="must be on"):
        s.load_roots(ok)
    with pytest.raises(ValueError, match="must be on"):
        s.load_roots(ok, torch.zeros(4, dtype=torch.int64))


# ---- the n-step rule, in numpy -----------------------------------------------------------------------------------------------------------
def nstep(reward, done, value, first, count, n, gamma, bootstrap, z):
    """The header's statement, slot by slot: z's `count` slots from `first` on (modulo the ring), in place."""
    cap, B = reward.shape
    boot = np.zeros(B, np.float64) if bootstrap is None else bootstrap.astype(np.float64)
    for i in range(count):
        e = min(i + n, count)
        g = value[(first + e) % cap].astype(np.float64) if e < count else boot.copy()
        for j in range(e - 1, i - 1, -1):
            s = (first + j) % cap
            t = np.float64(gamma) * g
            g = reward[s].astype(np.float64) + np.where(done[s] != 0, 0.0, t)
        z[(first + i) % cap] = g.astype(np.float32)
    return z


def returns(reward, done, first, count, gamma, bootstrap, z):
    """snac_uct_returns as its header states it: one pass from the newest slot back."""
    cap, B = reward.shape
    g = np.zeros(B, np.float64) if bootstrap is None else bootstrap.astype(np.float64)
    for i in range(count - 1, -1, -1):
        s = (first + i) % cap
        t = np.float64(gamma) * g
        g = reward[s].astype(np.float64) + np.where(done[s] != 0, 0.0, t)
        z[s] = g.astype(np.float32)
    return z


@pytest.mark.parametrize("first,count", [(0, 6), (4, 4), (2, 1), (5, 6), (3, 0)])
def test_the_n_step_rule_at_one_step_and_at_the_whole_window(first, count):
    rng = np.random.default_rng(10 * first + count)
    cap, B, gamma = 6, 33, 0.9
    reward = (rng.integers(-100, 11, size=(cap, B)) + rng.random((cap, B))).astype(np.float32)
    done = (rng.random((cap, B)) < 0.3).astype(np.uint8)
    value = rng.normal(size=(cap, B)).astype(np.float32)
    boot = rng.normal(size=B).astype(np.float32)
    for bootstrap in (None, boot):
        z = nstep(reward, done, value, first, count, 1, gamma, bootstrap, np.full((cap, B), -7.5, np.float32))
        for i in range(count):                                       # n = 1: r + (done ? 0 : gamma * v_next), the ring's end bootstrapped
            s, nxt = (first + i) % cap, (first + i + 1) % cap
            v = value[nxt].astype(np.float64) if i + 1 < count else (np.zeros(B) if bootstrap is None else bootstrap.astype(np.float64))
            want = (reward[s].astype(np.float64) + np.where(done[s] != 0, 0.0, np.float64(gamma) * v)).astype(np.float32)
            assert z[s].tobytes() == want.tobytes()
        outside = [s for s in range(cap) if (s - first) % cap >= count]
        assert (z[outside] == -7.5).all()
        mc = returns(reward, done, first, count, gamma, bootstrap, np.full((cap, B), -7.5, np.float32))
        for n in (count, count + 1, 100, 0x7FFFFFFF):                # n >= count: the Monte-Carlo returns, bit for bit
            if n >= 1:
                got = nstep(reward, done, value, first, count, n, gamma, bootstrap, np.full((cap, B), -7.5, np.float32))
                assert got.tobytes() == mc.tobytes()
        if count >= 3:                                               # and a middle n differs from both somewhere: the values entered
            mid = nstep(reward, done, value, first, count, 2, gamma, bootstrap, np.full((cap, B), -7.5, np.float32))
            assert mid.tobytes() != mc.tobytes() and mid.tobytes() != z.tobytes()
