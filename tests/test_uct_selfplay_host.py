"""Host: the self-play entry points (snac_uct_pick_moves, snac_uct_restart, snac_uct_returns) are exported and check every argument
before any HIP call -- each failing call below fails its checks first, so the placeholder pointers are never dereferenced, and an empty
job returns 0 although no device exists to launch on -- and SelfPlay / UCTSearch.pick_moves / UCTSearch.restart reject bad arguments
before they touch a device.  Last, the sampler's rule as include/snac_hip.h states it ("Self-play": u = (w * total) >> 32, the lowest a
whose running sum of visits passes u), in numpy, independently of the kernel: u lands in [0, total), an unvisited action is never drawn,
and over an evenly spaced sweep of w the draws are within 1 of N_a / total of the sweep."""
import ctypes as C

import numpy as np
import pytest

from cabi_checks import ODD, PH, _desc, _err, _NoDevice
from snac_amd import _lib


def _pick(L, desc=True, A=5, stats=PH, rows=100, B=4, cap=8, greedy=PH, t=3, action=PH, pi=PH, value=PH):
    d = _desc(2)
    return L.snac_uct_pick_moves(C.byref(d) if desc else None, A, stats, rows, B, cap, greedy, t, action, pi, value, None)


def _restart(L, A=5, stats=PH, rows=100, B=4, cap=8, records=PH, rb=128, rrows=100, mask=PH, term=PH, used=PH):
    return L.snac_uct_restart(A, stats, rows, B, cap, records, rb, rrows, mask, term, used, None)


def _returns(L, B=4, capm=8, first=0, count=8, gamma=0.97, reward=PH, done=PH, boot=PH, z=PH):
    return L.snac_uct_returns(B, capm, first, count, gamma, reward, done, boot, z, None)


def test_the_library_exports_the_self_play_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    for n, k in (("snac_uct_pick_moves", 12), ("snac_uct_restart", 12), ("snac_uct_returns", 10)):
        assert n in _lib.EXPORTS
        assert getattr(L, n) is not None
        assert len(getattr(L, n).argtypes) == k


def tree_checks(L, call):
    for A in (0, 2, 4, 6, 7, 9):
        _err(L, call(L, A=A), b"num_actions")
    _err(L, call(L, stats=None), b"null stats")
    _err(L, call(L, B=0), b"B must be")
    _err(L, call(L, B=-3), b"B must be")
    _err(L, call(L, cap=0), b"cap must be")
    _err(L, call(L, rows=4 * 9 - 1), b"exceed stats_rows")           # B * (cap + 1) = 36 rows needed
    _err(L, call(L, B=1 << 16, cap=1 << 15, rows=0x7FFFFFFF), b"exceed int32")
    _err(L, call(L, stats=ODD), b"128-byte")


def test_pick_moves_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    tree_checks(L, _pick)
    _err(L, _pick(L, desc=False), b"null desc")
    assert _pick(L, action=None, pi=None, value=None) == 0           # nothing asked for: no launch
    assert _pick(L, action=None, pi=None, value=None, greedy=None, rows=36) == 0
    _err(L, _pick(L, action=None, pi=None, value=None, rows=35), b"exceed stats_rows")      # the checks come first


def test_restart_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    tree_checks(L, _restart)
    _err(L, _restart(L, records=None), b"null records")
    _err(L, _restart(L, records=ODD), b"records must be 128-byte")
    for rb in (0, 64, 256, 512, 895, 1024):
        _err(L, _restart(L, rb=rb), b"record_bytes")
    _err(L, _restart(L, rrows=35), b"exceed record_rows")
    _err(L, _restart(L, rb=896, rrows=35), b"exceed record_rows")
    _err(L, _restart(L, mask=None), b"null mask")
    _err(L, _restart(L, used=None), b"null used")


def test_returns_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _err(L, _returns(L, B=0), b"B must be")
    _err(L, _returns(L, B=-1), b"B must be")
    _err(L, _returns(L, capm=0, count=0), b"cap_moves must be")
    _err(L, _returns(L, B=1 << 16, capm=1 << 16, count=1), b"exceed int32")
    _err(L, _returns(L, first=-1), b"first must be")
    _err(L, _returns(L, first=8), b"first must be")
    _err(L, _returns(L, count=-1), b"count must be")
    _err(L, _returns(L, count=9), b"count must be")
    for g in (float("nan"), float("inf"), float("-inf")):
        _err(L, _returns(L, gamma=g), b"gamma")
    _err(L, _returns(L, reward=None), b"null ring array")
    _err(L, _returns(L, done=None), b"null ring array")
    _err(L, _returns(L, z=None), b"null ring array")
    assert _returns(L, count=0) == 0                                 # no slot to fill: no launch
    assert _returns(L, count=0, boot=None, first=7) == 0
    _err(L, _returns(L, count=0, z=None), b"null ring array")        # the checks come first


def hostless_search(trees=4, num_envs=4, **kw):
    """A UCTSearch that was never constructed on a device: the attributes the checks read, nothing else."""
    from snac_amd import UCTSearch

    s = object.__new__(UCTSearch)
    s.trees, s.num_actions, s.gamma, s.evaluator, s.max_iterations = trees, 5, 0.97, None, 100
    s.env = _NoDevice(num_envs=num_envs, **kw)
    return s


@pytest.mark.parametrize("kw", [dict(capacity_moves=0), dict(capacity_moves=-4), dict(capacity_moves=2.5), dict(capacity_moves=8, sample_moves=-1),
                                dict(capacity_moves=8, sample_moves=1.5), dict(capacity_moves=8, root_noise=3),
                                dict(capacity_moves=8, root_noise=lambda p: p), dict(capacity_moves=8, gamma=float("nan")),
                                dict(capacity_moves=8, gamma=float("inf"))])
def test_selfplay_rejects_bad_arguments_before_touching_a_device(kw):
    from snac_amd import SelfPlay

    with pytest.raises(ValueError):
        SelfPlay(hostless_search(), **kw)


def test_selfplay_needs_a_tree_per_env_row():
    from snac_amd import SelfPlay

    with pytest.raises(ValueError, match="tree b to env row b"):
        SelfPlay(hostless_search(trees=8, num_envs=4), 16)
    with pytest.raises(ValueError, match="tree b to env row b"):
        SelfPlay(hostless_search(trees=4, num_envs=8), 16)


def test_play_rejects_a_budget_below_an_episode_of_searches():
    from snac_amd import SelfPlay

    s = hostless_search(total_step=600)
    p = object.__new__(SelfPlay)                                     # as constructed, without the ring's device tensors
    p.search, p.env = s, s.env
    s.max_iterations = 601 * 8 - 1
    with pytest.raises(ValueError, match=r"\(total_step \+ 1\) \* iterations"):
        p.play(1, 8)
    with pytest.raises(ValueError):
        p.play(0, 8)                                                 # the budget is checked whatever the number of moves
    s.max_iterations = 601 * 8
    p._check_budget(8)
    with pytest.raises(ValueError):
        p._check_budget(9)
    for moves, its in ((-1, 1), (1, -1)):
        with pytest.raises(ValueError):
            p.play(moves, its)


def test_pick_moves_and_restart_reject_bad_arguments_before_touching_a_device():
    import torch

    s = hostless_search()
    for g in (torch.zeros(3, dtype=torch.uint8), torch.zeros(5, dtype=torch.bool), [True, False], "all", 0.5):
        with pytest.raises(ValueError):
            s.pick_moves(greedy=g)
    for out in ((torch.zeros(4, dtype=torch.int8),), (torch.zeros(4, dtype=torch.int8), torch.zeros(4, 5), torch.zeros(5)),
                (torch.zeros(4, dtype=torch.int64), torch.zeros(4, 5), torch.zeros(4)),
                (torch.zeros(4, dtype=torch.int8), torch.zeros(4, 3), torch.zeros(4)),
                (torch.zeros(4, dtype=torch.int8), torch.zeros(5, 4).t(), torch.zeros(4))):
        with pytest.raises(ValueError):
            s.pick_moves(out=out)
    for m in (torch.zeros(3, dtype=torch.uint8), torch.zeros(5, dtype=torch.bool), [1, 0, 1]):
        with pytest.raises(ValueError):
            s.restart(m)
    with pytest.raises(ValueError):
        s.restart(torch.zeros(4, dtype=torch.uint8), rows=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        s.restart(torch.zeros(4, dtype=torch.uint8), rows=torch.zeros(4))
    with pytest.raises(ValueError):
        hostless_search(trees=8, num_envs=4).restart(torch.zeros(8, dtype=torch.uint8))  # more trees than env rows: rows must be given


# ---- the sampler's rule, in numpy ---------------------------------------------------------------------------------------------------
def draw(w, visits):
    """The header's statement: u = (w * total) >> 32, the lowest a with N_0 + ... + N_a > u.  w uint32 [n], visits [n, A] or [A]."""
    n = np.asarray(visits, np.uint64)
    total = n.sum(-1)
    u = (np.asarray(w, np.uint64) * total) >> np.uint64(32)
    return (np.cumsum(n, -1) <= u[..., None]).sum(-1), u, total


def test_the_sampling_rule_lands_inside_the_total_and_never_draws_an_unvisited_action():
    rng = np.random.default_rng(7)
    for A in (3, 5, 8):
        visits = rng.integers(0, 1 << rng.integers(1, 31, size=(4000, 1)), size=(4000, A))
        visits[rng.random((4000, A)) < 0.3] = 0
        visits[visits.sum(1) == 0, rng.integers(0, A)] = 1           # total >= 1: a total of 0 never reaches the draw
        assert visits.sum(1).max() < 1 << 34
        w = rng.integers(0, 1 << 32, size=4000, dtype=np.uint64)
        w[:4] = (0, 1, (1 << 32) - 1, (1 << 32) - 2)                  # the ends of the word's range
        a, u, total = draw(w, visits)
        assert (u < total).all() and (a < A).all()
        assert (visits[np.arange(4000), a] > 0).all()
        first = np.argmax(visits > 0, axis=1)
        last = A - 1 - np.argmax(visits[:, ::-1] > 0, axis=1)
        a0, _, _ = draw(np.zeros(4000, np.uint64), visits)
        a1, _, _ = draw(np.full(4000, (1 << 32) - 1, np.uint64), visits)
        small = total <= 1 << 32                                     # the largest word gives u = total - ceil(total / 2^32): total - 1 here
        assert np.array_equal(a0, first) and np.array_equal(a1[small], last[small]) and small.any()


def test_the_sampling_rule_is_proportional_to_the_visits_over_a_sweep_of_words():
    rng = np.random.default_rng(11)
    sweep = 1 << 16
    w = np.arange(sweep, dtype=np.uint64) << np.uint64(16)           # all 2^16 values of a 16-bit-spaced sweep
    rows = [[1, 1, 1], [3, 0, 5, 0, 1], [0, 0, 0, 0, 0, 0, 0, 9], [100, 1, 0, 7, 31, 2, 0, 59], [1, 65535, 1], [16, 16, 16, 16, 16]]
    rows += [list(rng.integers(0, 4000, size=A)) for A in (3, 5, 8) for _ in range(6)]
    for visits in rows:
        visits = np.asarray(visits, np.int64)
        if visits.sum() == 0:
            continue
        a, _, total = draw(w, np.broadcast_to(visits, (sweep, len(visits))))
        counts = np.bincount(a, minlength=len(visits))
        want = visits.astype(np.float64) / float(total[0]) * sweep
        assert np.abs(counts - want).max() <= 1.0, (visits, counts, want)
        assert (counts[visits == 0] == 0).all()
