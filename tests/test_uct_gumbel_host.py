"""Host: the entry points of the Gumbel root search (snac_uct_select_gumbel, snac_uct_gumbel_candidates) are exported and check every
argument before any HIP call -- each failing call below fails its checks first, so the placeholder pointers are never dereferenced --
UCTSearch and SelfPlay reject a Gumbel configuration they cannot run before they allocate anything (no device is needed for that), and
gumbel_schedule() splits a budget into halving phases."""
import ctypes as C

import pytest

from cabi_checks import PH, _err, _fn, _NoDeviceOfFour
from snac_amd import _lib

OFF8 = C.c_void_p((1 << 20) + 8)                                     # 8-byte aligned only: not a bounds array
OFF64 = C.c_void_p((1 << 20) + 64)                                   # 16-byte aligned, not 128: not a statistics array
INT_MAX = 0x7FFFFFFF
BEGIN, HALVE, PICK = 0, 1, 2


def _select(L, A=5, stats=PH, rows=100, B=4, cap=8, K=3, vl=0.5, fpv=0.0, tlen=16, stab=PH, itab=PH, slots=PH, first=PH, bounds=PH, cand=PH,
            offset=0):
    return L.snac_uct_select_gumbel(A, stats, rows, B, cap, K, 1.25, vl, fpv, stab, itab, tlen, slots, slots, slots, slots, slots, slots, slots,
                                    first, bounds, cand, offset, None)


def _cands(L, A=5, stats=PH, rows=100, B=4, cap=8, mode=HALVE, m=4, scores=PH, c_visit=50.0, c_scale=1.0, fpv=0.0, bounds=PH, cand=PH, action=PH):
    return L.snac_uct_gumbel_candidates(A, stats, rows, B, cap, mode, m, scores, c_visit, c_scale, fpv, bounds, cand, action, None)


def test_the_library_exports_the_gumbel_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    for n, k in (("snac_uct_select_gumbel", 24), ("snac_uct_gumbel_candidates", 15)):
        assert n in _lib.EXPORTS
        assert getattr(L, n) is not None
        assert len(getattr(L, n).argtypes) == k
    assert len(L.snac_uct_select_gumbel.argtypes) == len(L.snac_uct_select_puct_norm.argtypes) + 2        # cand and offset before the stream


def test_select_gumbel_runs_the_checks_of_select_puct_norm():
    L = _lib.lib()
    for A in (0, 4, 9):
        _err(L, _select(L, A=A), b"num_actions")
    _err(L, _select(L, stats=None), b"null stats")
    _err(L, _select(L, stats=OFF64), b"128-byte")
    _err(L, _select(L, B=-3), b"B must be")
    _err(L, _select(L, cap=0), b"cap must be")
    _err(L, _select(L, K=-2), b"paths must be")
    _err(L, _select(L, rows=4 * 9, K=2), b"exceed stats_rows")
    _err(L, _select(L, B=1 << 16, cap=1, K=1 << 15, rows=INT_MAX), b"exceed int32")
    for x in (float("nan"), float("inf")):
        _err(L, _select(L, vl=x), b"virtual_loss")
        _err(L, _select(L, fpv=x), b"first_play_value")
    _err(L, _select(L, stab=None), b"null sqrt_table")
    _err(L, _select(L, itab=None), b"inv_table")
    _err(L, _select(L, tlen=0), b"table_len")
    _err(L, _select(L, slots=None), b"null per-slot")
    _err(L, _select(L, first=None), b"null per-slot")
    _err(L, _select(L, bounds=None), b"null bounds")
    _err(L, _select(L, bounds=OFF8), b"16-byte")
    _err(L, _select(L, fpv=float("nan"), bounds=None, cand=None), b"first_play_value")       # the inherited checks come first
    _err(L, _select(L, bounds=None, cand=None), b"null bounds")


def test_select_gumbel_checks_cand_and_offset():
    L = _lib.lib()
    _err(L, _select(L, cand=None), b"null cand")
    _err(L, _select(L, offset=-1), b"offset must be")
    _err(L, _select(L, offset=INT_MAX), b"offset + paths")
    _err(L, _select(L, offset=INT_MAX - 2, K=3), b"offset + paths")   # 2^31 - 3 + 3 = 2^31: one past int32
    _err(L, _select(L, offset=INT_MAX - 3, K=3, cand=None), b"null cand")        # 2^31 - 1 is inside: the call fails on cand alone


def test_gumbel_candidates_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    for mode in (BEGIN, HALVE, PICK):
        for A in (0, 4, 9):
            _err(L, _cands(L, mode=mode, A=A), b"num_actions")
        _err(L, _cands(L, mode=mode, stats=None), b"null stats")
        _err(L, _cands(L, mode=mode, stats=OFF64), b"128-byte")
        _err(L, _cands(L, mode=mode, B=0), b"B must be")
        _err(L, _cands(L, mode=mode, cap=0), b"cap must be")
        _err(L, _cands(L, mode=mode, rows=4 * 9 - 1), b"exceed stats_rows")      # B * (cap + 1) = 36 rows needed
        _err(L, _cands(L, mode=mode, B=1 << 16, cap=1 << 15, rows=INT_MAX), b"exceed int32")
        _err(L, _cands(L, mode=mode, scores=None), b"null scores")
        for x in (float("nan"), float("inf"), float("-inf")):
            _err(L, _cands(L, mode=mode, c_visit=x), b"c_visit")
            _err(L, _cands(L, mode=mode, c_scale=x), b"c_scale")
            _err(L, _cands(L, mode=mode, fpv=x), b"first_play_value")
        _err(L, _cands(L, mode=mode, cand=None), b"null cand")
    for mode in (-1, 3, 7):
        _err(L, _cands(L, mode=mode), b"mode must be")
    for m in (0, -2):
        _err(L, _cands(L, mode=BEGIN, m=m), b"m must be")
    for mode in (HALVE, PICK):
        _err(L, _cands(L, mode=mode, bounds=None), b"null bounds")
        _err(L, _cands(L, mode=mode, bounds=OFF8), b"16-byte")
        _err(L, _cands(L, mode=mode, bounds=C.c_void_p((1 << 20) + 4)), b"16-byte")
    _err(L, _cands(L, mode=PICK, action=None), b"null action")
    # what a mode does not use is not checked for it: these calls fail on the one argument that IS wrong
    _err(L, _cands(L, mode=BEGIN, bounds=None, action=None, cand=None), b"null cand")
    _err(L, _cands(L, mode=HALVE, m=0, action=None, cand=None), b"null cand")


@pytest.mark.parametrize("kw", [dict(gumbel=4), dict(gumbel=4, evaluator=_fn), dict(gumbel=4, q_normalise=True),
                                dict(gumbel=0, evaluator=_fn, q_normalise=True), dict(gumbel=-3, evaluator=_fn, q_normalise=True),
                                dict(gumbel=2.0, evaluator=_fn, q_normalise=True), dict(gumbel="4", evaluator=_fn, q_normalise=True),
                                dict(gumbel=True, evaluator=_fn, q_normalise=True),
                                dict(gumbel=4, evaluator=_fn, q_normalise=True, gumbel_c_visit=float("nan")),
                                dict(gumbel=4, evaluator=_fn, q_normalise=True, gumbel_c_scale=float("inf"))])
def test_uctsearch_rejects_a_gumbel_search_it_cannot_run_before_allocating(kw):
    from snac_amd import UCTSearch

    args = dict(nodes_per_tree=16, horizon=0, gamma=0.9)
    args.update(kw)
    with pytest.raises(ValueError, match="[gG]umbel"):
        UCTSearch(_NoDeviceOfFour(), **args)


class _Search:
    """Enough of a search for SelfPlay to reach its argument checks."""
    evaluator = staticmethod(_fn)

    def __init__(self, gumbel):
        self.gumbel = gumbel

    def __getattr__(self, name):
        raise AssertionError("SelfPlay touched search.%s before it rejected its arguments" % name)


def test_selfplay_rejects_a_gumbel_mode_it_cannot_run_before_allocating():
    from snac_amd import SelfPlay

    with pytest.raises(ValueError, match="[gG]umbel"):
        SelfPlay(_Search(None), 8, gumbel=True)                      # not a Gumbel search
    with pytest.raises(ValueError, match="root_noise"):
        SelfPlay(_Search(4), 8, gumbel=True, root_noise=lambda p: p)
    with pytest.raises(ValueError, match="gumbel"):
        SelfPlay(_Search(4), 8, gumbel=1)                            # a bool
    with pytest.raises(ValueError, match="generator"):
        SelfPlay(_Search(None), 8, generator=object())               # the generator belongs to the Gumbel mode


def test_gumbel_run_before_gumbel_begin_raises():
    """The host-side flag alone decides: nothing of the device is touched before the error."""
    from snac_amd import UCTSearch

    s = object.__new__(UCTSearch)
    s.gumbel, s._gumbel_begun, s._iteration, s.max_iterations = 4, False, 0, 64
    with pytest.raises(ValueError, match="gumbel_begin"):
        s.gumbel_run(6)
    s.gumbel = None
    with pytest.raises(ValueError, match="gumbel=m"):
        s.gumbel_run(6)


def test_gumbel_schedule():
    from snac_amd.uct import gumbel_schedule

    F, T = False, True
    assert gumbel_schedule(7, 4) == [(F, 0), (F, 1), (F, 2), (T, 0), (F, 1), (F, 2), (F, 3)]
    assert gumbel_schedule(3, 8) == [(F, 0), (T, 0), (T, 0)]
    assert gumbel_schedule(5, 1) == [(F, i) for i in range(5)] == gumbel_schedule(5, 2)
    for m, phases in ((1, 1), (2, 1), (3, 2), (4, 2), (5, 3), (8, 3)):
        for n in range(phases):
            with pytest.raises(ValueError):
                gumbel_schedule(n, m)
        assert len(gumbel_schedule(phases, m)) == phases
    with pytest.raises(ValueError):
        gumbel_schedule(4, 0)


@pytest.mark.parametrize("m", range(1, 9))
def test_gumbel_schedule_phases_sum_to_the_budget(m):
    from snac_amd.uct import gumbel_schedule

    phases = max(1, (m - 1).bit_length())
    for n in range(phases, 21):
        plan = gumbel_schedule(n, m)
        assert len(plan) == n and plan[0] == (False, 0)
        starts = [j for j, (h, i) in enumerate(plan) if i == 0]
        assert len(starts) == phases and [plan[j][0] for j in starts] == [False] + [True] * (phases - 1)
        lengths = [b - a for a, b in zip(starts, starts[1:] + [n])]
        assert sum(lengths) == n and lengths[:-1] == [n // phases] * (phases - 1) and lengths[-1] == n - (n // phases) * (phases - 1)
        for a, ln in zip(starts, lengths):                           # inside a phase: i counts up, and only its first iteration may halve
            assert [i for _, i in plan[a:a + ln]] == list(range(ln)) and not any(h for h, _ in plan[a + 1:a + ln])
        cands = m                                                    # the halvings leave two candidates (one where m == 1)
        for _ in range(phases - 1):
            cands = (cands + 1) // 2
        assert cands == min(m, 2)
