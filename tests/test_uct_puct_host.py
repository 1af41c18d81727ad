"""Host: the PUCT entry points (snac_observe_nodes1d / 2d / 3d, snac_uct_select_puct, snac_uct_set_priors) are exported and check every
argument before any HIP call -- each failing call below fails its checks first, so the placeholder pointers are never dereferenced --
and UCTSearch rejects a bad `evaluator` / `first_play_value` before it allocates anything (no device is needed for that)."""
import ctypes as C

import pytest

from cabi_checks import PH, _desc, _err, _fn, _NoDeviceOfFour
from snac_amd import _lib

OBSERVE = ("snac_observe_nodes1d", "snac_observe_nodes2d", "snac_observe_nodes3d")


def _select(L, A=5, stats=PH, rows=100, B=4, cap=8, K=3, vl=0.5, fpv=0.0, tlen=16, stab=PH, itab=PH, slots=PH, leaf=PH, first=PH):
    return L.snac_uct_select_puct(A, stats, rows, B, cap, K, 1.4, vl, fpv, stab, itab, tlen, slots, slots, slots, slots, leaf, slots, slots,
                                  first, None)


def _priors(L, A=5, stats=PH, rows=100, m=4, idx=PH, priors=PH, only=0):
    return L.snac_uct_set_priors(A, stats, rows, m, idx, priors, only, None)


def test_the_library_exports_the_puct_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    for n, k in (("snac_observe_nodes1d", 8), ("snac_observe_nodes2d", 8), ("snac_observe_nodes3d", 8), ("snac_uct_select_puct", 21),
                 ("snac_uct_set_priors", 8)):
        assert n in _lib.EXPORTS
        assert getattr(L, n) is not None
        assert len(getattr(L, n).argtypes) == k


def test_select_puct_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    for A in (0, 2, 4, 6, 7, 9):
        _err(L, _select(L, A=A), b"num_actions")
    _err(L, _select(L, stats=None), b"null stats")
    _err(L, _select(L, B=0), b"B must be")
    _err(L, _select(L, B=-3), b"B must be")
    _err(L, _select(L, cap=0), b"cap must be")
    _err(L, _select(L, K=0), b"paths must be")
    _err(L, _select(L, K=-2), b"paths must be")
    _err(L, _select(L, rows=4 * 11 - 1), b"exceed stats_rows")        # B * (cap + K) = 44 rows needed
    _err(L, _select(L, rows=4 * 9, K=2), b"exceed stats_rows")
    _err(L, _select(L, B=1 << 16, cap=1 << 15, rows=0x7FFFFFFF), b"exceed int32")
    _err(L, _select(L, B=1 << 16, cap=1, K=1 << 15, rows=0x7FFFFFFF), b"exceed int32")       # B * paths slots
    _err(L, _select(L, B=1 << 15, cap=1 << 15, K=1 << 15, rows=0x7FFFFFFF), b"exceed int32")  # B * (cap + paths) rows
    _err(L, _select(L, stats=C.c_void_p((1 << 20) + 64)), b"128-byte")
    _err(L, _select(L, slots=None), b"null per-slot")
    _err(L, _select(L, leaf=None), b"null per-slot")
    _err(L, _select(L, first=None), b"null per-slot")
    _err(L, _select(L, tlen=1), b"table_len")
    _err(L, _select(L, tlen=0), b"table_len")
    _err(L, _select(L, stab=None), b"null sqrt_table")
    _err(L, _select(L, itab=None), b"inv_table")
    for x in (float("nan"), float("inf"), float("-inf")):
        _err(L, _select(L, vl=x), b"virtual_loss")
        _err(L, _select(L, fpv=x), b"first_play_value")
    assert _select(L, K=1, rows=4 * 9 - 1) == -1                     # one path per tree: B * (cap + 1) rows


def test_set_priors_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    for A in (0, 2, 4, 6, 7, 9):
        _err(L, _priors(L, A=A), b"num_actions")
    _err(L, _priors(L, stats=None), b"null stats")
    _err(L, _priors(L, stats=C.c_void_p((1 << 20) + 64)), b"128-byte")
    _err(L, _priors(L, rows=0), b"stats_rows")
    _err(L, _priors(L, m=-1), b"m must be")
    _err(L, _priors(L, idx=None), b"null rows")
    _err(L, _priors(L, priors=None), b"priors")
    assert _priors(L, m=0) == 0                                      # nothing to do: no launch


def _observe(L, name, d, st, pool, pool_rows, m, idx=None, obs=PH):
    return getattr(L, name)(C.byref(d) if d is not None else None, C.byref(st) if st is not None else None, pool, pool_rows, m, idx, obs, None)


@pytest.mark.parametrize("name", OBSERVE)
def test_observe_nodes_validates_its_arguments_before_any_hip_call(name):
    L = _lib.lib()
    kind = int(name[-2])
    st = _lib.State(*[1 << 20] * 8)
    d = _desc(kind)

    def err(rc, *words):
        assert rc != 0, name
        msg = L.snac_last_error()
        assert any(w in msg for w in words), (name, msg)
        return rc

    err(_observe(L, name, None, st, PH, 16, 4), b"null")
    err(_observe(L, name, d, None, PH, 16, 4), b"null")
    err(_observe(L, name, d, st, None, 16, 4), b"null")               # null pool
    err(_observe(L, name, d, st, PH, 16, 4, obs=None), b"null obs")
    err(_observe(L, name, d, st, C.c_void_p((1 << 20) + 64), 16, 4), b"128-byte")
    for k in (1, 2, 3):
        if k != kind:
            assert err(_observe(L, name, _desc(k), st, PH, 16, 4), b"records are for the %dD kinds" % kind) == -3
    err(_observe(L, name, d, st, PH, 0, 4), b"pool_rows")
    err(_observe(L, name, d, st, PH, 16, -1), b"m must be")
    err(_observe(L, name, d, st, PH, 8, 9), b"exceeds")               # no index array: m may not exceed the pool
    variant = _desc(kind)
    variant.obs_scalars = _lib.SCALARS_RAW                            # a dynamic desc with raw counters: a layout variant
    assert err(_observe(L, name, variant, st, PH, 16, 4), b"canonical") == -3
    if kind == 1:
        assert err(_observe(L, name, _desc(kind, frame_value=2), st, PH, 16, 4), b"canonical") == -3


@pytest.mark.parametrize("kw", [dict(evaluator=3), dict(evaluator="net"), dict(evaluator=_fn, first_play_value=float("nan")),
                                dict(evaluator=_fn, first_play_value=float("inf")), dict(evaluator=_fn, first_play_value=float("-inf")),
                                dict(first_play_value=0.0), dict(first_play_value=-1.5), dict(evaluator=_fn, paths=0),
                                dict(evaluator=_fn, virtual_loss=float("nan")), dict(evaluator=_fn, paths=1 << 30, trees=4)])
def test_uctsearch_rejects_bad_evaluator_arguments_before_allocating(kw):
    from snac_amd import UCTSearch

    args = dict(nodes_per_tree=16, horizon=0, gamma=0.9)
    args.update(kw)
    with pytest.raises(ValueError):
        UCTSearch(_NoDeviceOfFour(), **args)
