"""Host: the entry points of the normalised search (snac_uct_select_paths_norm, snac_uct_select_puct_norm, snac_uct_backup_paths_norm,
snac_uct_bounds) are exported and check every argument before any HIP call -- each failing call below fails its checks first, so the
placeholder pointers are never dereferenced -- and UCTSearch rejects a `q_normalise` that is not a bool before it allocates anything
(no device is needed for that)."""
import ctypes as C

import pytest

from cabi_checks import PH, _err, _fn, _NoDeviceOfFour
from snac_amd import _lib

OFF8 = C.c_void_p((1 << 20) + 8)                                     # 8-byte aligned only: not a bounds array
OFF64 = C.c_void_p((1 << 20) + 64)                                   # 16-byte aligned, not 128: not a statistics array


def _select(L, A=5, stats=PH, rows=100, B=4, cap=8, K=3, vl=0.5, tlen=16, ltab=PH, rtab=PH, slots=PH, first=PH, bounds=PH):
    return L.snac_uct_select_paths_norm(A, stats, rows, B, cap, K, 1.4, vl, ltab, rtab, tlen, slots, slots, slots, slots, slots, slots, slots,
                                        first, bounds, None)


def _puct(L, A=5, stats=PH, rows=100, B=4, cap=8, K=3, vl=0.5, fpv=0.0, tlen=16, stab=PH, itab=PH, slots=PH, first=PH, bounds=PH):
    return L.snac_uct_select_puct_norm(A, stats, rows, B, cap, K, 1.25, vl, fpv, stab, itab, tlen, slots, slots, slots, slots, slots, slots,
                                       slots, first, bounds, None)


def _backup(L, A=5, stats=PH, rows=100, B=4, cap=8, K=3, slots=PH, est=PH, bounds=PH):
    return L.snac_uct_backup_paths_norm(A, stats, rows, B, cap, K, 0.97, slots, slots, slots, slots, slots, slots, est, bounds, None)


def _bounds(L, stats=PH, rows=100, B=4, cap=8, used=PH, mask=None, bounds=PH):
    return L.snac_uct_bounds(stats, rows, B, cap, used, mask, bounds, None)


def test_the_library_exports_the_normalised_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    for n, k in (("snac_uct_select_paths_norm", 21), ("snac_uct_select_puct_norm", 22), ("snac_uct_backup_paths_norm", 16), ("snac_uct_bounds", 8)):
        assert n in _lib.EXPORTS
        assert getattr(L, n) is not None
        assert len(getattr(L, n).argtypes) == k
    for n in ("snac_uct_select_paths", "snac_uct_select_puct", "snac_uct_backup_paths"):          # the arguments, bounds, the stream
        assert len(getattr(L, n + "_norm").argtypes) == len(getattr(L, n).argtypes) + 1


@pytest.mark.parametrize("call", [_select, _puct, _backup, _bounds])
def test_bounds_must_be_a_16_byte_aligned_array(call):
    L = _lib.lib()
    _err(L, call(L, bounds=None), b"null bounds")
    _err(L, call(L, bounds=OFF8), b"16-byte")
    _err(L, call(L, bounds=C.c_void_p((1 << 20) + 4)), b"16-byte")


def test_select_paths_norm_runs_the_checks_of_select_paths():
    L = _lib.lib()
    for A in (0, 4, 9):
        _err(L, _select(L, A=A), b"num_actions")
    _err(L, _select(L, stats=None), b"null stats")
    _err(L, _select(L, stats=OFF64), b"128-byte")
    _err(L, _select(L, B=0), b"B must be")
    _err(L, _select(L, cap=0), b"cap must be")
    _err(L, _select(L, K=0), b"paths must be")
    _err(L, _select(L, rows=4 * 11 - 1), b"exceed stats_rows")        # B * (cap + K) = 44 rows needed
    _err(L, _select(L, B=1 << 16, cap=1 << 15, rows=0x7FFFFFFF), b"exceed int32")
    _err(L, _select(L, vl=float("nan")), b"virtual_loss")
    _err(L, _select(L, ltab=None), b"null log_table")
    _err(L, _select(L, rtab=None), b"rsqrt_table")
    _err(L, _select(L, tlen=1), b"table_len")
    _err(L, _select(L, slots=None), b"null per-slot")
    _err(L, _select(L, first=None), b"null per-slot")
    _err(L, _select(L, stats=None, bounds=None), b"null stats")       # the inherited checks come first


def test_select_puct_norm_runs_the_checks_of_select_puct():
    L = _lib.lib()
    for A in (0, 4, 9):
        _err(L, _puct(L, A=A), b"num_actions")
    _err(L, _puct(L, stats=None), b"null stats")
    _err(L, _puct(L, stats=OFF64), b"128-byte")
    _err(L, _puct(L, B=-3), b"B must be")
    _err(L, _puct(L, cap=0), b"cap must be")
    _err(L, _puct(L, K=-2), b"paths must be")
    _err(L, _puct(L, rows=4 * 9, K=2), b"exceed stats_rows")
    _err(L, _puct(L, B=1 << 16, cap=1, K=1 << 15, rows=0x7FFFFFFF), b"exceed int32")
    for x in (float("nan"), float("inf")):
        _err(L, _puct(L, vl=x), b"virtual_loss")
        _err(L, _puct(L, fpv=x), b"first_play_value")
    _err(L, _puct(L, stab=None), b"null sqrt_table")
    _err(L, _puct(L, itab=None), b"inv_table")
    _err(L, _puct(L, tlen=0), b"table_len")
    _err(L, _puct(L, slots=None), b"null per-slot")
    _err(L, _puct(L, first=None), b"null per-slot")
    _err(L, _puct(L, fpv=float("nan"), bounds=None), b"first_play_value")


def test_backup_paths_norm_runs_the_checks_of_backup_paths():
    L = _lib.lib()
    for A in (0, 4, 9):
        _err(L, _backup(L, A=A), b"num_actions")
    _err(L, _backup(L, stats=None), b"null stats")
    _err(L, _backup(L, stats=OFF64), b"128-byte")
    _err(L, _backup(L, B=0), b"B must be")
    _err(L, _backup(L, cap=-1), b"cap must be")
    _err(L, _backup(L, K=0), b"paths must be")
    _err(L, _backup(L, rows=4 * 11 - 1), b"exceed stats_rows")
    _err(L, _backup(L, B=1 << 15, cap=1 << 15, K=1 << 15, rows=0x7FFFFFFF), b"exceed int32")
    _err(L, _backup(L, slots=None), b"null per-slot")
    _err(L, _backup(L, est=None), b"null per-slot")
    _err(L, _backup(L, est=None, bounds=None), b"null per-slot")


def test_bounds_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _err(L, _bounds(L, used=None), b"null used")
    _err(L, _bounds(L, stats=None), b"null stats")
    _err(L, _bounds(L, stats=OFF64), b"128-byte")
    _err(L, _bounds(L, B=0), b"B must be")
    _err(L, _bounds(L, B=-1), b"B must be")
    _err(L, _bounds(L, cap=0), b"cap must be")
    _err(L, _bounds(L, rows=4 * 9 - 1), b"exceed stats_rows")         # B * (cap + 1) = 36 rows needed
    _err(L, _bounds(L, B=1 << 16, cap=1 << 15, rows=0x7FFFFFFF), b"exceed int32")
    _err(L, _bounds(L, mask=PH, bounds=None), b"null bounds")        # a mask does not change the checks


@pytest.mark.parametrize("kw", [dict(q_normalise=1), dict(q_normalise="yes"), dict(q_normalise=0), dict(q_normalise=None),
                                dict(q_normalise=1, evaluator=_fn), dict(q_normalise="yes", evaluator=_fn, paths=4)])
def test_uctsearch_rejects_a_q_normalise_that_is_not_a_bool_before_allocating(kw):
    from snac_amd import UCTSearch

    args = dict(nodes_per_tree=16, horizon=0, gamma=0.9)
    args.update(kw)
    with pytest.raises(ValueError, match="q_normalise"):
        UCTSearch(_NoDeviceOfFour(), **args)
