"""Host: the K-paths-per-tree UCT entry points (snac_uct_select_paths / snac_uct_backup_paths) are exported and check every argument
before any HIP call -- each failing call below fails its checks first, so the placeholder pointers are never dereferenced -- and
UCTSearch rejects a bad `paths` / `virtual_loss` / size before it allocates anything (no device is needed for that)."""
import ctypes as C

import pytest

from cabi_checks import PH, _NoDeviceOfFour
from snac_amd import _lib


def _select(L, A=5, stats=PH, rows=100, B=4, cap=8, K=3, vl=0.5, tlen=16, ltab=PH, rtab=PH, slots=PH, leaf=PH, first=PH):
    return L.snac_uct_select_paths(A, stats, rows, B, cap, K, 1.4, vl, ltab, rtab, tlen, slots, slots, slots, slots, leaf, slots, slots, first,
                                   None)


def _backup(L, A=5, stats=PH, rows=100, B=4, cap=8, K=3, slots=PH, est=PH):
    return L.snac_uct_backup_paths(A, stats, rows, B, cap, K, 0.99, slots, slots, slots, slots, slots, slots, est, None)


def test_the_library_exports_the_multi_path_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    for n, k in (("snac_uct_select_paths", 20), ("snac_uct_backup_paths", 15)):
        assert n in _lib.EXPORTS
        assert getattr(L, n) is not None
        assert len(getattr(L, n).argtypes) == k


@pytest.mark.parametrize("call", [_select, _backup])
def test_multi_path_entry_points_validate_their_arguments_before_any_hip_call(call):
    L = _lib.lib()

    def err(rc, *words):
        assert rc == -1, (call.__name__, rc)
        msg = L.snac_last_error()
        assert any(w in msg for w in words), (call.__name__, msg)

    for A in (0, 2, 4, 6, 7, 9):
        err(call(L, A=A), b"num_actions")
    err(call(L, stats=None), b"null stats")
    err(call(L, B=0), b"B must be")
    err(call(L, B=-3), b"B must be")
    err(call(L, cap=0), b"cap must be")
    err(call(L, K=0), b"paths must be")
    err(call(L, K=-2), b"paths must be")
    err(call(L, rows=4 * 11 - 1), b"exceed stats_rows")                # B * (cap + K) = 44 rows needed
    err(call(L, rows=4 * 9, K=2), b"exceed stats_rows")                # what one path per tree needs is not enough for two
    err(call(L, B=1 << 16, cap=1 << 15, rows=0x7FFFFFFF), b"exceed int32")
    err(call(L, B=1 << 16, cap=1, K=1 << 15, rows=0x7FFFFFFF), b"exceed int32")       # B * paths slots
    err(call(L, B=1 << 15, cap=1 << 15, K=1 << 15, rows=0x7FFFFFFF), b"exceed int32")  # B * (cap + paths) rows
    err(call(L, stats=C.c_void_p((1 << 20) + 64)), b"128-byte")
    err(call(L, slots=None), b"null per-slot")
    if call is _select:
        err(call(L, tlen=1), b"table_len")
        err(call(L, tlen=0), b"table_len")
        err(call(L, ltab=None), b"null log_table")
        err(call(L, rtab=None), b"rsqrt_table")
        err(call(L, leaf=None), b"null per-slot")
        err(call(L, first=None), b"null per-slot")
        for vl in (float("nan"), float("inf"), float("-inf")):
            err(call(L, vl=vl), b"virtual_loss")
    else:
        err(call(L, est=None), b"null per-slot")


@pytest.mark.parametrize("kw", [dict(paths=0), dict(paths=-1), dict(paths=2.5), dict(paths=2, virtual_loss=float("nan")),
                                dict(paths=2, virtual_loss=float("inf")), dict(virtual_loss=float("-inf")),
                                dict(paths=1 << 30, trees=4), dict(paths=2, max_iterations=1 << 30), dict(paths=1 << 29, trees=8)])
def test_uctsearch_rejects_bad_path_arguments_before_allocating(kw):
    from snac_amd import UCTSearch

    args = dict(nodes_per_tree=16, horizon=10, gamma=0.9)
    args.update(kw)
    with pytest.raises(ValueError):
        UCTSearch(_NoDeviceOfFour(), **args)


class _Sharded(_NoDeviceOfFour):
    """_NoDeviceOfFour with a shard's base: the one attribute the key check reads."""

    def __init__(self, env_id_base):
        self.env_id_base = env_id_base


@pytest.mark.parametrize("base,K", [(1 << 62, 2), (1 << 61, 4), ((1 << 63) // 3, 3), ((1 << 62) - 3, 2), (-(1 << 62) - 1, 2), (-(1 << 61) - 1, 4)])
def test_uctsearch_rejects_a_base_whose_slot_keys_leave_int64(base, K):
    """Slot k of tree b draws with key (env_id_base + b) * K + k; with trees = 4 the keys span [base * K, (base + 4) * K)."""
    from snac_amd import UCTSearch

    assert not -(1 << 63) <= base * K <= (base + 4) * K - 1 < 1 << 63
    with pytest.raises(ValueError, match="int64"):
        UCTSearch(_Sharded(base), nodes_per_tree=16, horizon=10, gamma=0.9, paths=K)


@pytest.mark.parametrize("base,K", [((1 << 62) - 4, 2), (-(1 << 62), 2), (1000, 16), ((1 << 63) - 5, 1)])
def test_uctsearch_accepts_a_base_whose_slot_keys_fit_int64(base, K):
    """The key check passes: the constructor goes on to the env's first real attribute, which _NoDeviceOfFour answers with an AssertionError."""
    from snac_amd import UCTSearch

    assert K == 1 or -(1 << 63) <= base * K <= (base + 4) * K - 1 < 1 << 63
    with pytest.raises(AssertionError, match="num_actions"):
        UCTSearch(_Sharded(base), nodes_per_tree=16, horizon=10, gamma=0.9, paths=K)
