"""Host: leaf evaluation on node pools (snac_evaluate_nodes{1,2,3}d) is exported and checks its arguments before any HIP call -- every
failing call below fails its checks first, and m == 0 returns before one, so placeholder pointers are never dereferenced."""
import ctypes as C

import pytest

from cabi_checks import PH, _desc
from snac_amd import _lib

NAMES = ("snac_evaluate_nodes1d", "snac_evaluate_nodes2d", "snac_evaluate_nodes3d")


def _call(L, name, d, st, pool=PH, pool_rows=16, m=4, node_rows=None, H=8, gpow=PH, est=PH, steps=None):
    dp = C.byref(d) if d is not None else None
    sp = C.byref(st) if st is not None else None
    return getattr(L, name)(dp, sp, pool, pool_rows, m, node_rows, H, 0, gpow, est, steps, None)


def test_the_library_exports_the_evaluation_entry_points():
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.EXPORTS
        assert getattr(L, n) is not None
        assert len(getattr(L, n).argtypes) == 12


@pytest.mark.parametrize("name", NAMES)
def test_evaluation_validates_its_arguments_before_any_hip_call(name):
    L = _lib.lib()
    kind = int(name[-2])
    st = _lib.State(*[1 << 20] * 8)
    d = _desc(kind)

    def err(rc, *words):
        assert rc != 0, name
        msg = L.snac_last_error()
        assert any(w in msg for w in words), (name, msg)
        return rc

    assert err(_call(L, name, None, st), b"null") == -1
    assert err(_call(L, name, d, None), b"null") == -1
    assert err(_call(L, name, d, st, pool=None), b"null") == -1
    assert err(_call(L, name, d, st, pool=C.c_void_p((1 << 20) + 64)), b"128-byte") == -1
    for k in (1, 2, 3):
        if k != kind:
            assert err(_call(L, name, _desc(k), st), b"snac_node%dd records are for the %dD kinds" % (kind, kind)) == -3
    assert err(_call(L, name, d, st, pool_rows=0), b"pool_rows") == -1
    assert err(_call(L, name, d, st, m=-1), b"m must be") == -1
    assert err(_call(L, name, d, st, H=-1), b"H must be") == -1
    assert err(_call(L, name, d, st, pool_rows=8, m=9), b"exceeds the pool") == -1    # no node_rows: m may not exceed the pool
    assert err(_call(L, name, d, st, est=None), b"null est") == -1
    assert err(_call(L, name, d, st, gpow=None), b"null gpow") == -1
    variant = _desc(kind)
    variant.obs_scalars = _lib.SCALARS_RAW                            # a dynamic desc with raw counters: a layout variant
    assert err(_call(L, name, variant, st), b"canonical") == -3
    if kind != 3:
        assert err(_call(L, name, _desc(kind, frame_value=2), st), b"canonical") == -3


@pytest.mark.parametrize("name", NAMES)
def test_evaluation_of_no_leaves_returns_before_any_hip_call(name):
    L = _lib.lib()
    kind = int(name[-2])
    st = _lib.State(*[1 << 20] * 8)
    assert _call(L, name, _desc(kind), st, m=0, est=None) == 0
    assert _call(L, name, _desc(kind), st, m=0, H=0, est=None, gpow=None) == 0
    assert _call(L, name, _desc(kind), st, m=0, node_rows=PH, pool_rows=1) == 0


def test_the_existing_node_entry_points_keep_their_messages():
    """nodes_check is now shared with the evaluation: the 1D / 3D messages are unchanged, 2D keeps its own check."""
    L = _lib.lib()
    st = _lib.State(*[1 << 20] * 8)
    rc = L.snac_transition_nodes1d(C.byref(_desc(2)), C.byref(st), PH, 16, 4, None, None, 0, None, None, None, None, None, None)
    assert rc == -3 and L.snac_last_error() == b"snac_node1d records are for the 1D kinds"
    rc = L.snac_transition_nodes3d(C.byref(_desc(3)), C.byref(st), C.c_void_p((1 << 20) + 64), 16, 4, None, None, 0, None, None, None, None, None, None)
    assert rc == -1 and L.snac_last_error() == b"the node pool must be 128-byte aligned (records of whole lines)"
    rc = L.snac_transition_nodes2d(C.byref(_desc(2)), C.byref(st), C.c_void_p((1 << 20) + 64), 16, 4, None, None, 0, None, None, None, None, None, None)
    assert rc == -1 and L.snac_last_error() == b"the node pool must be 128-byte aligned (one record = one line)"
