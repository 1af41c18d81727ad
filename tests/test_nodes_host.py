"""Host: the 1D / 3D node-pool entry points (snac_nodes{1,3}d_pack / _unpack, snac_transition_nodes{1,3}d) are exported and check their
arguments before any HIP call -- every call below fails its checks first, so placeholder pointers are never dereferenced."""
import ctypes as C

import pytest

from cabi_checks import _desc
from snac_amd import _lib

NAMES = ("snac_nodes1d_pack", "snac_nodes1d_unpack", "snac_transition_nodes1d", "snac_nodes3d_pack", "snac_nodes3d_unpack", "snac_transition_nodes3d")


def _call(L, name, d, st, pool, pool_rows, m, idx=None):
    """One call of entry `name` with m rows / edges and no index arrays unless idx is given (then for both)."""
    vp = C.c_void_p
    dp = C.byref(d) if d is not None else None
    sp = C.byref(st) if st is not None else None
    if name.endswith("_pack"):
        return getattr(L, name)(dp, sp, idx, m, pool, pool_rows, idx, None)
    if name.endswith("_unpack"):
        return getattr(L, name)(dp, pool, pool_rows, idx, m, sp, idx, None)
    return getattr(L, name)(dp, sp, pool, pool_rows, m, idx, idx, 0, None, None, None, None, None, vp(None))


def test_the_library_exports_the_node_pool_entry_points():
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.EXPORTS
        assert getattr(L, n) is not None


@pytest.mark.parametrize("name", NAMES)
def test_node_entry_points_validate_their_arguments_before_any_hip_call(name):
    L = _lib.lib()
    kind = 1 if "1d" in name else 3
    other = [k for k in (1, 2, 3) if k != kind]
    st = _lib.State(*[1 << 20] * 8)
    pool = C.c_void_p(1 << 20)                                       # 128-byte aligned placeholder
    d = _desc(kind)

    def err(rc, *words):
        assert rc != 0, name
        msg = L.snac_last_error()
        assert any(w in msg for w in words), (name, msg)
        return rc

    err(_call(L, name, None, st, pool, 16, 4), b"null")
    err(_call(L, name, d, None, pool, 16, 4), b"null")
    err(_call(L, name, d, st, None, 16, 4), b"null")
    err(_call(L, name, d, st, C.c_void_p((1 << 20) + 64), 16, 4), b"128-byte")
    for k in other:
        assert err(_call(L, name, _desc(k), st, pool, 16, 4), b"records are for the %dD kinds" % kind) == -3
    err(_call(L, name, d, st, pool, 0, 4), b"pool_rows")
    err(_call(L, name, d, st, pool, 16, -1), b"m must be")
    err(_call(L, name, d, st, pool, 8, 9), b"exceeds")              # no index arrays: m may not exceed the pool ...
    if not name.startswith("snac_transition"):
        err(_call(L, name, _desc(kind, n=8), st, pool, 64, 9), b"exceeds")   # ... nor the batch
    variant = _desc(kind)
    variant.obs_scalars = _lib.SCALARS_RAW                            # a dynamic desc with raw counters: a layout variant
    assert err(_call(L, name, variant, st, pool, 16, 4), b"canonical") == -3
    if kind == 1:
        assert err(_call(L, name, _desc(kind, frame_value=2), st, pool, 16, 4), b"canonical") == -3
