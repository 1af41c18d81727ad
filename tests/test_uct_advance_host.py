"""Host: re-rooting after a move (snac_uct_advance) is exported and checks every argument before any HIP call -- each failing call
below fails its checks first, so the placeholder pointers are never dereferenced."""
import ctypes as C

from snac_amd import _lib

PH = C.c_void_p(1 << 20)                                             # 128-byte aligned placeholder


def _advance(L, A=5, stats=PH, rows=100, B=4, cap=8, records=PH, record_bytes=128, record_rows=100, slots=PH, used=PH, work=PH):
    return L.snac_uct_advance(A, stats, rows, B, cap, records, record_bytes, record_rows, slots, slots, slots, used, work, slots, slots, None)


def test_the_library_exports_the_advance_entry_point():
    L = _lib.lib()
    assert "snac_uct_advance" in _lib.EXPORTS
    assert L.snac_uct_advance is not None
    assert len(L.snac_uct_advance.argtypes) == 16


def test_advance_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()

    def err(rc, *words):
        assert rc == -1, rc
        msg = L.snac_last_error()
        assert any(w in msg for w in words), msg

    for A in (0, 2, 4, 6, 7, 9):
        err(_advance(L, A=A), b"num_actions")
    err(_advance(L, stats=None), b"null stats")
    err(_advance(L, B=0), b"B must be")
    err(_advance(L, B=-3), b"B must be")
    err(_advance(L, cap=0), b"cap must be")
    err(_advance(L, rows=4 * 9 - 1), b"exceed stats_rows")            # B * (cap + 1) = 36 rows needed
    err(_advance(L, B=1 << 16, cap=1 << 15, rows=0x7FFFFFFF, record_rows=0x7FFFFFFF), b"exceed int32")
    err(_advance(L, stats=C.c_void_p((1 << 20) + 64)), b"128-byte")
    err(_advance(L, records=None), b"null records")
    err(_advance(L, records=C.c_void_p((1 << 20) + 16)), b"records must be 128-byte")
    for rb in (0, 64, 127, 256, 512, 895, 1024):
        err(_advance(L, record_bytes=rb), b"record_bytes")
    err(_advance(L, record_rows=4 * 9 - 1), b"exceed record_rows")
    err(_advance(L, record_bytes=896, record_rows=35), b"exceed record_rows")
    err(_advance(L, slots=None), b"null per-tree")
    err(_advance(L, used=None), b"null per-tree")
    err(_advance(L, work=None), b"null work")
