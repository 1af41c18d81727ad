"""Host: UCT selection and backup (snac_uct_select / snac_uct_backup) are exported and check every argument before any HIP call -- each
failing call below fails its checks first, so the placeholder pointers are never dereferenced -- and the UCT tables are the python
floats sqrt(log(i)) / 1 / sqrt(i) bit for bit."""
import ctypes as C
import math
import struct

import pytest

from snac_amd import _lib

PH = C.c_void_p(1 << 20)                                             # 128-byte aligned placeholder


def _select(L, A=5, stats=PH, rows=100, B=4, cap=8, tlen=16, ltab=PH, rtab=PH, slots=PH, leaf=PH):
    return L.snac_uct_select(A, stats, rows, B, cap, 1.4, ltab, rtab, tlen, slots, slots, slots, slots, leaf, slots, slots, None)


def _backup(L, A=5, stats=PH, rows=100, B=4, cap=8, slots=PH, est=PH):
    return L.snac_uct_backup(A, stats, rows, B, cap, 0.99, slots, slots, slots, slots, slots, slots, est, None)


def test_the_library_exports_the_uct_entry_points():
    L = _lib.lib()
    for n, k in (("snac_uct_select", 17), ("snac_uct_backup", 14)):
        assert n in _lib.EXPORTS
        assert getattr(L, n) is not None
        assert len(getattr(L, n).argtypes) == k


@pytest.mark.parametrize("call", [_select, _backup])
def test_uct_entry_points_validate_their_arguments_before_any_hip_call(call):
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
    err(call(L, rows=4 * 9 - 1), b"exceed stats_rows")                 # B * (cap + 1) = 36 rows needed
    err(call(L, B=1 << 16, cap=1 << 15, rows=0x7FFFFFFF), b"exceed int32")
    err(call(L, stats=C.c_void_p((1 << 20) + 64)), b"128-byte")
    err(call(L, slots=None), b"null per-tree")
    if call is _select:
        err(call(L, tlen=1), b"table_len")
        err(call(L, tlen=0), b"table_len")
        err(call(L, ltab=None), b"null log_table")
        err(call(L, rtab=None), b"rsqrt_table")
        err(call(L, leaf=None), b"null per-tree")
    else:
        err(call(L, est=None), b"null per-tree")


def test_uct_tables_are_the_python_floats_bit_for_bit():
    import torch

    from snac_amd.uct import uct_tables

    lt, rt = uct_tables(4097)
    assert len(lt) == len(rt) == 4097 and lt[0] == 0.0 and rt[0] == 0.0
    for i in range(1, 4097):
        assert struct.pack("<d", lt[i]) == struct.pack("<d", math.sqrt(math.log(i)))
        assert struct.pack("<d", rt[i]) == struct.pack("<d", 1.0 / math.sqrt(i))
    # and they survive the upload as float64 unchanged
    t = torch.tensor(lt, dtype=torch.float64)
    assert t.numpy().tobytes() == struct.pack("<%dd" % len(lt), *lt)


def test_the_uct_record_layout_matches_the_header():
    """snac_uct_node: 256 bytes; the word offsets uct.py decodes."""
    import os
    import re

    import helpers
    from snac_amd import uct

    src = open(os.path.join(helpers.ROOT, "include", "snac_hip.h")).read()
    body = re.search(r"typedef struct snac_uct_node \{(.*?)\} snac_uct_node;", src, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double|float)\s+(\w+)(?:\[(\d+)\])?;", body, re.M)
    size = {"int32_t": 4, "double": 8, "float": 4}
    off, where = 0, {}
    for ty, name, n in fields:
        where[name] = off
        off += size[ty] * int(n or 1)
    assert off == 256 == uct.WORDS * 4
    assert where == {"child": 0, "child_visits": 32, "child_value": 64, "parent": 128, "action": 132, "terminal": 136, "visits": 140,
                     "value_sum": 144, "reward": 152, "zero": 156}
