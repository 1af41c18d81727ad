"""CPU: the two host-side pieces behind the ends of a headline pass.  snac_episodic_sums rejects its arguments before any HIP call
(null out3 / scratch, num_envs < 1, null sums), in the manner of tests/test_cabi_host.py; and the tile-order map of k_rollout2d
(snac_amd/csrc/tile_order.h, SNAC_2D_STAGE_XCD) is checked by a stand-alone program (tests/native/tile_order_test.cpp) built with
-fsanitize=address,undefined: every tile taken exactly once, every other wave past the end, for 1 .. 600 tiles in both orders."""
import ctypes as C
import os
import subprocess

import helpers


def test_episodic_sums_validates_its_arguments_before_any_hip_call():
    from snac_amd import _lib

    L = _lib.lib()
    d = _lib.EnvDesc(2, 1, 16, 4, 0, 0, 1, 0, 0, 0)
    st = _lib.State(*[1 << 20] * 8)                                # (aligned, never dereferenced: every call below fails its checks first)
    buf = (C.c_int64 * _lib.SUMS_SCRATCH_WORDS)()
    p = C.cast(buf, C.c_void_p)
    assert L.snac_episodic_sums(C.byref(d), C.byref(st), None, p, None) == -1 and b"null out3 / scratch" in L.snac_last_error()
    assert L.snac_episodic_sums(C.byref(d), C.byref(st), p, None, None) == -1 and b"null out3 / scratch" in L.snac_last_error()
    assert L.snac_episodic_sums(None, C.byref(st), p, p, None) == -1 and L.snac_episodic_sums(C.byref(d), None, p, p, None) == -1
    for n in (0, -5):
        bad = _lib.EnvDesc(2, 1, n, 4, 0, 0, 1, 0, 0, 0)
        assert L.snac_episodic_sums(C.byref(bad), C.byref(st), p, p, None) == -1 and b"num_envs" in L.snac_last_error()
    nul = _lib.State(*[1 << 20] * 6, 0, 1 << 20)
    assert L.snac_episodic_sums(C.byref(d), C.byref(nul), p, p, None) == -1 and b"null pointer" in L.snac_last_error()
    odd = _lib.State(*[1 << 20] * 6, (1 << 20) + 12, 1 << 20)
    assert L.snac_episodic_sums(C.byref(d), C.byref(odd), p, p, None) == -1 and b"aligned" in L.snac_last_error()
    assert all(v == 0 for v in buf)


def test_the_knob_is_the_last_entry_of_the_dispatch_table():
    from snac_amd import _lib

    t = _lib.tuning()
    assert list(t)[-1] == "SNAC_2D_STAGE_XCD" and t["SNAC_2D_STAGE_XCD"][1]
    if "SNAC_2D_STAGE_XCD" not in os.environ:
        assert t["SNAC_2D_STAGE_XCD"][0] in (0, 1, 2)             # never / always / where the grid needs no padding


def test_tile_order_map_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tile_order_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(helpers.ROOT, "snac_amd", "csrc"), os.path.join(helpers.TESTS, "native", "tile_order_test.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "TILE ORDER OK" in r.stdout, (r.stdout[-500:], r.stderr[-500:])
