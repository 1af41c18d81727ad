"""Host: action distributions of the counter RNG (include/snac_hip.h "Counter RNG", snac_action_dist, snac_env_desc.action_dist) --
the thresholds built from weights, a numpy statement of the draw (the uniform table draws exactly the multiply's actions), the weight
checks, and the table behind the C ABI: interning, capacity, and the descriptor checks (through snac_obs_dim: no device needed)."""
import ctypes as C
import math

import numpy as np
import pytest

import rng_spec
from snac_amd import _lib

MIX3D = [0.2] * 4 + [0.05] * 4                                      # Env/3D/DMP_simulator_3d_static_circle.py:361-362


def draw(w, cdf):
    """action = #{ j < A-1 : (w >> 16) >= cdf[j] }"""
    u = (np.asarray(w, np.uint64) >> np.uint64(16))[..., None]
    return (u >= np.asarray(cdf, np.uint64)).sum(-1).astype(np.int8)


def _desc(kind, handle):
    return _lib.EnvDesc(kind, 1, 16, 4, 0, 0, 1, 0, 0, 0, 0, 0, 0, handle)


@pytest.mark.parametrize("A", [3, 5, 8])
def test_uniform_weights_give_the_ceiling_table(A):
    cdf = _lib.action_cdf([1.0] * A, A)
    assert cdf.dtype == np.uint32
    assert cdf.tolist() == [math.ceil(65536 * (j + 1) / A) for j in range(A - 1)]
    assert _lib.action_cdf([7.5] * A, A).tolist() == cdf.tolist()


def test_zero_weights_give_empty_intervals():
    cdf = _lib.action_cdf([1, 0, 1, 0, 0], 5)
    assert cdf.tolist() == [32768, 32768, 65536, 65536]
    w = rng_spec.words(3, rng_spec.STREAM_STEP, np.arange(64, dtype=np.uint64)[:, None], np.arange(4096, dtype=np.uint64))
    assert set(np.unique(draw(w, cdf)).tolist()) == {0, 2}
    assert _lib.action_cdf([0, 0, 1], 3).tolist() == [0, 0]              # only the last action
    assert _lib.action_cdf([1, 0, 0], 3).tolist() == [65536, 65536]      # only the first


def test_the_reference_tables():
    # the 3D mix: cumulative 0.2 .. 0.8, then 0.85, 0.9, 0.95 (float64 sums, rounded up)
    assert _lib.action_cdf(MIX3D, 8).tolist() == [13108, 26215, 39322, 52429, 55706, 58983, 62260]
    # randint(3) over a kind's action_dim (multiprocess.py's reference actions)
    assert _lib.action_cdf([1, 1, 1], 3).tolist() == [21846, 43691]
    assert _lib.action_cdf([1, 1, 1, 0, 0], 5).tolist() == [21846, 43691, 65536, 65536]
    assert _lib.action_cdf([1, 1, 1, 0, 0, 0, 0, 0], 8).tolist() == [21846, 43691] + [65536] * 5


@pytest.mark.parametrize("A", [3, 5, 8])
def test_the_uniform_table_draws_the_multiply_over_a_million_words(A):
    env = np.arange(1000, dtype=np.uint64)[:, None] + np.uint64(1 << 33)
    w = rng_spec.words(12345, rng_spec.STREAM_STEP, env, np.arange(1000, dtype=np.uint64))
    assert w.size == 10 ** 6
    assert np.array_equal(draw(w, _lib.action_cdf([1] * A, A)), rng_spec.action_of(w, A))
    u = np.arange(65536, dtype=np.uint64) << np.uint64(16)             # every value of the high half
    assert np.array_equal(draw(u, _lib.action_cdf([1] * A, A)), rng_spec.action_of(u, A))


def test_the_draw_follows_the_thresholds():
    cdf = _lib.action_cdf(MIX3D, 8)
    u = np.arange(65536, dtype=np.uint64)
    counts = np.bincount(draw(u << np.uint64(16), cdf), minlength=8)
    assert counts.tolist() == np.diff(np.concatenate([[0], cdf.astype(np.int64), [65536]])).tolist()


@pytest.mark.parametrize("probs,words", [([1, 1], "3 weights"), ([1, 1, 1, 1], "3 weights"), ([1, -1, 1], "non-negative"),
                                         ([1, float("nan"), 1], "finite"), ([1, float("inf"), 1], "finite"), ([0, 0, 0], "positive sum")])
def test_bad_weights_are_refused(probs, words):
    with pytest.raises(ValueError, match=words):
        _lib.action_cdf(probs, 3)


def test_the_library_exports_the_entry_point():
    assert "snac_action_dist" in _lib.EXPORTS
    assert _lib.lib().snac_action_dist is not None
    assert [f for f, _ in _lib.EnvDesc._fields_][-1] == "action_dist"
    assert C.sizeof(_lib.EnvDesc) == 64                                 # the ABI-12 layout


def test_the_same_table_gets_the_same_handle():
    a = _lib.action_dist(5, [100, 200, 300, 400])
    b = _lib.action_dist(5, [100, 200, 300, 401])
    assert a >= 1 and b >= 1 and a != b
    assert _lib.action_dist(5, [100, 200, 300, 400]) == a
    assert _lib.action_dist(5, np.array([100, 200, 300, 400], np.uint32)) == a
    c = _lib.action_dist(3, [100, 200])
    assert c not in (a, b)


def test_the_entry_point_checks_its_arguments():
    L = _lib.lib()
    h = C.c_int32(-7)

    def call(A, vals, handle=C.byref(h)):
        arr = (C.c_uint32 * 8)(*vals) if vals is not None else None
        return L.snac_action_dist(A, arr, handle)

    for A, vals in ((1, [0]), (9, [0] * 8), (3, [2, 1]), (3, [0, 65537]), (5, [1, 2, 70000, 3])):
        assert call(A, vals) == -1                                    # SNAC_ERR_ARG
        assert L.snac_last_error()
    assert call(3, None) == -1
    assert call(3, [1, 2], None) == -1
    assert h.value == -7
    assert call(3, [0, 65536]) == 0 and h.value >= 1


def test_the_table_has_a_fixed_capacity():
    """A fresh process fills the table: 1024 distinct entries, then SNAC_ERR_ARG; known tables still resolve."""
    import os
    import subprocess
    import sys

    code = r"""
import sys
sys.path[:0] = %r
from snac_amd import _lib
L = _lib.lib()
hs = [_lib.action_dist(8, [j, 65536, 65536, 65536, 65536, 65536, 65536]) for j in range(1024)]
assert hs == list(range(1, 1025)), hs[:4]
try:
    _lib.action_dist(8, [1024] + [65536] * 6)
except _lib.SnacError as e:
    assert "full" in str(e)
else:
    raise AssertionError("past the capacity")
assert _lib.action_dist(8, [5] + [65536] * 6) == 6
print("ok")
""" % ([os.path.dirname(os.path.dirname(os.path.abspath(__file__)))],)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().endswith("ok")


def test_the_descriptor_checks_the_handle():
    L = _lib.lib()
    h3 = _lib.action_dist(3, _lib.action_cdf([1, 2, 3], 3))
    h8 = _lib.action_dist(8, _lib.action_cdf(MIX3D, 8))
    assert L.snac_obs_dim(C.byref(_desc(1, 0))) == 7
    assert L.snac_obs_dim(C.byref(_desc(1, h3))) == 7
    assert L.snac_obs_dim(C.byref(_desc(3, h8))) == 51
    for kind, h in ((2, h3), (2, h8), (3, h3), (1, h8)):
        assert L.snac_obs_dim(C.byref(_desc(kind, h))) == -1
        assert b"num_actions" in L.snac_last_error()
    for h in (1 << 20, -1, -5):
        assert L.snac_obs_dim(C.byref(_desc(2, h))) == -1
        assert b"action_dist" in L.snac_last_error()
