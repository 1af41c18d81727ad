"""Host: the entry points of the Gumbel interior search (snac_uct_set_priors_value, snac_uct_select_gumbel_interior,
snac_uct_improved_policy) are exported and check every argument before any HIP call -- each failing call below fails its checks first,
so the placeholder pointers are never dereferenced -- UCTSearch rejects a gumbel_interior it cannot run before it allocates anything, and
uct_exp(), the exponential of include/snac_hip.h ("Gumbel interior") restated in python floats (tests/test_gpu_uct_gumbel_interior.py
follows the device with it bit for bit), agrees with math.exp."""
import ctypes as C
import math

import pytest

from cabi_checks import PH, _err, _fn, _NoDeviceOfFour
from snac_amd import _lib

OFF8 = C.c_void_p((1 << 20) + 8)                                     # 8-byte aligned only: not a bounds array
OFF64 = C.c_void_p((1 << 20) + 64)                                   # 16-byte aligned, not 128: not a statistics array
INT_MAX = 0x7FFFFFFF
NOT_FINITE = (float("nan"), float("inf"), float("-inf"))


# ---- uct_exp, restated ----------------------------------------------------------------------------------------------------------------------
LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
COEF = [1.0 / math.factorial(i) for i in range(14)]                  # the float64 quotients 1.0 / i!


def uct_exp(x):
    """exp(x) for x <= 0 in float64 + - *, floor and ldexp alone, every operation rounded on its own, in the header's order."""
    x = float(x)
    if not x >= -700.0:                                              # a NaN too
        return 0.0
    if x > 0.0:
        x = 0.0
    k = float(math.floor(x * LOG2E + 0.5))
    r = (x - k * LN2_HI) - k * LN2_LO
    p = COEF[13]
    for i in range(12, -1, -1):
        p = p * r + COEF[i]
    return math.ldexp(p, int(k))


def test_uct_exp_agrees_with_exp():
    """The margin: the Taylor remainder |r|^14 / 14! is about 4e-18 for |r| <= ln 2 / 2, and about 20 roundings of 1.1e-16 each enter the
    reduction and the Horner sum: within 1e-14 relative."""
    grid = [-700.0 * i / 20000 for i in range(20001)] + [-math.pi * i / 7 for i in range(1500)] + [0.0, -1e-300, -700.0, -0.5 * math.log(2.0)]
    worst = 0.0
    for x in grid:
        assert -700.0 <= x <= 0.0
        want = math.exp(x)
        worst = max(worst, abs(uct_exp(x) - want) / want)
    print("max relative difference from math.exp over %d arguments: %.3g" % (len(grid), worst))
    assert worst <= 1.0e-14
    assert uct_exp(0.0) == 1.0 and uct_exp(-1e-300) == 1.0
    for x in (-700.0000001, -1.0e3, -1.0e300, float("-inf"), float("nan")):
        assert uct_exp(x) == 0.0                                     # below -700 and for a NaN
    for x in (1.0e-9, 3.0, float("inf")):
        assert uct_exp(x) == 1.0                                     # x > 0 reads as 0
    assert 0.0 < uct_exp(-700.0) < 1.0e-300 and uct_exp(-700.0) >= 2.0 ** -1022      # the smallest result is a normal number


# ---- the entry points -------------------------------------------------------------------------------------------------------------------------
def _select(L, A=5, stats=PH, rows=100, B=4, cap=8, K=3, vl=0.5, fpv=0.0, tlen=16, stab=PH, itab=PH, slots=PH, first=PH, bounds=PH, cand=PH,
            offset=0, c_visit=50.0, c_scale=1.0):
    return L.snac_uct_select_gumbel_interior(A, stats, rows, B, cap, K, 1.25, vl, fpv, stab, itab, tlen, slots, slots, slots, slots, slots, slots,
                                             slots, first, bounds, cand, offset, c_visit, c_scale, None)


def _priors(L, A=5, stats=PH, rows=100, m=4, node_rows=PH, priors=PH, value=PH, only_unvisited=0):
    return L.snac_uct_set_priors_value(A, stats, rows, m, node_rows, priors, value, only_unvisited, None)


def _policy(L, A=5, stats=PH, rows=100, B=4, cap=8, m=4, node_rows=PH, c_visit=50.0, c_scale=1.0, bounds=PH, pi=PH):
    return L.snac_uct_improved_policy(A, stats, rows, B, cap, m, node_rows, c_visit, c_scale, bounds, pi, None)


def test_the_library_exports_the_gumbel_interior_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    for n, k in (("snac_uct_set_priors_value", 9), ("snac_uct_select_gumbel_interior", 26), ("snac_uct_improved_policy", 12)):
        assert n in _lib.EXPORTS
        assert getattr(L, n) is not None
        assert len(getattr(L, n).argtypes) == k
    assert len(L.snac_uct_select_gumbel_interior.argtypes) == len(L.snac_uct_select_gumbel.argtypes) + 2    # c_visit, c_scale before the stream
    assert len(L.snac_uct_set_priors_value.argtypes) == len(L.snac_uct_set_priors.argtypes) + 1             # value before only_unvisited


def test_select_gumbel_interior_runs_the_checks_of_select_gumbel_first():
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
    for x in NOT_FINITE[:2]:
        _err(L, _select(L, vl=x), b"virtual_loss")
        _err(L, _select(L, fpv=x), b"first_play_value")
    _err(L, _select(L, stab=None), b"null sqrt_table")
    _err(L, _select(L, itab=None), b"inv_table")
    _err(L, _select(L, tlen=0), b"table_len")
    _err(L, _select(L, slots=None), b"null per-slot")
    _err(L, _select(L, first=None), b"null per-slot")
    _err(L, _select(L, bounds=None), b"null bounds")
    _err(L, _select(L, bounds=OFF8), b"16-byte")
    _err(L, _select(L, cand=None), b"null cand")
    _err(L, _select(L, offset=-1), b"offset must be")
    _err(L, _select(L, offset=INT_MAX - 2, K=3), b"offset + paths")
    # the inherited checks come first, in their order
    _err(L, _select(L, fpv=float("nan"), bounds=None, cand=None, c_visit=float("nan")), b"first_play_value")
    _err(L, _select(L, bounds=None, cand=None, c_scale=float("inf")), b"null bounds")
    _err(L, _select(L, cand=None, c_visit=float("nan")), b"null cand")
    _err(L, _select(L, offset=-1, c_visit=float("nan")), b"offset must be")


def test_select_gumbel_interior_checks_c_visit_and_c_scale():
    L = _lib.lib()
    for x in NOT_FINITE:
        _err(L, _select(L, c_visit=x), b"c_visit")
        _err(L, _select(L, c_scale=x), b"c_scale")
    _err(L, _select(L, offset=INT_MAX - 3, K=3, c_scale=float("nan")), b"c_scale")   # 2^31 - 1 is inside: the call fails on c_scale alone


def test_set_priors_value_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    for A in (0, 4, 9):
        _err(L, _priors(L, A=A), b"num_actions")
    _err(L, _priors(L, stats=None), b"null stats")
    _err(L, _priors(L, rows=0), b"stats_rows")
    _err(L, _priors(L, m=-1), b"m must be")
    _err(L, _priors(L, stats=OFF64), b"128-byte")
    _err(L, _priors(L, node_rows=None), b"null rows")
    _err(L, _priors(L, priors=None), b"priors")
    _err(L, _priors(L, value=None), b"null value")
    _err(L, _priors(L, priors=None, value=None), b"priors")         # the checks of snac_uct_set_priors come first
    _err(L, _priors(L, m=0, value=None), b"null value")             # and every check before the m == 0 return
    assert _priors(L, m=0) == 0                                      # nothing to do: nothing is launched, nothing dereferenced


def test_improved_policy_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    for A in (0, 4, 9):
        _err(L, _policy(L, A=A), b"num_actions")
    _err(L, _policy(L, stats=None), b"null stats")
    _err(L, _policy(L, stats=OFF64), b"128-byte")
    _err(L, _policy(L, B=0), b"B must be")
    _err(L, _policy(L, cap=0), b"cap must be")
    _err(L, _policy(L, rows=4 * 9 - 1), b"exceed stats_rows")        # B * (cap + 1) = 36 rows needed
    _err(L, _policy(L, B=1 << 16, cap=1 << 15, rows=INT_MAX), b"exceed int32")
    _err(L, _policy(L, m=-1), b"m must be")
    _err(L, _policy(L, node_rows=None), b"null rows")
    for x in NOT_FINITE:
        _err(L, _policy(L, c_visit=x), b"c_visit")
        _err(L, _policy(L, c_scale=x), b"c_scale")
    _err(L, _policy(L, bounds=None), b"null bounds")
    _err(L, _policy(L, bounds=OFF8), b"16-byte")
    _err(L, _policy(L, bounds=C.c_void_p((1 << 20) + 4)), b"16-byte")
    _err(L, _policy(L, pi=None), b"null pi")
    _err(L, _policy(L, m=0, pi=None), b"null pi")                    # every check before the m == 0 return
    assert _policy(L, m=0) == 0


# ---- UCTSearch --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(gumbel_interior=True), dict(gumbel_interior=True, evaluator=_fn, q_normalise=True),
                                dict(gumbel=4, evaluator=_fn, q_normalise=True, gumbel_interior=1),
                                dict(gumbel=4, evaluator=_fn, q_normalise=True, gumbel_interior=None),
                                dict(gumbel=4, evaluator=_fn, q_normalise=True, gumbel_interior="yes"),
                                dict(gumbel_interior=0)])
def test_uctsearch_rejects_a_gumbel_interior_it_cannot_run_before_allocating(kw):
    from snac_amd import UCTSearch

    args = dict(nodes_per_tree=16, horizon=0, gamma=0.9)
    args.update(kw)
    with pytest.raises(ValueError, match="gumbel_interior"):
        UCTSearch(_NoDeviceOfFour(), **args)
