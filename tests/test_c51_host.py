"""Host: the rule of include/snac_hip.h, "Distributional targets", restated in numpy (c51_expect_rule, c51_rule), independently of the
kernels (tests/test_gpu_c51.py compares them with it byte for byte): against the textbook floor / ceil projection in float64, its structure
(mass, sign, discount 0, bad samples, the choice of the action), and the inputs the GPU test runs on (make_case: that they contain every
case is asserted here).  Then snac_c51_expect / snac_c51_project are exported and check every argument before any HIP call -- each failing
call below fails its checks first, so the placeholder pointers are never dereferenced -- and the errors of CategoricalSupport, which
checks its tensors before it touches a device."""
import ctypes as C

import numpy as np
import pytest

from cabi_checks import PH, _err_code as _err
from snac_amd import _lib

SUPPORTS = ((51, -10.0, 10.0), (2, -1.0, 1.0), (33, -100.0, 300.0), (63, 0.0, 200.0), (64, -3.0, 7.0))
ACTIONS = (3, 5, 8)


# ---- the rule, in numpy: every ufunc call below is one float64 operation, rounded on its own --------------------------------------------
def support(K, vmin, vmax):
    """(dz, z [K]) in float64."""
    dz = (np.float64(vmax) - np.float64(vmin)) / np.float64(K - 1)
    return dz, np.float64(vmin) + np.arange(K, dtype=np.float64) * dz


def c51_expect_rule(p, vmin, vmax):
    """float64 [...]: the expected value of rows p [..., K] float32 by the header's tree over 64 lanes."""
    p = np.asarray(p, np.float32)
    K = p.shape[-1]
    _, z = support(K, vmin, vmax)
    x = np.zeros(p.shape[:-1] + (64,), np.float64)
    with np.errstate(invalid="ignore"):
        x[..., :K] = p.astype(np.float64) * z
        for s in (32, 16, 8, 4, 2, 1):
            x[..., :s] = x[..., :s] + x[..., s:2 * s]
    return x[..., 0].copy()


def bad_of(ret, discount):
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(ret) | ~np.isfinite(discount) | (discount < 0)


def c51_rule(p_next, ret, discount, vmin, vmax, p_select=None):
    """-> dict(m float32 [B, K], a_star int8 [B], q_star float32 [B], q float32 [B, A] (snac_c51_expect of p_next), bad_rows int)."""
    p_next, ret, discount = np.asarray(p_next, np.float32), np.asarray(ret, np.float32), np.asarray(discount, np.float32)
    B, A, K = p_next.shape
    dz, z = support(K, vmin, vmax)
    q = c51_expect_rule(p_next if p_select is None else p_select, vmin, vmax)
    best, a_star = q[:, 0].copy(), np.zeros(B, np.int64)
    with np.errstate(invalid="ignore"):
        for a in range(1, A):
            wins = q[:, a] > best
            best, a_star = np.where(wins, q[:, a], best), np.where(wins, a, a_star)
    bad = bad_of(ret, discount)
    a_star[bad] = 0
    every = np.arange(B)
    rows = p_next[every, a_star]
    q_star = c51_expect_rule(rows, vmin, vmax).astype(np.float32)
    q_star[bad] = 0.0
    r, d = np.where(bad, 0.0, ret.astype(np.float64)), np.where(bad, 0.0, discount.astype(np.float64))      # (bad rows are zeroed below)
    acc = np.zeros((B, K), np.float64)
    vmin, vmax = np.float64(vmin), np.float64(vmax)
    with np.errstate(invalid="ignore"):
        for i in range(K):
            t = r + d * z[i]
            t = np.where(t < vmin, vmin, t)
            t = np.where(t > vmax, vmax, t)
            pos = (t - vmin) / dz
            l = np.minimum(np.floor(pos).astype(np.int64), K - 1)
            f = pos - l.astype(np.float64)
            p_i = rows[:, i].astype(np.float64)
            top = l == K - 1
            acc[every, l] = acc[every, l] + np.where(top, p_i, p_i * (1.0 - f))
            inner = ~top
            acc[every[inner], l[inner] + 1] = acc[every[inner], l[inner] + 1] + (p_i * f)[inner]
    m = acc.astype(np.float32)
    m[bad] = 0.0
    return dict(m=m, a_star=a_star.astype(np.int8), q_star=q_star, q=c51_expect_rule(p_next, vmin, vmax).astype(np.float32), bad_rows=int(bad.sum()))


def textbook(rows, ret, discount, vmin, vmax):
    """The textbook projection (Bellemare et al. 2017, algorithm 1, with the usual repairs of l == u) in float64 with np.add.at: float64
    [B, K] of the good samples' chosen rows.  b is held at K - 1, which the quotient can pass by a rounding."""
    B, K = rows.shape
    dz, z = support(K, vmin, vmax)
    tz = np.clip(ret.astype(np.float64)[:, None] + discount.astype(np.float64)[:, None] * z[None, :], vmin, vmax)
    b = np.minimum((tz - vmin) / dz, K - 1.0)
    l, u = np.floor(b).astype(np.int64), np.ceil(b).astype(np.int64)
    l[(u > 0) & (l == u)] -= 1
    u[(l < K - 1) & (l == u)] += 1
    m = np.zeros((B, K), np.float64)
    at = np.repeat(np.arange(B), K)
    p = rows.astype(np.float64)
    np.add.at(m, (at, l.reshape(-1)), (p * (u - b)).reshape(-1))
    np.add.at(m, (at, u.reshape(-1)), (p * (b - l)).reshape(-1))
    return m


# ---- the inputs of tests/test_gpu_c51.py: sixteen sorts of sample taking turns, sample i of sort (i + shift) % 16 -------------------------
SORTS = ("plain", "at_vmin", "at_vmax", "below", "above", "discount_0", "discount_1", "discount_3_steps", "discount_above_1", "tie", "nan_select",
         "bad_ret", "bad_discount_inf", "bad_discount_negative", "zero_reward", "plain")
BAD_SORTS = ("bad_ret", "bad_discount_inf", "bad_discount_negative")


def _softmax_rows(rng, shape):
    """float32 distributions with about one exact zero in six (never a whole row)."""
    e = np.exp(2.0 * rng.normal(size=shape))
    zero = rng.random(shape) < 1.0 / 6.0
    zero[..., 0] = False                                             # never a whole row
    e[zero] = 0.0
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def make_case(rng, B, A, K, vmin, vmax, shift=0):
    """dict(p_next, p_select float32 [B, A, K], ret, discount float32 [B], sort: the samples' sorts)."""
    span = vmax - vmin
    p_next, p_select = _softmax_rows(rng, (B, A, K)), _softmax_rows(rng, (B, A, K))
    ret = rng.uniform(vmin + 0.3 * span, vmax - 0.3 * span, size=B).astype(np.float32)
    discount = np.full(B, 0.95, np.float32)
    sorts = [SORTS[(i + shift) % len(SORTS)] for i in range(B)]
    for i, sort in enumerate(sorts):
        if sort == "at_vmin":
            ret[i], discount[i] = vmin, 0.0
        elif sort == "at_vmax":
            ret[i], discount[i] = vmax, 0.0
        elif sort == "below":
            ret[i], discount[i] = vmin - 2.0 * span, 0.5
        elif sort == "above":
            ret[i], discount[i] = vmax + 2.0 * span, 1.0
        elif sort == "discount_0":
            discount[i] = 0.0
        elif sort == "discount_1":
            discount[i] = 1.0
        elif sort == "discount_3_steps":
            discount[i] = 0.95 ** 3
        elif sort == "discount_above_1":
            discount[i] = 1.5
        elif sort == "tie":                                          # two equal rows with the largest value there is: all mass on the top atom
            a1, a2 = sorted(rng.choice(A, size=2, replace=False))
            p_select[i, a1] = p_select[i, a2] = np.eye(K, dtype=np.float32)[K - 1]
        elif sort == "nan_select":                                   # in turn every action, row 0 among them
            p_select[i, (i // len(SORTS)) % A, rng.integers(K)] = np.nan
        elif sort == "bad_ret":
            ret[i] = (np.nan, np.inf, -np.inf)[(i // len(SORTS)) % 3]
        elif sort == "bad_discount_inf":
            discount[i] = (np.inf, np.nan)[(i // len(SORTS)) % 2]
        elif sort == "bad_discount_negative":
            discount[i] = -0.5
        elif sort == "zero_reward":
            ret[i] = 0.0
    return dict(p_next=p_next, p_select=p_select, ret=ret, discount=discount, sort=np.array(sorts))


def bad_rows_of(B, shift=0):
    return sum(SORTS[(i + shift) % len(SORTS)] in BAD_SORTS for i in range(B))


def _cases():
    for n, (K, vmin, vmax) in enumerate(SUPPORTS):
        for A in ACTIONS:
            yield A, K, vmin, vmax, make_case(np.random.default_rng(100 * n + A), 16 * 8 * 3, A, K, vmin, vmax)


def test_the_generated_inputs_contain_every_case():
    for A, K, vmin, vmax, c in _cases():
        p_next, p_select, ret, discount, sort = c["p_next"], c["p_select"], c["ret"], c["discount"], c["sort"]
        B = len(ret)
        assert set(sort) == set(SORTS) and bad_rows_of(B) == B // 16 * 3 and bad_rows_of(1, 11) == 1 and bad_rows_of(1) == 0
        assert (p_next == 0).any() and (p_select[~np.isnan(p_select).any(axis=(1, 2))] == 0).any()
        assert np.allclose(p_next.astype(np.float64).sum(-1), 1.0, atol=1e-5)
        _, z = support(K, vmin, vmax)
        bad = bad_of(ret, discount)
        assert bad.sum() == bad_rows_of(B) and set(sort[bad]) == set(BAD_SORTS)
        assert np.isnan(ret).any() and np.isinf(ret).any() and np.isinf(discount).any() and np.isnan(discount).any() and (discount[~np.isnan(discount)] < 0).any()
        good = ~bad
        lo, hi = ret[good].astype(np.float64) + discount[good] * z[0], ret[good].astype(np.float64) + discount[good] * z[-1]
        assert ((lo == vmin) & (hi == vmin)).any() and ((lo == vmax) & (hi == vmax)).any()      # both ends exactly
        assert (hi < vmin).any() and (lo > vmax).any()                                          # beyond both ends
        for d in (0.0, 1.0, 0.95 ** 3, 1.5):
            assert (discount == np.float32(d)).any(), d
        ties = sort == "tie"
        q = c51_expect_rule(p_select, vmin, vmax)
        assert all((q[i] == q[i].max()).sum() >= 2 for i in np.nonzero(ties)[0])                # the tie is at the top
        nan_rows = np.isnan(p_select).any(axis=2)
        assert nan_rows.any(axis=1).sum() == (sort == "nan_select").sum() and nan_rows[:, 0].any() and nan_rows[:, 1:].any()
        assert not np.isnan(p_next).any()


# ---- against the textbook ----------------------------------------------------------------------------------------------------------------
def test_the_rule_stays_within_2_to_the_minus_24_of_the_textbook_projection():
    """A float32 rounding of a value of at most 1 is at most 2^-25, the float64 accumulations differ by about 1e-15: the factor 2 is the margin."""
    for A, K, vmin, vmax, c in _cases():
        out = c51_rule(c["p_next"], c["ret"], c["discount"], vmin, vmax, c["p_select"])
        good = ~bad_of(c["ret"], c["discount"])
        rows = c["p_next"][np.arange(len(good)), out["a_star"]][good]
        want = textbook(rows, c["ret"][good], c["discount"][good], vmin, vmax)
        m = out["m"][good]
        err = np.abs(m.astype(np.float64) - want).max()
        mass = np.abs(m.astype(np.float64).sum(1) - rows.astype(np.float64).sum(1)).max()
        print("A %d K %d: max |m - textbook| %.3g, mass error %.3g" % (A, K, err, mass))
        assert err <= 2.0 ** -24, (A, K, err)
        assert mass <= K * 2.0 ** -25, (A, K, mass)
        assert (m >= 0).all()


# ---- structure ---------------------------------------------------------------------------------------------------------------------------
def test_discount_0_leaves_at_most_two_adjacent_atoms():
    for A, K, vmin, vmax, c in _cases():
        m = c51_rule(c["p_next"], c["ret"], c["discount"], vmin, vmax, c["p_select"])["m"]
        rows = np.nonzero((c["discount"] == 0) & ~bad_of(c["ret"], c["discount"]))[0]
        assert len(rows) >= 3
        for i in rows:
            at = np.nonzero(m[i])[0]
            assert 1 <= len(at) <= 2 and at[-1] - at[0] <= 1, (i, at)
        ends = {s: np.nonzero(c["sort"] == s)[0] for s in ("at_vmin", "at_vmax")}
        assert (m[ends["at_vmin"], 1:] == 0).all() and (m[ends["at_vmax"], :-1] == 0).all()      # exactly on the end atoms


def test_bad_samples_give_zero_rows_and_the_exact_count():
    for A, K, vmin, vmax, c in _cases():
        out = c51_rule(c["p_next"], c["ret"], c["discount"], vmin, vmax, c["p_select"])
        bad = bad_of(c["ret"], c["discount"])
        assert out["bad_rows"] == bad.sum() == bad_rows_of(len(bad)) > 0
        assert not out["m"][bad].any() and not out["a_star"][bad].any() and not out["q_star"][bad].any()
        assert (out["m"][~bad].sum(1) > 0.99).all() and np.isfinite(out["m"]).all() and np.isfinite(out["q_star"]).all()
        assert out["m"].dtype == np.float32 and out["a_star"].dtype == np.int8 and out["q_star"].dtype == np.float32


def test_the_choice_takes_the_lowest_index_on_ties_and_never_a_nan_row_but_row_0():
    for A, K, vmin, vmax, c in _cases():
        out = c51_rule(c["p_next"], c["ret"], c["discount"], vmin, vmax, c["p_select"])
        a_star, sort = out["a_star"], c["sort"]
        assert a_star.min() >= 0 and a_star.max() < A and len(set(a_star.tolist())) == A
        q = c51_expect_rule(c["p_select"], vmin, vmax)
        for i in np.nonzero(sort == "tie")[0]:
            assert a_star[i] == np.nonzero(q[i] == q[i].max())[0][0] < A - 1
        nan_rows = np.isnan(c["p_select"]).any(axis=2)
        for i in np.nonzero(sort == "nan_select")[0]:
            assert np.isnan(q[i]).sum() == 1
            if nan_rows[i, 0]:
                assert a_star[i] == 0                                # best starts as a NaN: nothing is greater
            else:
                assert not nan_rows[i, a_star[i]] and a_star[i] == np.nanargmax(q[i])
        good = ~bad_of(c["ret"], c["discount"])
        assert np.array_equal(out["q_star"][good], c51_expect_rule(c["p_next"], vmin, vmax)[np.arange(len(good)), a_star].astype(np.float32)[good])
        # without p_select the choice is p_next's own
        own = c51_rule(c["p_next"], c["ret"], c["discount"], vmin, vmax)
        same = c51_rule(c["p_next"], c["ret"], c["discount"], vmin, vmax, c["p_next"])
        for k in ("m", "a_star", "q_star"):
            assert own[k].tobytes() == same[k].tobytes(), k
        assert np.array_equal(own["a_star"][good], np.argmax(c51_expect_rule(c["p_next"], vmin, vmax), axis=1)[good])
        assert (own["q_star"][good] == own["q"].max(axis=1)[good]).all()


def test_the_expected_value_is_the_dot_product_with_the_support():
    for A, K, vmin, vmax, c in _cases():
        _, z = support(K, vmin, vmax)
        q = c51_expect_rule(c["p_next"], vmin, vmax)
        assert np.abs(q - (c["p_next"].astype(np.float64) * z).sum(-1)).max() <= 1e-12 * max(abs(vmin), abs(vmax))
        assert c51_expect_rule(np.eye(K, dtype=np.float32), vmin, vmax).tolist() == z.tolist()


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------
def _expect(L, B=4, A=5, K=51, vmin=-10.0, vmax=10.0, p=PH, q=PH):
    return L.snac_c51_expect(B, A, K, vmin, vmax, p, q, None)


def _project(L, B=4, A=5, K=51, vmin=-10.0, vmax=10.0, p_next=PH, p_select=None, ret=PH, discount=PH, m=PH, a_star=PH, q_star=PH, bad=PH):
    return L.snac_c51_project(B, A, K, vmin, vmax, p_next, p_select, ret, discount, m, a_star, q_star, bad, None)


def test_the_library_exports_the_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    for name, n in (("snac_c51_expect", 8), ("snac_c51_project", 14)):
        assert name in _lib.EXPORTS and len(getattr(L, name).argtypes) == n
        assert _lib.PROTOTYPES[name][1][:5] == [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double]
        assert all(t == C.c_void_p for t in _lib.PROTOTYPES[name][1][5:])


def test_both_entry_points_validate_their_arguments_before_any_hip_call():
    L = _lib.lib()
    _err(L, _expect(L, p=None), -1, b"null p/q")
    _err(L, _expect(L, q=None), -1, b"null p/q")
    for name in ("p_next", "ret", "discount", "m"):
        _err(L, _project(L, **{name: None}), -1, b"null p_next/ret/discount/m")
    for call in (_expect, _project):
        for B in (0, -1, -(1 << 31)):
            _err(L, call(L, B=B), -1, b"B must be >= 1")
        for K in (1, 0, -1, 65, 1 << 20):
            _err(L, call(L, K=K), -1, b"atoms must be in [2, 64]")
        for vmin, vmax in ((float("nan"), 1.0), (0.0, float("nan")), (float("-inf"), 0.0), (0.0, float("inf")), (1.0, 1.0), (2.0, 1.0)):
            _err(L, call(L, vmin=vmin, vmax=vmax), -1, b"vmin and vmax must be finite, with vmin < vmax")
        for A in (0, 1, 2, 4, 6, 7, 9, -3):
            _err(L, call(L, A=A), -3, b"num_actions must be 3, 5 or 8")
    # the optional arguments do not change the checks
    _err(L, _project(L, B=0, p_select=PH, a_star=None, q_star=None, bad=None), -1, b"B must be >= 1")
    _err(L, _project(L, K=65, a_star=None), -1, b"atoms must be in")


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------------
def test_categorical_support_checks_its_arguments_before_it_touches_a_device():
    import torch
    from snac_amd import CategoricalSupport

    for bad in (dict(num_actions=4), dict(num_actions=True), dict(num_actions="5"), dict(atoms=1), dict(atoms=65), dict(atoms=51.0),
                dict(vmin=float("nan")), dict(vmax=float("inf")), dict(vmin=1.0, vmax=1.0), dict(vmin=2.0, vmax=-2.0), dict(device="cpu"),
                dict(device=None)):
        with pytest.raises(ValueError):
            CategoricalSupport(**dict(dict(num_actions=5, device="cuda:0"), **bad))
    cs = CategoricalSupport(5, atoms=51, vmin=-10.0, vmax=10.0, device="cuda:0")
    assert (cs.num_actions, cs.atoms, cs.vmin, cs.vmax) == (5, 51, -10.0, 10.0) and cs.dz == support(51, -10.0, 10.0)[0]
    p, v = torch.zeros(4, 5, 51), torch.zeros(4)
    with pytest.raises(ValueError, match=r"p must have shape \(B, 5, 51\), got \(4, 5, 50\)"):
        cs.expected(torch.zeros(4, 5, 50))
    with pytest.raises(ValueError, match="p must have shape"):
        cs.expected(torch.zeros(4, 255))
    with pytest.raises(ValueError, match="p must have shape"):
        cs.expected(torch.zeros(0, 5, 51))
    with pytest.raises(ValueError, match="p must be a contiguous torch.float32 tensor"):
        cs.expected(p.double())
    with pytest.raises(ValueError, match="p must be a contiguous torch.float32 tensor"):
        cs.expected(torch.zeros(4, 5, 102)[:, :, ::2])
    with pytest.raises(ValueError, match="p must be a contiguous torch.float32 tensor"):
        cs.expected(p.numpy())
    with pytest.raises(ValueError, match="p must be on cuda:0"):
        cs.expected(p)
    with pytest.raises(ValueError, match="p_next must have shape"):
        cs.project(torch.zeros(4, 3, 51), v, v)
    with pytest.raises(ValueError, match="p_next must be on cuda:0"):
        cs.project(p, v, v)
