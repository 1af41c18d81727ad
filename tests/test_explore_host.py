"""Host: the rules of include/snac_hip.h, "Exploration noise", restated in numpy independently of the kernels (tests/test_gpu_explore.py
compares the kernels with them byte for byte): LOGP against np.log, the log of a Gamma draw, the Dirichlet root noise, the Gumbel
scores and the move by a temperature.  The restatement equals snac_amd/csrc/explore_rule.h compiled for the host byte for byte
(tests/native/explore_host.cpp), which also runs as a stand-alone program under the host sanitizers; the Dirichlet components pass a
two-sample Kolmogorov-Smirnov test against numpy's sampler, the temperature draws match their weights and the weights N ** (1 / T), the
Gumbel noise has the Gumbel's mean and variance.  Last, the three entry points check every argument before any HIP call -- each failing
call fails its checks first, so the placeholder pointers are never dereferenced -- and the wrappers reject bad arguments before they
touch a device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from cabi_checks import ODD, PH, _desc, _err
import helpers
from hostcode import load_shared, run_sanitized
import rng_spec
from snac_amd import _lib
from specmath import spec_exp, spec_log
from test_uct_selfplay_host import hostless_search, tree_checks

ACTIONS = (3, 5, 8)
ALPHAS = (0.03, 0.3, 1.0, 2.5)
M32 = 0xFFFFFFFF
STREAM_PICK, STREAM_DIRICHLET, STREAM_GUMBEL = 3, 6, 7
TWO28 = 268435456.0


# ---- the rules, in numpy: every ufunc call below is one float64 operation, rounded on its own -------------------------------------------
def unit_of(w):
    return (np.asarray(w).astype(np.float64) + 0.5) * 2.0 ** -32


def env_ids_of(base, B):
    """env_id_base + b as the unsigned 64-bit integers the keys are built from."""
    return np.array([(int(base) + b) & 0xFFFFFFFFFFFFFFFF for b in range(B)], np.uint64)


def slot_keys(env_ids, A):
    """(env_id_base + b) * 8 + a, [B, A], in unsigned 64-bit wrap-around: the factor is 8 for every A."""
    return np.asarray(env_ids, np.uint64)[:, None] * np.uint64(8) + np.arange(A, dtype=np.uint64)[None, :]


def gamma_params(alpha):
    alpha = np.float64(alpha)
    boost = bool(alpha < 1.0)
    a1 = alpha + 1.0 if boost else alpha
    d = a1 - np.float64(1.0) / np.float64(3.0)
    c = 1.0 / np.sqrt(9.0 * d)
    return boost, d, c, spec_log(d)


def gamma_log(seed, keys, t, alpha, attempts):
    """-> (lg float64, accepted bool), shaped as keys: the log of a Gamma(alpha, 1) draw per key at move t."""
    boost, d, c, logd = gamma_params(alpha)
    flat = np.asarray(keys, np.uint64).reshape(-1)
    t = int(t) & M32
    lv, got = np.zeros(flat.size), np.zeros(flat.size, bool)
    idx = np.arange(flat.size)                                       # the draws still without an accepted attempt
    for j in range(attempts):
        if idx.size == 0:
            break
        u1, u2, u3 = (unit_of(rng_spec.words(seed, STREAM_DIRICHLET, flat[idx], np.uint64((t * 128 + 4 * j + k) & M32))) for k in range(3))
        x = (1.7156 * (u2 - 0.5)) / u1
        x2 = x * x
        normal = x2 <= -4.0 * spec_log(u1)
        s = 1.0 + c * x
        v = (s * s) * s
        positive = v > 0.0
        lt = spec_log(np.where(positive, v, 1.0))
        rhs = ((0.5 * x2 + d) - d * v) + d * lt
        acc = normal & positive & (spec_log(u3) < rhs)
        lv[idx[acc]], got[idx[acc]] = lt[acc], True
        idx = idx[~acc]
    lg = np.where(got, logd + lv, logd)
    if boost:
        lg = lg + spec_log(unit_of(rng_spec.words(seed, STREAM_DIRICHLET, flat, np.uint64((t * 128 + 3) & M32)))) / np.float64(alpha)
    return lg.reshape(np.shape(keys)), got.reshape(np.shape(keys))


def priors_bad(p):
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(p).all(axis=1) | (p < 0).any(axis=1) | ~(p > 0).any(axis=1)


def dirichlet_rule(seed, env_ids, t, priors, alpha, eps, attempts=16, mask=None):
    """-> dict(priors float32 [B, A]: the rows after the call; bad_rows int; eta float64 [B, A] (rows that drew); accepted bool [B, A])."""
    p = np.asarray(priors, np.float32)
    B, A = p.shape
    bad = priors_bad(p)
    on = np.ones(B, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    support = p > 0
    lg, got = gamma_log(seed, slot_keys(env_ids, A), t, alpha, attempts)
    l = np.where(support, lg.astype(np.float32), np.float32(-np.inf)).astype(np.float32)
    m = l[:, 0].copy()
    for a in range(1, A):
        m = np.where(l[:, a] > m, l[:, a], m)
    row = on & ~bad
    with np.errstate(invalid="ignore"):
        x = l.astype(np.float64) - m.astype(np.float64)[:, None]
    x[~row] = 0.0
    e = spec_exp(x)
    S = np.zeros(B)
    for a in range(A):
        S = S + e[:, a]
    eta = e / S[:, None]
    om = np.float64(1.0) - np.float64(eps)
    with np.errstate(invalid="ignore"):                              # a bad row's NaN or infinity: the row is not written
        new = (om * p.astype(np.float64) + np.float64(eps) * eta).astype(np.float32)
    write = row[:, None] & support
    out = p.copy()
    out[write] = new[write]
    return dict(priors=out, bad_rows=int((on & bad).sum()), eta=eta, accepted=got | ~support, drew=write)


def gumbel_noise(seed, keys, t):
    w = rng_spec.words(seed, STREAM_GUMBEL, np.asarray(keys, np.uint64), np.uint64(int(t) & M32))
    return -spec_log(-spec_log(unit_of(w)))


def gumbel_rule(seed, env_ids, t, priors, noisy=None):
    """-> scores float32 [B, A]."""
    p = np.asarray(priors, np.float32)
    B, A = p.shape
    on = np.ones(B, bool) if noisy is None else np.asarray(noisy).reshape(-1) != 0
    n = np.where(on[:, None], gumbel_noise(seed, slot_keys(env_ids, A), t), 0.0)
    with np.errstate(invalid="ignore"):
        good = (p > 0) & np.isfinite(p)
        val = (spec_log(np.where(good, p.astype(np.float64), 1.0)) + n).astype(np.float32)
        return np.where(good, val, np.where(p == 0, np.float32(-np.inf), np.float32(np.nan))).astype(np.float32)


def temp_weights(counts, T):
    """-> (w uint64 [B, A], total uint64 [B]) of a T that is neither 0 nor 1 (T float64 [B]); rows where T <= 0 or a NaN hold garbage."""
    n = np.maximum(np.asarray(counts, np.int64), 0)
    nmax = n.max(axis=1)
    lmax = spec_log(np.maximum(nmax, 1).astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = 1.0 / np.asarray(T, np.float64)
        x = (spec_log(np.maximum(n, 1).astype(np.float64)) - lmax[:, None]) * r[:, None]
    top = n == nmax[:, None]
    x[top | ~(np.asarray(T, np.float64) > 0)[:, None] | (n == 0)] = 0.0
    w = np.floor(spec_exp(x) * TWO28).astype(np.uint64)
    w = np.where(n == 0, 0, np.where(top, 1 << 28, w)).astype(np.uint64)
    return w, w.sum(axis=1)


def _draw(w, total, word):
    """u = (word * total) >> 32 without leaving 64 bits; the lowest a whose running sum passes u."""
    word, total = np.asarray(word, np.uint64), np.asarray(total, np.uint64)
    u = word * (total >> np.uint64(32)) + ((word * (total & np.uint64(M32))) >> np.uint64(32))
    return (np.cumsum(np.asarray(w, np.uint64), axis=1) > u[:, None]).argmax(axis=1)


def temp_rule(seed, env_ids, t, counts, greedy=None, T=1.0):
    """-> action int8 [B].  greedy: None (every tree) or [B] (non-zero: greedy); T: a number or float32 [B]."""
    n = np.maximum(np.asarray(counts, np.int64), 0).astype(np.uint64)
    B, A = n.shape
    total = n.sum(axis=1)
    word = rng_spec.words(seed, STREAM_PICK, np.asarray(env_ids, np.uint64), np.uint64(int(t) & M32))
    g = np.ones(B, bool) if greedy is None else np.asarray(greedy).reshape(-1) != 0
    T = np.broadcast_to(np.asarray(T, np.float32 if np.ndim(T) else np.float64).astype(np.float64), (B,))
    best = n.argmax(axis=1)                                          # the lowest a with the largest count
    w, wtotal = temp_weights(n, T)
    with np.errstate(invalid="ignore"):
        act = np.where(g | ~(T > 0), best, np.where(T == 1.0, _draw(n, total, word), _draw(w, wtotal, word)))
    return np.where(total == 0, 0, act).astype(np.int8)


# ---- the inputs the host and the GPU tests share ----------------------------------------------------------------------------------------
SORTS = ("normal", "normal", "one_zero", "nan", "plus_inf", "negative", "all_zero", "neg_zero", "peaked", "several_zero", "normal")
BAD = ("nan", "plus_inf", "negative", "all_zero")


def make_priors(rng, B, A, shift=0):
    """float32 [B, A] rows of root priors, row b of sort SORTS[(b + shift) % len(SORTS)]: softmax-like rows, rows with zeros (off the
    support), -0.0, and a bad row of each sort."""
    p = rng.dirichlet(np.ones(A), B).astype(np.float32)
    for b in range(B):
        sort = SORTS[(b + shift) % len(SORTS)]
        a = int(rng.integers(A))
        if sort == "one_zero":
            p[b, a] = 0.0
        elif sort == "nan":
            p[b, a] = np.nan
        elif sort == "plus_inf":
            p[b, a] = np.inf
        elif sort == "negative":
            p[b, a] = -0.125
        elif sort == "all_zero":
            p[b] = 0.0
        elif sort == "neg_zero":
            p[b, a] = -0.0
        elif sort == "peaked":
            p[b] = 1e-30
            p[b, a] = 1.0
        elif sort == "several_zero":
            p[b] = 0.0
            p[b, a] = 0.75
            p[b, (a + 1) % A] = 0.25
    return p


def bad_rows_of(B, shift=0, mask=None):
    return sum(SORTS[(b + shift) % len(SORTS)] in BAD and (mask is None or mask[b] != 0) for b in range(B))


def make_counts(rng, B, A):
    """int32 [B, A] child visits: zeros, equal counts, a count of 2^31 - 1, an empty row, a negative word (reads as zero)."""
    n = rng.integers(0, 60, (B, A)).astype(np.int32)
    for b in range(B):
        k = b % 7
        if k == 1:
            n[b] = 0
        elif k == 2:
            n[b] = 17
        elif k == 3:
            n[b, int(rng.integers(A))] = 0x7FFFFFFF
        elif k == 4:
            n[b, int(rng.integers(A))] = -5
        elif k == 5:
            n[b, int(rng.integers(A))] = 0
    return n


TEMPS = (0.0, 1.0, 0.5, 2.0, 0.25, float("inf"), float("nan"), -1.0, 1e-30, 4.0, 1.0 + 2.0 ** -20)


def make_temps(B):
    return np.array([TEMPS[b % len(TEMPS)] for b in range(B)], np.float32)


def _same(got, want, what):
    """Byte for byte, but a NaN of the rule is any NaN."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind != "f":
        assert np.array_equal(got, want), (what, np.nonzero(np.asarray(got != want).reshape(len(got), -1).any(axis=1))[0][:8])
        return
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaNs")
    g, w = np.where(nan, 0, got).astype(got.dtype).view(np.uint32), np.where(nan, 0, want).astype(got.dtype).view(np.uint32)
    diff = np.nonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(axis=1))[0]
    assert diff.size == 0, (what, "first row that differs", int(diff[0]), got[diff[0]], want[diff[0]])


def test_the_generated_inputs_contain_every_sort():
    rng = np.random.default_rng(3)
    for A in ACTIONS:
        p = make_priors(rng, 64, A)
        bad = priors_bad(p)
        assert bad.sum() == bad_rows_of(64) > 0 and (~bad).sum() > 32
        assert ((p == 0) & ~bad[:, None]).any() and np.signbit(p[p == 0]).any() and np.isnan(p).any() and np.isinf(p).any() and (p < 0).any()
        n = make_counts(rng, 64, A)
        assert (n.max(axis=1) == 0x7FFFFFFF).any() and (n < 0).any() and (np.maximum(n, 0).sum(axis=1) == 0).any()
        assert (n == 17).all(axis=1).any()
    t = make_temps(64)
    assert set(np.unique(t[np.isfinite(t)])) >= {0.0, 1.0, 0.5, 2.0} and np.isnan(t).any() and np.isinf(t).any() and (t < 0).any()


# ---- LOGP -------------------------------------------------------------------------------------------------------------------------------
def test_logp_stays_within_the_derived_bound_of_the_logarithm_from_2_to_the_minus_33_to_2_to_the_31():
    """s = f * 2^e with f in [sqrt 1/2, sqrt 2): |z| = |f - 1| / (f + 1) < 0.1716, and the series 2 z sum_{n<11} z^2n / (2n + 1) leaves out
    2 z^23 / 23 / (1 - z^2) < 2.3e-19.  The roundings: z carries two (f - 1 is exact), the Horner steps of q and the product 2 z q a
    few units of 2^-53 on a value of at most 0.3466, and e * LN2_HI is exact, so the two last sums round values of at most |log s| +
    0.3466.  Sixteen units of 2^-53 on that magnitude cover all of them; np.log itself is within one more."""
    rng = np.random.default_rng(11)
    s = np.exp2(rng.uniform(-33.0, 31.0, 400000))
    edges = [2.0 ** -33, 2.0 ** 31, float(2 ** 31 - 1), 1.0, np.nextafter(1.0, 0), np.nextafter(1.0, 2), float.fromhex("0x1.6a09e667f3bcdp-1"),
             np.nextafter(float.fromhex("0x1.6a09e667f3bcdp-1"), 0), 0.5, 2.0, unit_of(0), unit_of(M32), 2.0 / 3.0, 1024.0 - 1.0 / 3.0]
    s = np.concatenate([s, np.array(edges), np.arange(1, 4097, dtype=np.float64), unit_of(rng.integers(0, 1 << 32, 100000))])
    got, want = spec_log(s), np.log(s)
    bound = 2.3e-19 + 17 * 2.0 ** -53 * (np.abs(want) + 0.3466)
    err = np.abs(got - want)
    print("LOGP: largest error / bound %.3f" % float((err / bound).max()))
    assert (err <= bound).all(), (s[np.argmax(err / bound)], float((err / bound).max()))
    assert spec_log(np.float64(1.0)) == 0.0
    # the existing domain keeps its bytes: the sequence is LOG's, and the C code of the library agrees below, byte for byte


# ---- the Gamma draw and the Dirichlet noise ---------------------------------------------------------------------------------------------
def test_one_attempt_fails_in_about_three_draws_of_ten_and_sixteen_attempts_do_not():
    keys = np.arange(100000, dtype=np.uint64) + np.uint64(12345)
    for alpha in ALPHAS:
        _, got1 = gamma_log(5, keys, 9, alpha, 1)
        _, got2 = gamma_log(5, keys, 9, alpha, 2)
        lg16, got16 = gamma_log(5, keys, 9, alpha, 16)
        rate = float(got1.mean())
        print("alpha %g: one attempt accepted %.4f, two %.4f" % (alpha, rate, float(got2.mean())))
        assert 0.66 < rate < 0.76 and got1.sum() < got2.sum() < keys.size and got16.all()
        assert np.isfinite(lg16).all()
        # the first accepted attempt is the same whatever the bound: a draw that one attempt gives, sixteen give too
        lg1, _ = gamma_log(5, keys, 9, alpha, 1)
        assert np.array_equal(lg1[got1], lg16[got1])


def _ks(x, y):
    """The two-sample Kolmogorov-Smirnov distance."""
    x, y = np.sort(x), np.sort(y)
    both = np.concatenate([x, y])
    return float(np.abs(np.searchsorted(x, both, "right") / x.size - np.searchsorted(y, both, "right") / y.size).max())


@pytest.mark.parametrize("A", ACTIONS)
def test_the_dirichlet_components_pass_a_two_sample_ks_test_against_numpys_sampler(A):
    n = 100000
    threshold = math.sqrt(-math.log(0.5e-9) / 2.0) * math.sqrt(2.0 / n)        # significance 1e-9: a condition, not a fit
    assert abs(threshold - 0.0146) < 1e-4
    worst = 0.0
    for alpha in ALPHAS:
        p = np.full((n, A), 1.0 / A, np.float32)
        eta = dirichlet_rule(20261021, env_ids_of(1 << 33, n), 7, p, alpha, 1.0)["eta"]
        ref = np.random.default_rng(1000 + A).dirichlet(np.full(A, alpha), n)
        assert np.abs(eta.sum(axis=1) - 1.0).max() < 1e-12
        for a in range(A):
            d = _ks(np.maximum(eta[:, a], 1e-15), np.maximum(ref[:, a], 1e-15))
            worst = max(worst, d)
            assert d < threshold, (A, alpha, a, d)
    print("A %d: largest KS distance %.4f (threshold %.4f)" % (A, worst, threshold))


def test_the_dirichlet_rule_leaves_bad_rows_masked_rows_and_priors_off_the_support_alone():
    rng = np.random.default_rng(8)
    for A in ACTIONS:
        B = 66
        p = make_priors(rng, B, A, 2)
        mask = (np.arange(B) % 3 != 1).astype(np.uint8)
        for eps in (0.0, 0.25, 1.0):
            o = dirichlet_rule(3, env_ids_of(50, B), 4, p, 0.3, eps, 16, mask)
            assert o["bad_rows"] == bad_rows_of(B, 2, mask) > 0
            keep = ~o["drew"]
            assert np.array_equal(o["priors"].view(np.uint32)[keep], p.view(np.uint32)[keep])
            rows = o["drew"].any(axis=1)
            assert rows.sum() > B // 3 and not rows[mask == 0].any() and not rows[priors_bad(p)].any()
            if eps == 0.0:
                assert np.array_equal(o["priors"].view(np.uint32), p.view(np.uint32))
            if eps == 1.0:
                assert np.abs(o["priors"][rows].sum(axis=1) - 1.0).max() < 1e-6
        # env ids alone key the draws: a shard equals the whole
        whole = dirichlet_rule(3, env_ids_of(50, B), 4, p, 0.3, 0.25)["priors"]
        part = dirichlet_rule(3, env_ids_of(50 + 20, B - 20), 4, p[20:], 0.3, 0.25)["priors"]
        assert np.array_equal(whole[20:].view(np.uint32), part.view(np.uint32))


# ---- the Gumbel scores ------------------------------------------------------------------------------------------------------------------
def test_the_gumbel_noise_has_the_gumbels_mean_and_variance():
    n = 400000
    g = gumbel_noise(99, np.arange(n, dtype=np.uint64) * np.uint64(8) + np.uint64(3), 17)
    var = math.pi ** 2 / 6.0
    se_mean, se_var = math.sqrt(var / n), var * math.sqrt(4.4 / n)   # the Gumbel's excess kurtosis is 2.4: var(s^2) = (5.4 - 1) var^2 / n
    print("Gumbel noise: mean %.5f (%.5f), variance %.5f (%.5f)" % (g.mean(), np.euler_gamma, g.var(), var))
    assert abs(g.mean() - np.euler_gamma) < 6 * se_mean and abs(g.var() - var) < 6 * se_var
    p = np.array([[0.5, 0.0, -0.0, np.nan, -1.0, np.inf, 1e-40, 1.0]], np.float32)
    s = gumbel_rule(1, env_ids_of(0, 1), 0, p, noisy=[0])
    assert s[0, 0] == np.float32(np.log(0.5)) and s[0, 1] == s[0, 2] == -np.inf and np.isnan(s[0, 3:6]).all() and s[0, 7] == 0.0
    assert abs(float(s[0, 6]) - math.log(1e-40)) < 1e-4              # a float32 subnormal is a float64 normal


# ---- the move by a temperature ----------------------------------------------------------------------------------------------------------
ROOTS = {3: [0, 5, 5], 5: [7, 0, 7, 0x7FFFFFFF, 1], 8: [3, 0, 12, 12, 1, 40, 0, 9]}


@pytest.mark.parametrize("A", ACTIONS)
def test_the_temperature_draws_match_their_weights_and_the_weights_the_powers_of_the_counts(A):
    """w_a / 2^28 is within D = 2^-28 + 1e-11 of q_a = (N_a / N_max) ** (1 / T): the floor loses less than 2^-28, and EXP and LOGP stay
    within 1e-12 and 2e-14 of the exact functions, times r <= 4 and a q_a <= 1.  With the largest weight exactly 1 both sums are at
    least 1, so |w_a / sum w - q_a / sum q| <= D / sum w + q_a |sum q - sum w| / (sum w sum q) <= (A + 1) D."""
    draws = 200000
    counts = np.tile(np.array(ROOTS[A], np.int32), (draws, 1))
    n = np.array(ROOTS[A], np.float64)
    env = np.full(draws, 77, np.uint64)
    ts = np.arange(draws)
    word = rng_spec.words(1, STREAM_PICK, env, ts.astype(np.uint64))
    for T in (0.25, 0.5, 2.0, 4.0, float("inf")):
        w, total = temp_weights(counts[:1], np.array([T]))
        assert 1 << 28 <= int(total[0]) <= 1 << 31 and int(w[0].max()) == 1 << 28 and not w[0][n == 0].any()
        q = np.where(n > 0, (n / n.max()) ** (1.0 / T), 0.0)
        prob = w[0] / float(total[0])
        assert np.abs(prob - q / q.sum()).max() <= (A + 1) * (2.0 ** -28 + 1e-11), (T, prob, q / q.sum())
        act = _draw(np.tile(w, (draws, 1)), np.tile(total, draws), word)
        freq = np.bincount(act, minlength=A) / draws
        se = np.sqrt(prob * (1 - prob) / draws)
        print("A %d T %g: largest deviation %.2f standard errors" % (A, T, float((np.abs(freq - prob) / np.maximum(se, 1e-300))[prob > 0].max())))
        assert (np.abs(freq - prob) <= 6 * se).all(), (T, freq, prob)
        got = temp_rule(1, env, 0, counts[:1], greedy=[0], T=T)       # the rule's own path draws by these weights
        assert got[0] == _draw(w, total, word[:1])[0]
    if A == 5:                                                       # T = inf is uniform over the visited actions
        w, _ = temp_weights(counts[:1], np.array([np.inf]))
        assert list(w[0]) == [1 << 28, 0, 1 << 28, 1 << 28, 1 << 28]


def test_temperature_one_is_the_integer_rule_and_zero_is_greedy():
    rng = np.random.default_rng(21)
    for A in ACTIONS:
        B = 700
        n = make_counts(rng, B, A)
        env = env_ids_of(-3, B)
        none = np.zeros(B, np.uint8)
        nn = np.maximum(n, 0).astype(np.uint64)
        word = rng_spec.words(4, STREAM_PICK, env, np.uint64(6))
        u = (word * nn.sum(axis=1)) >> np.uint64(32)                 # these totals stay below 2^32: the header's own statement
        small = nn.sum(axis=1) < (1 << 31)
        integer = np.where(nn.sum(axis=1) == 0, 0, (np.cumsum(nn, axis=1) > u[:, None]).argmax(axis=1)).astype(np.int8)
        one = temp_rule(4, env, 6, n, none, 1.0)
        assert np.array_equal(one[small], integer[small]) and small.sum() > B // 2
        greedy = np.where(nn.sum(axis=1) == 0, 0, nn.argmax(axis=1)).astype(np.int8)
        for T in (0.0, -1.0, float("nan")):
            assert np.array_equal(temp_rule(4, env, 6, n, none, np.full(B, T, np.float32)), greedy)
        assert np.array_equal(temp_rule(4, env, 6, n, None, 0.5), greedy)        # greedy by the mask, whatever T
        assert np.array_equal(temp_rule(4, env, 6, n, np.ones(B, np.uint8), make_temps(B)), greedy)
        mixed = temp_rule(4, env, 6, n, none, make_temps(B))
        assert (mixed != greedy).any() and (mixed != one).any()
        assert (nn[np.arange(B), mixed] > 0)[nn.sum(axis=1) > 0].all()             # an unvisited action is never drawn


# ---- the C entry points -----------------------------------------------------------------------------------------------------------------
def _dir(L, desc=True, A=5, stats=PH, rows=100, B=4, cap=8, mask=PH, t=3, alpha=0.3, eps=0.25, attempts=16, bad=PH):
    d = _desc(2)
    return L.snac_explore_root_dirichlet(C.byref(d) if desc else None, A, stats, rows, B, cap, mask, t, alpha, eps, attempts, bad, None)


def _gum(L, desc=True, A=5, stats=PH, rows=100, B=4, cap=8, noisy=PH, t=3, scores=PH):
    d = _desc(2)
    return L.snac_explore_gumbel_scores(C.byref(d) if desc else None, A, stats, rows, B, cap, noisy, t, scores, None)


def _tmp(L, desc=True, A=5, stats=PH, rows=100, B=4, cap=8, greedy=PH, t=3, temperature=PH, temp=1.0, action=PH, pi=PH, value=PH):
    d = _desc(2)
    return L.snac_explore_pick_moves_temp(C.byref(d) if desc else None, A, stats, rows, B, cap, greedy, t, temperature, temp, action, pi, value, None)


def test_the_library_exports_the_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    for n, k in (("snac_explore_root_dirichlet", 13), ("snac_explore_gumbel_scores", 10), ("snac_explore_pick_moves_temp", 14)):
        assert n in _lib.EXPORTS and len(getattr(L, n).argtypes) == k
    args = _lib.PROTOTYPES["snac_explore_root_dirichlet"][1]
    assert args[8:11] == [C.c_double, C.c_double, C.c_int32] and args[7] == C.c_uint32
    assert _lib.PROTOTYPES["snac_explore_pick_moves_temp"][1][9] == C.c_double


def test_the_exploration_entry_points_validate_their_arguments_before_any_hip_call():
    L = _lib.lib()
    none = dict(action=None, pi=None, value=None)
    for call in (_dir, _gum, _tmp):
        tree_checks(L, call)
        _err(L, call(L, desc=False), b"null desc")
    for x in (0.0, 2.0 ** -11, np.nextafter(2.0 ** -10, 0), np.nextafter(1024.0, 2048.0), 2048.0, -0.3, float("nan"), float("inf")):
        _err(L, _dir(L, alpha=float(x)), b"alpha must be in")
    for x in (-1e-9, np.nextafter(1.0, 2.0), float("nan"), float("inf"), -1.0):
        _err(L, _dir(L, eps=float(x)), b"eps must be in")
    for x in (0, -1, 33, 1 << 20):
        _err(L, _dir(L, attempts=x), b"attempts must be in")
    _err(L, _gum(L, scores=None), b"null scores")
    for x in (-1e-300, -1.0, float("nan"), float("-inf")):
        _err(L, _tmp(L, temp=x), b"temp must be")
    # nothing to write: no launch, although no device exists to launch on -- but the checks come first
    assert _dir(L, eps=0.0, bad=None) == 0 and _dir(L, eps=0.0, bad=None, mask=None, alpha=2.0 ** -10, attempts=32) == 0
    _err(L, _dir(L, eps=0.0, bad=None, alpha=0.0), b"alpha must be in")
    _err(L, _dir(L, eps=0.0, bad=None, rows=35), b"exceed stats_rows")
    for temp in (0.0, 1.0, 0.5, float("inf")):
        assert _tmp(L, temp=temp, **none) == 0 and _tmp(L, temp=temp, temperature=None, greedy=None, rows=36, **none) == 0
    _err(L, _tmp(L, temp=-1.0, **none), b"temp must be")
    _err(L, _tmp(L, stats=ODD, **none), b"128-byte")


def test_the_wrappers_reject_bad_arguments_before_touching_a_device():
    import torch
    from snac_amd import SelfPlay

    s = hostless_search()
    for T in (-0.5, float("nan"), "1", True, torch.ones(3), torch.ones(4, dtype=torch.float64), torch.ones(4, 1), [1.0] * 4):
        with pytest.raises(ValueError, match="temperature"):
            s.pick_moves(greedy=False, temperature=T)
    with pytest.raises(ValueError, match="PUCT"):
        s.add_dirichlet_noise(0.3)
    s.evaluator = lambda obs: None
    for kw in (dict(alpha=0.0), dict(alpha=2000.0), dict(alpha=float("nan")), dict(alpha="0.3"), dict(alpha=True), dict(alpha=0.3, eps=-0.1),
               dict(alpha=0.3, eps=1.5), dict(alpha=0.3, eps=None), dict(alpha=0.3, attempts=0), dict(alpha=0.3, attempts=33),
               dict(alpha=0.3, attempts=2.0), dict(alpha=0.3, t=1.5), dict(alpha=0.3, mask=torch.ones(3)), dict(alpha=0.3, mask=[1, 1, 1, 1])):
        with pytest.raises(ValueError):
            s.add_dirichlet_noise(**kw)
    s.gumbel = None
    with pytest.raises(ValueError, match="not a Gumbel search"):
        s.gumbel_scores(t=0)
    s.gumbel = 4
    for kw in (dict(t=0, generator=object()), dict(t=1.5), dict(t=True), dict(t=0, noise=torch.ones(3)), dict(t=0, noise="yes")):
        with pytest.raises(ValueError):
            s.gumbel_scores(**kw)
    fn = lambda p: p  # noqa: E731
    for kw in (dict(dirichlet=(0.3, 0.25), root_noise=fn), dict(dirichlet=(0.3, 0.25), gumbel=True), dict(dirichlet=0.3), dict(dirichlet=(0.3,)),
               dict(dirichlet=(0.0, 0.25)), dict(dirichlet=(0.3, 1.5)), dict(dirichlet=("a", 0.25)), dict(dirichlet=(True, 0.25)),
               dict(temperature=1.0, gumbel=True), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature="1"),
               dict(temperature=True), dict(counter_noise=True), dict(counter_noise=1), dict(counter_noise=True, gumbel=True, generator=object())):
        with pytest.raises(ValueError):
            SelfPlay(s, 8, **kw)
    s.evaluator = None
    with pytest.raises(ValueError, match="PUCT"):
        SelfPlay(s, 8, dirichlet=(0.3, 0.25))


# ---- the kernels' code on the host ------------------------------------------------------------------------------------------------------
HOST_SRC = os.path.join(helpers.TESTS, "native", "explore_host.cpp")
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", _lib.CSRC, HOST_SRC]


def test_the_kernels_code_compiled_for_the_host_equals_the_rules_byte_for_byte(tmp_path):
    H = load_shared(tmp_path, "explore_host", ["-O2", "-fPIC", "-shared"] + HOST_FLAGS, timeout=600)
    head = [C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_uint32]
    H.explore_dirichlet_host.restype, H.explore_dirichlet_host.argtypes = C.c_int, head + [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int32,
                                                                                          C.c_void_p]
    H.explore_gumbel_host.restype, H.explore_gumbel_host.argtypes = C.c_int, head + [C.c_void_p] * 3
    H.explore_temp_host.restype, H.explore_temp_host.argtypes = C.c_int, head + [C.c_void_p] * 3 + [C.c_double, C.c_void_p]
    H.explore_logp_host.restype, H.explore_logp_host.argtypes = None, [C.c_int64, C.c_void_p, C.c_void_p]
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

    s = np.concatenate([np.exp2(np.random.default_rng(2).uniform(-33, 31, 20000)), np.linspace(1.0, 64.0, 5000)])
    out = np.zeros_like(s)
    H.explore_logp_host(s.size, vp(s), vp(out))
    assert np.array_equal(out.view(np.uint64), spec_log(s).view(np.uint64))

    seed, base = 0x123456789ABCDEF, (1 << 40) + 5
    rng = np.random.default_rng(77)
    fails = {1: 0, 16: 0}
    for A in ACTIONS:
        for B, t in ((1, 0), (9, 1), (257, (1 << 25) + 3)):
            env = env_ids_of(base, B)
            for shift in (range(len(SORTS)) if B == 1 else (B % len(SORTS),)):
                p = make_priors(rng, B, A, shift)
                mask = (np.arange(B) % 4 != 2).astype(np.uint8)
                for alpha in ALPHAS:
                    for eps in (0.0, 0.25, 1.0):
                        for attempts in (1, 2, 16):
                            for m in (None, mask):
                                want = dirichlet_rule(seed, env, t, p, alpha, eps, attempts, m)
                                got, acc = p.copy(), np.ones((B, A), np.uint8)
                                bad = H.explore_dirichlet_host(seed, base, B, A, t, vp(got), vp(m), alpha, eps, attempts, vp(acc))
                                what = (A, B, shift, alpha, eps, attempts, m is not None)
                                assert bad == want["bad_rows"] == bad_rows_of(B, shift, m), what
                                assert np.array_equal(got.view(np.uint32), want["priors"].view(np.uint32)), what
                                rows = want["drew"].any(axis=1)
                                assert np.array_equal(acc[rows] != 0, want["accepted"][rows]), what
                                if attempts in fails and eps == 0.25 and m is None:
                                    fails[attempts] += int((~want["accepted"][rows]).sum())
                for noisy in (None, mask, np.zeros(B, np.uint8)):
                    got = np.full((B, A), 7, np.float32)
                    assert H.explore_gumbel_host(seed, base, B, A, t, vp(p), vp(noisy), vp(got)) == 0
                    _same(got, gumbel_rule(seed, env, t, p, noisy), (A, B, shift, "gumbel"))
            n, temps = make_counts(rng, B, A), make_temps(B)
            for greedy in (None, mask, np.zeros(B, np.uint8)):
                for T in (temps, 0.0, 1.0, 0.5, 3.0, float("inf"), 1e-320):
                    got = np.full(B, 7, np.int8)
                    per = isinstance(T, np.ndarray)
                    assert H.explore_temp_host(seed, base, B, A, t, vp(n), vp(greedy), vp(T) if per else None, 1.0 if per else T, vp(got)) == 0
                    _same(got, temp_rule(seed, env, t, n, greedy, T), (A, B, "temp", greedy is not None, None if per else T))
    assert fails[1] > 100 and fails[16] == 0, fails                  # both branches of the acceptance ran
    assert H.explore_dirichlet_host(1, 0, 1, 4, 0, None, None, 0.3, 0.25, 16, None) == -1


def test_the_kernels_code_runs_clean_under_the_host_sanitizers(tmp_path):
    """A stand-alone program (explore_host.cpp with its main), not code loaded into python."""
    r = run_sanitized(tmp_path, "explore_host_main", ["-DEXPLORE_HOST_MAIN"] + HOST_FLAGS, probe_timeout=300, build_timeout=600, run_timeout=300)
    assert r.stdout.count("bad ") == 54 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
