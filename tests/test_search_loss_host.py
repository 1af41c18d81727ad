"""Host: the rule of include/snac_hip.h, "Search loss (AlphaZero / Gumbel self-play)", restated in numpy (search_rule), independently of
the kernel (tests/test_gpu_search_loss.py compares them byte for byte): its loss and gradients before the rounding to float32 against a
float64 torch composition (log_softmax, mse_loss / huber_loss) and torch autograd, bad samples, both stages of the batch reduction
(tree_sums is PPO's), and the inputs the GPU test runs on (make_search_case: that they contain every sort, that every sort lands in the
branch it is meant for, and that the stated order of the sums can be told from a plain index-order sum, is asserted here).  Then
snac_search_loss is exported and checks every argument before any HIP call -- each failing call below fails its checks first, so the
placeholder pointers are never dereferenced -- and SearchLoss checks its arguments before it touches a device.  Last, the per-sample
function the kernel runs (snac_amd/csrc/search_rule.h) and a C++ restatement of the reduction are compiled for the host with the system
compiler and compared with search_rule byte for byte, and the same source runs once as a program under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os

import numpy as np
import pytest

from cabi_checks import PH, _err_code as _err
import helpers
from hostcode import load_shared, run_sanitized
from snac_amd import _lib
from specmath import _same, spec_exp, spec_log, tree_sums

ACTIONS = (3, 5, 8)
DELTA = 1.0                                                          # the Huber delta of the generated cases; 0: the squared error
DELTAS = (0.0, DELTA)
VF_COEF = 0.7
STATS = ("total", "Lpi", "Lv", "H", "ab", "agree", "good", "w")
INPUTS = ("logits", "value", "pi", "z", "weight")


# ---- the rule, in numpy: every ufunc call below is one float64 operation, rounded on its own --------------------------------------------
def _first_largest(v):
    """The stated loop: start at index 0, v[a] > best wins, ties keep the lower index."""
    best, at = v[:, 0].copy(), np.zeros(len(v), np.int64)
    for a in range(1, v.shape[1]):
        wins = v[:, a] > best
        best, at = np.where(wins, v[:, a], best), np.where(wins, a, at)
    return at


def search_rule(logits, value, pi, z, weight=None, vf_coef=1.0, delta=0.0, scale=1.0):
    """-> dict(loss, priority, grad_value float32 [B], grad_logits float32 [B, A], stats float64 [8], mean_loss float32 [1], partials
    float64 [W, 8], bad_rows int; and before the rounding to float32: per, total, GL [B, A], GV; u [B, 8] the contributions; Lpi, Lv, H,
    M, S, dv, ab, g, w [B]; x, e, p, lp, pj [B, A]; lin, agree, bad)."""
    f32 = lambda a: np.array(a, np.float32)  # noqa: E731
    l, pi32, value, z = f32(logits), f32(pi), f32(value), f32(z)
    B, A = l.shape
    with np.errstate(all="ignore"):
        m = l[:, 0].copy()
        for a in range(1, A):
            m = np.where(l[:, a] > m, l[:, a], m)
        bad = np.isnan(l).any(axis=1) | (l == np.inf).any(axis=1) | (m == -np.inf)
        bad = bad | (~np.isfinite(pi32)).any(axis=1) | (pi32 < 0).any(axis=1) | ((pi32 > 0) & (l == -np.inf)).any(axis=1)
        bad = bad | ~np.isfinite(value) | ~np.isfinite(z)
        if weight is not None:
            w32 = f32(weight)
            bad = bad | ~np.isfinite(w32) | (w32 < 0)
            w = np.where(bad, np.float32(1.0), w32).astype(np.float64)
        else:
            w = np.ones(B)
        good = ~bad
        l[bad], m[bad], pi32[bad], value[bad], z[bad] = 0.0, 0.0, 0.0, 0.0, 0.0      # (bad samples are zeroed below)
        x = l.astype(np.float64) - m.astype(np.float64)[:, None]
        e = spec_exp(x)
        S, T = np.zeros(B), np.zeros(B)
        for a in range(A):
            S = S + e[:, a]
            T = T + np.where(e[:, a] == 0.0, 0.0, e[:, a] * x[:, a])
        L = spec_log(S)
        H = L - T / S
        lp = x - L[:, None]
        p = e / S[:, None]
        pj = pi32.astype(np.float64)
        M, ce = np.zeros(B), np.zeros(B)
        for a in range(A):
            M = M + pj[:, a]
            ce = ce + np.where(pj[:, a] == 0.0, 0.0, pj[:, a] * lp[:, a])
        Lpi = -ce
        agree = _first_largest(l) == _first_largest(pi32)
        dv = value.astype(np.float64) - z.astype(np.float64)
        ab = np.abs(dv)
        d, vf, sc = np.float64(delta), np.float64(vf_coef), np.float64(scale)
        if delta == 0:
            lin = np.zeros(B, bool)
            Lv = dv * dv
            g = 2.0 * dv
        else:
            lin = ab > d
            Lv = np.where(lin, d * (ab - 0.5 * d), 0.5 * (dv * dv))
            g = np.where(lin, np.where(dv < 0, -d, d), dv)
        per = Lpi + vf * Lv
        total = w * per
        GL = np.where(l == -np.inf, 0.0, sc * (w[:, None] * (M[:, None] * p - pj)))
        GV = sc * (w * (vf * g))
        u = np.stack([total, Lpi, Lv, H, ab, agree.astype(np.float64), np.ones(B), w], axis=1)
        u = np.where(good[:, None], u, 0.0)
        z32 = lambda v: np.where(good, v.astype(np.float32), np.float32(0.0))  # noqa: E731
        loss, priority, grad_value = z32(per), z32(ab), z32(GV)
        grad_logits = np.where(good[:, None] & (l != -np.inf), GL.astype(np.float32), np.float32(0.0))
    partials, sums = tree_sums(u)
    stats = np.array([s if STATS[k] == "good" else s / np.float64(B) for k, s in enumerate(sums)], np.float64)
    return dict(loss=loss, priority=priority, grad_logits=grad_logits, grad_value=grad_value, stats=stats, mean_loss=np.array([stats[0]], np.float32),
                partials=partials, bad_rows=int(bad.sum()), bad=bad, per=per, total=total, GL=GL, GV=GV, u=u, Lpi=Lpi, Lv=Lv, H=H, M=M, dv=dv, ab=ab,
                g=g, w=w, S=S, x=x, e=e, p=p, lp=lp, pj=pj, lin=lin & good, agree=agree & good)


# ---- the inputs of tests/test_gpu_search_loss.py: the sorts of sample take turns, sample i of sort (i + shift) % len(SORTS) --------------
PLACED = {"below": 0.5, "at": 1.0, "above": 2.5}                     # |dv| in units of DELTA, exact in float32 and float64
FAR = (45.5, 60.0, 300.0)                                            # below the largest logit: EXP gives exactly 0 below -45
SORTS = ("normal", "peaked", "flat", "equal", "far_hit", "far_zero", "masked_ok", "masked_hit", "pi_first", "pi_last", "pi_mass", "pi_neg", "pi_negzero",
         "pi_bad", "pi_uniform", "logit_nan", "logit_inf", "logit_allneg", "value_bad", "z_bad", "weight_bad", "weight_zero", "below_pos", "below_neg",
         "at_pos", "at_neg", "above_pos", "above_neg", "dv_zero", "big", "big_neg", "tie_logit", "tie_pi")
BAD_ALWAYS = ("masked_hit", "pi_neg", "pi_bad", "logit_nan", "logit_inf", "logit_allneg", "value_bad", "z_bad")
BAD_WEIGHT = ("weight_bad",)
NOT_FINITE = (np.nan, np.inf, -np.inf)


def make_search_case(rng, B, A, shift=0):
    """dict(logits, pi float32 [B, A], value, z, weight float32 [B], sort: the samples' sorts)."""
    logits = (1.5 * rng.normal(size=(B, A))).astype(np.float32)
    t = rng.normal(size=(B, A))
    pi = (np.exp(t) / np.exp(t).sum(axis=1, keepdims=True)).astype(np.float32)
    value = rng.normal(size=B).astype(np.float32)
    z = rng.normal(size=B).astype(np.float32)
    weight = (0.1 + 0.9 * rng.random(size=B)).astype(np.float32)
    sorts = [SORTS[(i + shift) % len(SORTS)] for i in range(B)]
    for i, sort in enumerate(sorts):
        turn = i // len(SORTS)
        top = int(logits[i].argmax())
        j = (top + 1 + int(rng.integers(A - 1))) % A                 # a place that does not hold the largest logit
        kind, _, sign = sort.partition("_")
        if sort == "peaked":
            logits[i, top] += np.float32(20.0)
        elif sort == "flat":
            logits[i] *= np.float32(0.01)
        elif sort == "equal":
            logits[i] = logits[i, 0]
        elif sort in ("far_hit", "far_zero"):                        # finite, and more than 45 below the largest: no weight
            logits[i, j] = logits[i, top] - np.float32(FAR[turn % 3])
            if sort == "far_zero":
                pi[i, j] = 0.0
        elif sort in ("masked_ok", "masked_hit"):
            logits[i, j] = -np.inf
            if sort == "masked_ok":
                pi[i, j] = 0.0
                if turn % 2:                                         # a second masked action
                    k = [a for a in range(A) if a not in (top, j)][int(rng.integers(A - 2))]
                    logits[i, k], pi[i, k] = -np.inf, 0.0
        elif sort in ("pi_first", "pi_last"):                        # one-hot at the first and at the last index
            pi[i] = 0.0
            pi[i, 0 if sort == "pi_first" else A - 1] = 1.0
        elif sort == "pi_mass":                                      # a mass that is not 1, and no mass at all
            pi[i] *= np.float32((0.5, 2.0, 0.0)[turn % 3])
        elif sort == "pi_neg":
            pi[i, j] = (-0.5, -1e-30)[turn % 2]
        elif sort == "pi_negzero":
            pi[i, j] = -0.0
        elif sort == "pi_bad":
            pi[i, (0, A - 1, j)[turn % 3]] = NOT_FINITE[turn % 3]
        elif sort == "pi_uniform":
            pi[i] = np.float32(1.0 / A)
        elif sort == "logit_nan":
            logits[i, (0, A - 1)[turn % 2]] = np.nan
        elif sort == "logit_inf":
            logits[i, (0, A - 1)[turn % 2]] = np.inf
        elif sort == "logit_allneg":
            logits[i] = -np.inf
            if turn % 2:
                pi[i] = 0.0                                          # no target on a masked action: the scan alone says bad
        elif sort == "value_bad":
            value[i] = NOT_FINITE[turn % 3]
        elif sort == "z_bad":
            z[i] = NOT_FINITE[turn % 3]
        elif sort == "weight_bad":
            weight[i] = (np.nan, np.inf, -np.inf, -0.5)[turn % 4]
        elif sort == "weight_zero":
            weight[i] = 0.0
        elif kind in PLACED or sort == "dv_zero":
            z[i] = np.float32(np.round(8.0 * z[i]) / 8.0)
            off = 0.0 if sort == "dv_zero" else PLACED[kind] * DELTA * (1.0 if sign == "pos" else -1.0)
            value[i] = np.float32(np.float64(z[i]) + off)
            assert np.float64(value[i]) - np.float64(z[i]) == off
        elif sort in ("big", "big_neg"):                             # magnitudes 1 and 1e3 (squared: 1e6) in one sum: the order of the additions shows
            value[i] = np.float32((1.0 if sort == "big" else -1.0) * 1e3 * (1.0 + rng.random()))
        elif sort in ("tie_logit", "tie_pi"):                        # the two largest are equal: the lower index is the first largest
            j1, j2 = sorted(rng.choice(A, size=2, replace=False))
            tied, other = (logits, pi) if sort == "tie_logit" else (pi, logits)
            tied[i, j1] = tied[i, j2] = np.float32(np.abs(tied[i]).max() + 1.0)
            other[i, (j1, j2)[turn % 2]] = np.float32(np.abs(other[i]).max() + 1.0)      # agrees at j1, not at j2
    return dict(logits=logits, value=value, pi=pi, z=z, weight=weight, sort=np.array(sorts))


def bad_sorts(weighted):
    return BAD_ALWAYS + (BAD_WEIGHT if weighted else ())


def bad_rows_of(B, shift=0, weighted=True):
    """From the generator alone: how many samples of make_search_case(rng, B, A, shift) are bad."""
    bad = bad_sorts(weighted)
    return sum(SORTS[(i + shift) % len(SORTS)] in bad for i in range(B))


def rule_of(c, weighted=True, delta=DELTA, scale=1.0, vf_coef=VF_COEF):
    return search_rule(c["logits"], c["value"], c["pi"], c["z"], c["weight"] if weighted else None, vf_coef, delta, scale)


def _cases(rows=len(SORTS) * 48):
    for A in ACTIONS:
        yield A, make_search_case(np.random.default_rng(A), rows, A)


def plain_sum(col):
    s = np.float64(0.0)
    for t in col:
        s = s + t
    return s


def test_the_generated_inputs_contain_every_sort_in_its_branch_and_the_order_of_the_sums_shows():
    for A, c in _cases():
        sort = c["sort"]
        B = len(sort)
        n = B // len(SORTS)
        assert set(sort) == set(SORTS)
        l, pi = c["logits"], c["pi"]
        for weighted in (False, True):
            out, sq = rule_of(c, weighted), rule_of(c, weighted, delta=0.0)
            want = bad_sorts(weighted)
            assert out["bad_rows"] == sq["bad_rows"] == bad_rows_of(B, 0, weighted) == n * len(want)
            assert set(sort[out["bad"]]) == set(want), (weighted, set(sort[out["bad"]]) ^ set(want))
            good = ~out["bad"]
            assert np.isfinite(out["u"]).all() and np.isfinite(out["stats"]).all() and np.isfinite(out["GL"][good]).all()
            for kind, k in PLACED.items():                           # below, at and above delta, both signs; exactly at it: not linear
                for sign, s in (("pos", 1.0), ("neg", -1.0)):
                    at = sort == "%s_%s" % (kind, sign)
                    assert at.sum() >= 3 and (out["dv"][at] == s * k * DELTA).all() and out["lin"][at].all() == (kind == "above")
                    assert out["lin"][at].any() == (kind == "above")
            assert not out["dv"][sort == "dv_zero"].any() and not out["GV"][sort == "dv_zero"].any() and not sq["lin"].any()
            big = out["ab"][good]
            assert (big > 1e3).any() and (big < 1.0).any()
            # a finite logit more than 45 below the largest: no weight, a finite log-probability; with a target there the gradient is
            # -scale w pi, without one it is zero
            for k in ("far_hit", "far_zero"):
                at = np.nonzero(sort == k)[0]
                far = (out["x"][at] < -45.0) & np.isfinite(out["x"][at])
                assert good[at].all() and (far.sum(axis=1) >= 1).all() and not out["e"][at][far].any() and np.isfinite(out["lp"][at]).all()
                hit = out["pj"][at][far] > 0
                assert hit.all() == hit.any() == (k == "far_hit")
                assert np.array_equal(out["GL"][at][far], -(out["w"][at][:, None] * out["pj"][at])[far])
                assert {float(v) for v in np.round(-out["x"][at][far], 1)} >= set(FAR)
            assert out["GL"][sort == "far_hit"].any() and (out["Lpi"][sort == "far_hit"] > 45.0 * pi[sort == "far_hit"].min(axis=1)).all()
            ok = sort == "masked_ok"
            masked = l[ok] == -np.inf
            assert good[ok].all() and set(masked.sum(axis=1)) == {1, 2} and not pi[ok][masked].any() and not out["GL"][ok][masked].any()
            assert np.isfinite(out["Lpi"][ok]).all() and ((l[sort == "masked_hit"] == -np.inf) & (pi[sort == "masked_hit"] > 0)).any(axis=1).all()
            first, last = sort == "pi_first", sort == "pi_last"
            assert (out["M"][first] == 1.0).all() and np.array_equal(out["Lpi"][first], -out["lp"][first, 0])
            assert (out["M"][last] == 1.0).all() and np.array_equal(out["Lpi"][last], -out["lp"][last, A - 1])
            mass = out["M"][sort == "pi_mass"]
            assert (mass == 0.0).any() and (np.abs(mass - 0.5) < 1e-6).any() and (np.abs(mass - 2.0) < 1e-6).any()
            assert not out["Lpi"][(sort == "pi_mass") & (out["M"] == 0.0)].any()
            nz = sort == "pi_negzero"
            assert good[nz].all() and (np.signbit(pi[nz]) & (pi[nz] == 0)).any(axis=1).all()
            assert (out["S"][sort == "equal"] == A).all() and (out["S"][good] >= 1.0).all() and (out["S"][good] <= A).all()
            assert np.allclose(out["H"][sort == "equal"], np.log(A), rtol=0, atol=1e-11)
            assert (out["H"][sort == "peaked"] < 0.5 * out["H"][sort == "flat"]).all()
            for k, tied in (("tie_logit", l), ("tie_pi", pi)):       # the lower index of the tied pair is the first largest: agrees every other turn
                at = sort == k
                assert ((tied[at] == tied[at].max(axis=1, keepdims=True)).sum(axis=1) == 2).all()
                assert out["agree"][at].tolist() == [t % 2 == 0 for t in range(n)]
            assert out["agree"][good].any() and not out["agree"][good].all() and 0 < out["stats"][5] < 1
            if weighted:
                assert not out["total"][sort == "weight_zero"].any() and out["per"][sort == "weight_zero"].all()
                assert not out["GL"][sort == "weight_zero"].any() and not out["GV"][sort == "weight_zero"].any()
        neg = pi[sort == "pi_neg"]
        assert (neg == -0.5).any() and (neg == np.float32(-1e-30)).any() and ((neg < 0).sum(axis=1) == 1).all()
        for k, v in (("pi_bad", pi[sort == "pi_bad"]), ("value_bad", c["value"][sort == "value_bad"]), ("z_bad", c["z"][sort == "z_bad"]),
                     ("weight_bad", c["weight"][sort == "weight_bad"])):
            assert np.isnan(v).any() and (v == np.inf).any() and (v == -np.inf).any(), k
        assert (c["weight"][sort == "weight_bad"] == -0.5).any()
        assert np.isnan(l[sort == "logit_nan"]).sum(axis=1).tolist() == [1] * n and np.isnan(l[sort == "logit_nan"][:, [0, A - 1]]).any(axis=0).all()
        assert (l[sort == "logit_inf"] == np.inf).sum(axis=1).tolist() == [1] * n and (l[sort == "logit_allneg"] == -np.inf).all()
    # the stated tree against a plain sum in index order: at B = 4097 they differ in at least one bit, so the GPU test can tell them apart
    B = 4097
    for A in ACTIONS:
        out = rule_of(make_search_case(np.random.default_rng(100 * A + B), B, A, B % len(SORTS)))
        plain, tree = plain_sum(out["u"][:, 0]), tree_sums(out["u"])[1][0]
        assert np.float64(plain).tobytes() != np.float64(tree).tobytes(), (A, plain, tree)
        assert abs(plain - tree) <= 1e-9 * np.abs(out["u"][:, 0]).sum()                          # the same sum, in another order


# ---- against float64 torch and autograd --------------------------------------------------------------------------------------------------
ROUND = 2.0 ** -48                                                   # a few dozen float64 roundings, each 2^-53 relative
EPS_EXP, DELTA_LOG = 2e-12, 1e-12
FLOOR = np.exp(-45.0)                                                # EXP returns exactly 0 below -45: the true probability there is up to this
MASK = -1.0e4                                                        # the reference's stand-in for a -inf logit: exp(MASK - m) is 0.0 in float64


def _torch_reference(c, weighted, delta, scale, vf_coef, rows):
    """(ce, Lv, total, d (scale * total) / dlogits, d / dvalue) of `rows` in float64 torch: log_softmax, mse_loss / huber_loss, autograd.
    A masked action's logit is MASK: its probability is exactly 0 and 0 * its finite log-probability is 0, where -inf would give a NaN."""
    import torch
    import torch.nn.functional as F

    t = lambda a: torch.tensor(np.asarray(a, np.float64)[rows], dtype=torch.float64)  # noqa: E731
    l = torch.tensor(np.nan_to_num(c["logits"].astype(np.float64)[rows], neginf=MASK), dtype=torch.float64, requires_grad=True)
    v = t(c["value"]).requires_grad_()
    ce = -(t(c["pi"]) * torch.log_softmax(l, dim=1)).sum(dim=1)
    Lv = F.mse_loss(v, t(c["z"]), reduction="none") if delta == 0 else F.huber_loss(v, t(c["z"]), reduction="none", delta=delta)
    per = ce + vf_coef * Lv
    total = t(c["weight"]) * per if weighted else per
    (scale * total).sum().backward()
    return ce.detach().numpy(), Lv.detach().numpy(), total.detach().numpy(), l.grad.numpy(), v.grad.numpy()


def test_loss_and_gradients_stay_within_the_derived_bound_of_float64_torch_and_autograd():
    """The bound is derived, not fitted to what is seen (which is printed).  The policy part follows the C51 bound of
    tests/test_qloss_host.py, from the header's 1e-12 on EXP and LOG: EXP is within eps = 2e-12 relative, so S is (a sum of positive terms),
    and L = LOG(S) and every lp_a = x_a - L are within err_l = 1e-12 + 2 eps absolute; p_a = e_a / S is within 2 eps relative -- except
    where EXP cuts: below -45 it returns exactly 0 where the true probability is up to e^-45 = 2.9e-20, an absolute error of p_a that the
    relative bound does not cover.  With Mabs = sum |pi_a|:
        ce          = -sum pi_a lp_a:             <= Mabs err_l + ROUND (sum |pi_a lp_a| + 1)
        grad_logits = scale w (M p_a - pi_a):     <= |scale| w (2 eps |M| p_a + |M| e^-45 + ROUND (Mabs p_a + |pi_a|))
    The value part is TD's bound: dv = value - z is one rounding of numbers up to V = |value| + |z|, so
        Lv          <= ROUND ((|dv| + delta) V + Lv)          grad_value <= |scale| w vf_coef ROUND (V + |g|)
        total = w (ce + vf_coef Lv):              <= w (bound of ce + vf_coef bound of Lv) + ROUND |total|
    with ROUND = 2^-48 for the few dozen roundings (the reference's among them).  Every good sample is compared; none is left out."""
    seen = np.zeros(5)
    rows_seen = 0
    err_l = DELTA_LOG + 2.0 * EPS_EXP
    tiny = 1e-300
    for A, c in _cases(len(SORTS) * 96):
        for weighted in (False, True):
            for delta in DELTAS:
                for scale in (1.0, 1.0 / 4096.0):
                    out = rule_of(c, weighted, delta, scale)
                    rows = ~out["bad"]
                    assert rows.sum() >= len(rows) // 2
                    ce, Lv, total, GL, GV = _torch_reference(c, weighted, delta, scale, VF_COEF, rows)
                    pj, p, w, M = out["pj"][rows], out["p"][rows], out["w"][rows], np.abs(out["M"][rows])
                    lp = np.where(pj == 0.0, 0.0, out["lp"][rows])
                    mabs = np.abs(pj).sum(axis=1)
                    b_ce = mabs * err_l + ROUND * (np.abs(pj * lp).sum(axis=1) + 1.0)
                    b_gl = abs(scale) * w[:, None] * (2.0 * EPS_EXP * M[:, None] * p + M[:, None] * FLOOR + ROUND * (mabs[:, None] * p + np.abs(pj))) + tiny
                    V = np.abs(c["value"].astype(np.float64)[rows]) + np.abs(c["z"].astype(np.float64)[rows])
                    ab, g = out["ab"][rows], np.abs(out["g"][rows])
                    b_lv = ROUND * ((ab + delta) * V + out["Lv"][rows]) + tiny
                    b_gv = abs(scale) * w * VF_COEF * ROUND * (V + g) + tiny
                    b_total = w * (b_ce + VF_COEF * b_lv) + ROUND * np.abs(out["total"][rows]) + tiny
                    ratios = (np.abs(out["Lpi"][rows] - ce) / b_ce, np.abs(out["Lv"][rows] - Lv) / b_lv, np.abs(out["total"][rows] - total) / b_total,
                              (np.abs(out["GL"][rows] - GL) / b_gl).max(axis=1), np.abs(out["GV"][rows] - GV) / b_gv)
                    seen = np.maximum(seen, [x.max() for x in ratios])
                    rows_seen += int(rows.sum())
                    for name, x in zip(("ce", "value error", "total", "grad_logits", "grad_value"), ratios):
                        assert x.max() <= 1.0, (A, weighted, delta, scale, name, x.max(), c["sort"][rows][x.argmax()])
    print("largest error / bound: ce %.3g, value error %.3g, total %.3g, grad_logits %.3g, grad_value %.3g over %d rows" % (*seen, rows_seen))


def test_bad_samples_give_zeros_add_nothing_and_are_counted():
    for A, c in _cases():
        B = len(c["sort"])
        for weighted in (False, True):
            for delta in DELTAS:
                out = rule_of(c, weighted, delta, 1.0 / B)
                bad = out["bad"]
                assert out["bad_rows"] == bad.sum() == bad_rows_of(B, 0, weighted) > 0
                for k in ("loss", "priority", "grad_logits", "grad_value"):
                    assert out[k].dtype == np.float32 and not out[k][bad].view(np.uint32).any() and np.isfinite(out[k]).all(), k
                assert not out["u"][bad].any() and not np.signbit(out["u"][bad]).any() and out["stats"][6] == B - out["bad_rows"]
                assert out["mean_loss"].dtype == np.float32 and out["mean_loss"][0] == np.float32(out["stats"][0])
                assert abs(out["stats"][0] - out["total"][~bad].sum() / B) <= 1e-12 * np.abs(out["total"][~bad]).sum() / B
                assert np.array_equal(out["priority"][~bad], out["ab"][~bad].astype(np.float32))
                assert not out["grad_logits"][c["logits"] == -np.inf].view(np.uint32).any()      # a masked action: exactly +0.0
                if not weighted:
                    assert abs(out["stats"][0] - (out["stats"][1] + VF_COEF * out["stats"][2])) <= 1e-12 * abs(out["stats"][0])
                    assert out["stats"][7] == out["stats"][6] / B
                # the gradient of a row sums to zero where the target has mass 1 and nothing is cut or masked
                unit = ~bad & (np.abs(out["M"] - 1.0) < 1e-6) & (out["e"] != 0).all(axis=1)
                assert unit.sum() > B // 4 and (np.abs(out["GL"][unit].sum(axis=1)) <= 1e-6 / B).all()


# ---- the C entry point -------------------------------------------------------------------------------------------------------------------
def _sl(L, B=4, A=5, logits=PH, value=PH, pi=PH, z=PH, weight=PH, vf_coef=1.0, delta=1.0, scale=1.0, loss=PH, prio=PH, gl=PH, gv=PH, stats=PH,
        mean=PH, partials=PH, bad=PH):
    return L.snac_search_loss(B, A, logits, value, pi, z, weight, vf_coef, delta, scale, loss, prio, gl, gv, stats, mean, partials, bad, None)


def test_the_library_exports_the_entry_point():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    assert "snac_search_loss" in _lib.EXPORTS and len(L.snac_search_loss.argtypes) == 19 and _lib.SEARCH_STATS == 8
    res, args = _lib.PROTOTYPES["snac_search_loss"]
    assert res == C.c_int and args[:2] == [C.c_int32, C.c_int32] and args[7:10] == [C.c_double] * 3
    assert all(t == C.c_void_p for t in args[2:7] + args[10:])


def test_search_loss_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    for k in ("logits", "value", "pi", "z"):
        _err(L, _sl(L, **{k: None}), -1, b"null " + k.encode())
    for B in (0, -1, -(1 << 31)):
        _err(L, _sl(L, B=B), -1, b"B must be >= 1")
    for x in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        _err(L, _sl(L, vf_coef=x), -1, b"vf_coef must be finite and >= 0")
        _err(L, _sl(L, delta=x), -1, b"delta must be finite and >= 0")
    for x in (float("nan"), float("inf"), float("-inf")):
        _err(L, _sl(L, scale=x), -1, b"scale must be finite")
    _err(L, _sl(L, partials=None), -1, b"partials are needed for stats")
    _err(L, _sl(L, stats=None), -1, b"stats is needed")
    _err(L, _sl(L, stats=C.c_void_p((1 << 20) + 4)), -1, b"stats and partials must be 8-byte aligned")
    _err(L, _sl(L, partials=C.c_void_p((1 << 20) + 4)), -1, b"stats and partials must be 8-byte aligned")
    for A in (0, 1, 2, 4, 6, 7, 9, -3):
        _err(L, _sl(L, A=A), -3, b"num_actions must be 3, 5 or 8")
    # no output: no launch, although no device exists to launch on -- but the checks come first
    none = dict(loss=None, prio=None, gl=None, gv=None, stats=None, mean=None, bad=None)
    for A in ACTIONS:
        assert _sl(L, A=A, **none) == 0 and _sl(L, A=A, partials=None, **none) == 0
        assert _sl(L, A=A, weight=None, delta=0.0, vf_coef=0.0, scale=-2.0, **none) == 0
    _err(L, _sl(L, B=0, **none), -1, b"B must be >= 1")
    _err(L, _sl(L, A=4, **none), -3, b"num_actions must be")
    _err(L, _sl(L, delta=-1.0, **none), -1, b"delta must be finite")
    _err(L, _sl(L, pi=None, **none), -1, b"null pi")


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------------
def test_search_loss_checks_its_arguments_before_it_touches_a_device():
    import torch
    from snac_amd import SearchLoss

    ok = dict(num_actions=5, device="cuda:0")
    for bad in (dict(num_actions=4), dict(num_actions=True), dict(num_actions="5"), dict(num_actions=5.0), dict(device="cpu"), dict(device=None),
                dict(huber=0.0), dict(huber=-1.0), dict(huber=float("nan")), dict(huber=float("inf")), dict(huber="1"), dict(huber=True),
                dict(vf_coef=-0.5), dict(vf_coef=float("nan")), dict(vf_coef=float("inf")), dict(vf_coef="1"), dict(vf_coef=True), dict(vf_coef=None)):
        with pytest.raises(ValueError):
            SearchLoss(**dict(ok, **bad))
    sl = SearchLoss(5, device="cuda:0")
    assert sl.num_actions == 5 and sl.device == torch.device("cuda:0") and sl.env is None and sl.stats is None
    assert sl.delta == 0.0 and sl.vf_coef == 1.0
    other = SearchLoss(3, 0, 1, "cuda:0")
    assert other.vf_coef == 0.0 and other.delta == 1.0 and SearchLoss(8, vf_coef=0.5, huber=0.5, device="cuda:0").delta == 0.5
    with pytest.raises(ValueError, match="no loss"):
        sl.stats_dict()
    l, v, pi = torch.zeros(4, 5), torch.zeros(4), torch.zeros(4, 5)
    for mb in (dict(), dict(pi=pi), dict(z=v), dict(weight=v)):
        with pytest.raises(ValueError, match="mb must hold pi and z"):
            sl.loss(l, v, mb)
    for mb in ((), (pi,), (pi, v, v, v), 5, None):
        with pytest.raises(ValueError, match="mb must be a minibatch dict or the tuple"):
            sl.loss(l, v, mb)
    with pytest.raises(ValueError, match=r"logits must have shape \(B, 5\), got \(4, 3\)"):
        sl.loss(torch.zeros(4, 3), v, (pi, v))
    with pytest.raises(ValueError, match="logits must have shape"):
        sl.loss(torch.zeros(0, 5), v[:0], (pi[:0], v[:0]))
    with pytest.raises(ValueError, match="logits must be a contiguous torch.float32 tensor"):
        sl.loss(l.double(), v, (pi, v))
    with pytest.raises(ValueError, match="logits must be a contiguous torch.float32 tensor"):
        sl.loss(torch.zeros(4, 6)[:, :5], v, (pi, v))                # the slice of a network's joint output: .contiguous() is the caller's
    with pytest.raises(ValueError, match="logits must be on cuda:0"):
        sl.loss(l, v, (pi, v))
    with pytest.raises(ValueError, match="logits must be on cuda:0"):
        sl.loss(l.requires_grad_(), v, dict(pi=pi, z=v, weight=v), want_per_sample=True)


# ---- the kernel's code on the host -------------------------------------------------------------------------------------------------------
OUTPUTS = ("loss", "priority", "grad_logits", "grad_value", "stats", "mean_loss", "partials")
HOST_SRC = os.path.join(helpers.TESTS, "native", "search_host.cpp")
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", _lib.CSRC, HOST_SRC]


def test_the_kernels_code_compiled_for_the_host_equals_the_rule_byte_for_byte(tmp_path):
    fn = load_shared(tmp_path, "search_host", ["-O2", "-fPIC", "-shared"] + HOST_FLAGS, timeout=600).search_host
    fn.restype, fn.argtypes = C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_double] * 3 + [C.c_void_p] * 7
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def ins(c, weighted):
        return [vp(c["logits"]), vp(c["value"]), vp(c["pi"]), vp(c["z"]), vp(c["weight"]) if weighted else None]
    for A in ACTIONS:
        for B in (1, 64, 65, 4097, 8193):
            shifts = range(len(SORTS)) if B == 1 else (B % len(SORTS),)
            for shift in shifts:
                c = make_search_case(np.random.default_rng(100 * A + B + shift), B, A, shift)
                for weighted, delta in ((True, DELTA), (False, 0.0), (True, 0.0), (False, DELTA)):
                    want = rule_of(c, weighted, delta, 1.0 / B)
                    W = (B + 63) // 64
                    got = dict(loss=np.full(B, 7, np.float32), priority=np.full(B, 7, np.float32), grad_logits=np.full((B, A), 7, np.float32),
                               grad_value=np.full(B, 7, np.float32), stats=np.full(8, 7, np.float64), mean_loss=np.full(1, 7, np.float32),
                               partials=np.full((W, 8), 7, np.float64))
                    bad = fn(B, A, *ins(c, weighted), VF_COEF, delta, 1.0 / B, *[vp(got[k]) for k in OUTPUTS])
                    assert bad == want["bad_rows"] == bad_rows_of(B, shift, weighted), (A, B, shift, weighted, bad, want["bad_rows"])
                    for k in OUTPUTS:
                        _same(got[k], want[k], (A, B, shift, weighted, delta, k))
    # no statistics asked for: stats, mean_loss and partials are not touched
    prio = np.full(B, 7, np.float32)
    assert fn(B, A, *ins(c, False), VF_COEF, 0.0, 1.0, None, vp(prio), None, None, None, None, None) == bad_rows_of(B, shift, False)
    _same(prio, rule_of(c, False, 0.0)["priority"], "the priorities alone")


def test_the_kernels_code_runs_clean_under_the_host_sanitizers(tmp_path):
    """A stand-alone program (search_host.cpp with its main), not code loaded into python."""
    r = run_sanitized(tmp_path, "search_host_main", ["-DSEARCH_HOST_MAIN"] + HOST_FLAGS, probe_timeout=300, build_timeout=600, run_timeout=300)
    assert r.stdout.count("bad ") == 36 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
