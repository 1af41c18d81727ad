"""Host: the rule of include/snac_hip.h, "Q-learning losses", restated in numpy (td_rule), independently of the kernels
(tests/test_gpu_qloss.py compares them with it byte for byte): its loss and gradient before the rounding to float32 against a float64
torch composition (mse_loss / huber_loss) and torch autograd, bad samples, both stages of the batch reduction (tree_sums is PPO's), and
the inputs the GPU test runs on (make_case: that they contain every sort, that every sort lands in the branch it is meant for, and that
the stated order of the sums can be told from a plain index-order sum, is asserted here).  Then snac_td_loss is exported and checks every
argument before any HIP call -- each failing call below fails its checks first, so the placeholder pointers are never dereferenced --
and TDLoss checks its arguments before it touches a device.  Last, the per-sample function the kernel runs (snac_amd/csrc/td_rule.h) and
a C++ restatement of the reduction are compiled for the host with the system compiler and compared with td_rule byte for byte, and the
same source runs once as a program under the address and undefined-behaviour sanitizers.  The second half does the same for
snac_c51_loss (c51_loss_rule, make_c51_case, float64 log_softmax and autograd, LOG over [1, 64], the entry point and
CategoricalSupport.loss); its kernel has no host form: lane = atom."""
import ctypes as C
import os

import numpy as np
import pytest

from cabi_checks import PH, _err_code as _err
import helpers
from hostcode import load_shared, run_sanitized
from snac_amd import _lib
from specmath import _same, spec_exp, spec_log, tree_sums

assert {"snac_td_loss", "snac_c51_loss"} <= set(_lib.EXPORTS), "include/snac_hip.h declares the entry points this file is about"

ACTIONS = (3, 5, 8)
DELTA = 1.0                                                          # the Huber delta of the generated cases; 0: the squared error
DELTAS = (0.0, DELTA)
MODES = ("y", "next", "double")                                      # the target: y; from q_next, chosen on q_next; chosen on q_select
STATS = ("total", "L", "ab", "qa", "yv", "lin", "good", "w")
INPUTS = ("q", "action", "y", "q_next", "q_select", "ret", "discount", "weight")


# ---- the rule, in numpy: every ufunc call below is one float64 operation, rounded on its own --------------------------------------------
def td_rule(q, action, y=None, q_next=None, q_select=None, ret=None, discount=None, weight=None, delta=0.0, scale=1.0):
    """-> dict(loss, priority, y_out float32 [B], grad_q float32 [B, A], stats float64 [8], mean_loss float32 [1], partials float64
    [W, 8], bad_rows int; and before the rounding to float32: L, total, GQ; u [B, 8] the contributions; td, ab, yv [B]; lin, a_star,
    bad).  y given: mode Y; else mode NEXT on q_next, ret, discount and, if given, q_select."""
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    q = f32(q)
    B, A = q.shape
    action = np.asarray(action, np.int64)
    rows = np.arange(B)
    bad = (action < 0) | (action >= A)
    act = np.where(bad, 0, action)
    qa = np.where(bad, np.float32(0.0), q[rows, act])
    bad = bad | ~np.isfinite(qa)
    a_star = np.zeros(B, np.int64)
    with np.errstate(all="ignore"):
        if y is None:
            nxt = f32(q_next)
            s = nxt if q_select is None else f32(q_select)
            best = s[:, 0].copy()
            for a in range(1, A):
                wins = s[:, a] > best                                # a NaN never compares greater; ties keep the lower index
                best = np.where(wins, s[:, a], best)
                a_star = np.where(wins, a, a_star)
            qn = nxt[rows, a_star]
            ret, discount = f32(ret), f32(discount)
            bad = bad | ~np.isfinite(ret) | ~np.isfinite(discount) | (discount < 0) | ~np.isfinite(qn)
            yv = ret.astype(np.float64) + discount.astype(np.float64) * qn.astype(np.float64)
        else:
            y = f32(y)
            bad = bad | ~np.isfinite(y)
            yv = y.astype(np.float64)
        if weight is not None:
            w32 = f32(weight)
            bad = bad | ~np.isfinite(w32) | (w32 < 0)
            w = w32.astype(np.float64)
        else:
            w = np.ones(B)
        good = ~bad
        td = qa.astype(np.float64) - yv
        ab = np.abs(td)
        d, sc = np.float64(delta), np.float64(scale)
        if delta == 0:
            lin = np.zeros(B, bool)
            L = td * td
            g = 2.0 * td
        else:
            lin = ab > d
            L = np.where(lin, d * (ab - 0.5 * d), 0.5 * (td * td))
            g = np.where(lin, np.where(td < 0, -d, d), td)
        total = w * L
        GA = sc * (w * g)
        onehot = (np.arange(A)[None, :] == act[:, None]) & good[:, None]
        GQ = np.where(onehot, GA[:, None], 0.0)
        u = np.stack([total, L, ab, qa.astype(np.float64), yv, lin.astype(np.float64), np.ones(B), w], axis=1)
        u = np.where(good[:, None], u, 0.0)
        z32 = lambda v: np.where(good, v.astype(np.float32), np.float32(0.0))  # noqa: E731
        loss, priority, y_out = z32(L), z32(ab), z32(yv)
        grad_q = np.where(onehot, GA.astype(np.float32)[:, None], np.float32(0.0))
    partials, sums = tree_sums(u)
    stats = np.array([s if STATS[k] == "good" else s / np.float64(B) for k, s in enumerate(sums)], np.float64)
    return dict(loss=loss, priority=priority, y_out=y_out, grad_q=grad_q, stats=stats, mean_loss=np.array([stats[0]], np.float32), partials=partials,
                bad_rows=int(bad.sum()), bad=bad, L=L, total=total, GQ=GQ, u=u, td=td, ab=ab, yv=yv, lin=lin & good, a_star=a_star, w=w, g=g)


# ---- the inputs of tests/test_gpu_qloss.py: the sorts of sample take turns, sample i of sort (i + shift) % len(SORTS) --------------------
PLACED = {"below": 0.5, "at": 1.0, "above": 2.5}                     # |td| in units of DELTA, exact in float32 and float64
SORTS = ("normal", "below_pos", "below_neg", "at_pos", "at_neg", "above_pos", "above_neg", "td_zero", "tie", "sel_nan_first", "sel_nan_last",
         "q_untaken", "next_unchosen", "action_bad", "qa_bad", "qn_bad", "ret_bad", "discount_bad", "discount_neg", "y_bad", "weight_bad",
         "weight_zero", "big", "big_neg", "done")
BAD_ALWAYS = ("action_bad", "qa_bad")
BAD_NEXT = ("qn_bad", "ret_bad", "discount_bad", "discount_neg")     # bad where the target comes from q_next
BAD_Y = ("y_bad",)
BAD_WEIGHT = ("weight_bad",)
NOT_FINITE = (np.nan, np.inf, -np.inf)


def make_case(rng, B, A, shift=0):
    """dict(q, q_next, q_select float32 [B, A], action int64 [B], y, ret, discount, weight float32 [B], sort: the samples' sorts).  The
    placed sorts (below / at / above DELTA, td_zero) have a target that is exact in every mode: discount 0, or discount 0.5 over a row
    of q_next whose values are all the same multiple of 1/4; y is the same number."""
    q = (2.0 * rng.normal(size=(B, A))).astype(np.float32)
    q_next = (2.0 * rng.normal(size=(B, A))).astype(np.float32)
    q_select = (q_next + rng.normal(size=(B, A))).astype(np.float32)
    action = rng.integers(0, A, size=B).astype(np.int64)
    ret = rng.normal(size=B).astype(np.float32)
    discount = np.full(B, 0.97, np.float32)
    y = (2.0 * rng.normal(size=B)).astype(np.float32)
    weight = (0.1 + 0.9 * rng.random(size=B)).astype(np.float32)
    sorts = [SORTS[(i + shift) % len(SORTS)] for i in range(B)]
    for i, sort in enumerate(sorts):
        turn = i // len(SORTS)
        a = int(action[i])
        other = (a + 1 + int(rng.integers(A - 1))) % A               # an action that is not the taken one
        kind, _, sign = sort.partition("_")
        if kind in PLACED or sort == "td_zero":
            ret[i] = np.float32(np.round(8.0 * ret[i]) / 8.0)
            if turn % 2:
                v = np.float32(np.round(4.0 * q_next[i, 0]) / 4.0)
                q_next[i], discount[i] = v, 0.5
                target = np.float64(ret[i]) + 0.5 * np.float64(v)
            else:
                discount[i] = 0.0
                target = np.float64(ret[i])
            y[i] = np.float32(target)
            off = 0.0 if sort == "td_zero" else PLACED[kind] * DELTA * (1.0 if sign == "pos" else -1.0)
            q[i, a] = np.float32(target + off)
            assert np.float64(y[i]) == target and np.float64(q[i, a]) - target == off
        elif sort == "tie":                                          # the two largest of q_select are equal: the lower index is chosen
            j1, j2 = sorted(rng.choice(A, size=2, replace=False))
            q_select[i, j1] = q_select[i, j2] = np.float32(np.abs(q_select[i]).max() + 1.0)
            q_next[i, j2] = np.float32(q_next[i, j1] + 3.0)
        elif sort == "sel_nan_first":
            q_select[i, 0] = np.nan
        elif sort == "sel_nan_last":
            q_select[i, A - 1] = np.nan
        elif sort == "q_untaken":
            q[i, other] = NOT_FINITE[turn % 3]
        elif sort in ("next_unchosen", "qn_bad"):
            if sort == "qn_bad" and turn % 2 == 0:
                c, value = 0, np.nan                                 # a NaN at the first place stays the best: no later compare succeeds
            else:
                c, value = int(rng.integers(A)), np.inf
            top = np.float32(max(np.abs(q_select[i]).max(), np.abs(q_next[i]).max()) + 1.0)
            q_select[i, c] = q_next[i, c] = top                      # c is chosen on q_select and on q_next
            if sort == "qn_bad":
                q_next[i, c] = value
            else:                                                    # a later place that is not chosen: a NaN or -inf there never wins
                o = [j for j in range(1, A) if j != c][int(rng.integers(A - 2))]
                q_next[i, o] = (np.nan, -np.inf)[turn % 2]
        elif sort == "action_bad":
            action[i] = (-1, A, 1 << 32, -(1 << 63))[turn % 4]       # 1 << 32: its low word is a valid action
        elif sort == "qa_bad":
            q[i, a] = NOT_FINITE[turn % 3]
        elif sort == "ret_bad":
            ret[i] = NOT_FINITE[turn % 3]
        elif sort == "discount_bad":
            discount[i] = NOT_FINITE[turn % 3]
        elif sort == "discount_neg":
            discount[i] = (-0.5, -1e-30)[turn % 2]
        elif sort == "y_bad":
            y[i] = NOT_FINITE[turn % 3]
        elif sort == "weight_bad":
            weight[i] = (np.nan, np.inf, -np.inf, -0.5)[turn % 4]
        elif sort == "weight_zero":
            weight[i] = 0.0
        elif sort in ("big", "big_neg"):                             # magnitudes 1 and 1e3 in one sum: the order of the additions shows
            q[i, a] = np.float32((1.0 if sort == "big" else -1.0) * 1e3 * (1.0 + rng.random()))
        elif sort == "done":
            discount[i] = 0.0
    return dict(q=q, action=action, y=y, q_next=q_next, q_select=q_select, ret=ret, discount=discount, weight=weight, sort=np.array(sorts))


def bad_sorts(mode, weighted):
    return BAD_ALWAYS + (BAD_Y if mode == "y" else BAD_NEXT) + (BAD_WEIGHT if weighted else ())


def bad_rows_of(B, shift=0, mode="double", weighted=True):
    """From the generator alone: how many samples of make_case(rng, B, A, shift) are bad."""
    bad = bad_sorts(mode, weighted)
    return sum(SORTS[(i + shift) % len(SORTS)] in bad for i in range(B))


def rule_of(c, mode="double", weighted=True, delta=DELTA, scale=1.0):
    kw = dict(y=c["y"]) if mode == "y" else dict(q_next=c["q_next"], ret=c["ret"], discount=c["discount"], q_select=c["q_select"] if mode == "double" else None)
    return td_rule(c["q"], c["action"], weight=c["weight"] if weighted else None, delta=delta, scale=scale, **kw)


def test_the_generated_inputs_contain_every_sort_in_its_branch_and_the_order_of_the_sums_shows():
    for A, c in helpers.cases_per_action(make_case, ACTIONS, len(SORTS) * 48):
        sort = c["sort"]
        B = len(sort)
        n = B // len(SORTS)
        assert set(sort) == set(SORTS)
        rows = np.arange(B)
        for mode in MODES:
            for weighted in (False, True):
                out, sq = rule_of(c, mode, weighted), rule_of(c, mode, weighted, delta=0.0)
                want = bad_sorts(mode, weighted)
                assert out["bad_rows"] == sq["bad_rows"] == bad_rows_of(B, 0, mode, weighted) == n * len(want)
                assert set(sort[out["bad"]]) == set(want), (mode, weighted, set(sort[out["bad"]]) ^ set(want))
                for kind, k in PLACED.items():                       # below, at and above delta, both signs; exactly at it: not linear
                    for sign, s in (("pos", 1.0), ("neg", -1.0)):
                        at = sort == "%s_%s" % (kind, sign)
                        assert at.sum() >= 3 and (out["td"][at] == s * k * DELTA).all() and out["lin"][at].all() == (kind == "above")
                        assert out["lin"][at].any() == (kind == "above")
                assert not out["td"][sort == "td_zero"].any() and not out["GQ"][sort == "td_zero"].any() and not sq["lin"].any()
                assert out["stats"][5] == out["lin"].sum() / B > 0 and sq["stats"][5] == 0
                good = ~out["bad"]
                for k in ("q_untaken", "next_unchosen", "sel_nan_first", "sel_nan_last", "tie", "weight_zero", "big", "done"):
                    assert good[sort == k].all(), (mode, k)          # what these hold does not show
                assert np.isfinite(out["u"]).all() and np.isfinite(out["stats"]).all()
                big = np.abs(out["td"][good])
                assert (big > 1e3).any() and (big < 1.0).any()
                if weighted:
                    assert not out["total"][sort == "weight_zero"].any() and out["L"][sort == "weight_zero"].all()
        dbl, nxt = rule_of(c, "double"), rule_of(c, "next")
        tie = sort == "tie"                                          # the lowest index of the tied pair, whose q_next is 3 less than the other's
        sel = c["q_select"][tie]
        assert ((sel == sel.max(axis=1, keepdims=True)).sum(axis=1) == 2).all()
        assert (dbl["a_star"][tie] == (sel == sel.max(axis=1, keepdims=True)).argmax(axis=1)).all()
        # a NaN in q_select: at the last place it never wins; at the first place it is the starting value and no compare against it
        # succeeds, so the rule's a_star stays 0 (the stated loop, as snac_c51_project's)
        last, first = sort == "sel_nan_last", sort == "sel_nan_first"
        assert np.isnan(c["q_select"][last, A - 1]).all() and (dbl["a_star"][last] < A - 1).all()
        assert (dbl["a_star"][last] == np.nan_to_num(c["q_select"][last], nan=-np.inf).argmax(axis=1)).all()
        assert np.isnan(c["q_select"][first, 0]).all() and (dbl["a_star"][first] == 0).all()
        for out in (dbl, nxt):                                       # the unchosen place of q_next holds a NaN or -inf, the untaken of q anything
            un = sort == "next_unchosen"
            assert (~np.isfinite(c["q_next"][un])).sum() == un.sum() and np.isfinite(c["q_next"][un, out["a_star"][un]]).all()
            bq = sort == "qn_bad"
            assert (~np.isfinite(c["q_next"][bq, out["a_star"][bq]])).all()
        ut = sort == "q_untaken"
        assert (~np.isfinite(c["q"][ut])).sum() == ut.sum() and np.isfinite(c["q"][rows, np.clip(c["action"], 0, A - 1)][ut]).all()
        assert {int(x) for x in c["action"][sort == "action_bad"]} == {-1, A, 1 << 32, -(1 << 63)}
        for k, where in (("q", sort == "qa_bad"), ("ret", sort == "ret_bad"), ("discount", sort == "discount_bad"), ("y", sort == "y_bad"),
                         ("weight", sort == "weight_bad")):
            v = c[k][where]
            assert np.isnan(v).any() and (v == np.inf).any() and (v == -np.inf).any(), k
        assert (c["weight"][sort == "weight_bad"] == -0.5).any() and (c["discount"][sort == "discount_neg"] < 0).all()
    # the stated tree against a plain sum in index order: at B = 4097 they differ in at least one bit, so the GPU test can tell them apart
    B = 4097
    for A in ACTIONS:
        for mode in MODES:
            out = rule_of(make_case(np.random.default_rng(100 * A + B + B % len(SORTS)), B, A, B % len(SORTS)), mode)
            plain = np.float64(0.0)
            for t in out["u"][:, 0]:
                plain = plain + t
            tree = tree_sums(out["u"])[1][0]
            assert np.float64(plain).tobytes() != np.float64(tree).tobytes(), (A, mode, plain, tree)
            assert abs(plain - tree) <= 1e-9 * np.abs(out["u"][:, 0]).sum()                      # the same sum, in another order


# ---- against float64 torch and autograd --------------------------------------------------------------------------------------------------
ROUND = 2.0 ** -48                                                   # a few dozen float64 roundings, each 2^-53 relative


def _torch_reference(c, mode, weighted, delta, scale, rows):
    """(L, total, d (scale * total) / dq) of `rows` in float64 torch: gather, mse_loss / huber_loss and autograd.  The choice of the next
    action is numpy's first largest entry of the row with its NaNs taken out (index 0 where the row starts with one, as the rule's loop)."""
    import torch
    import torch.nn.functional as F

    t = lambda a: torch.tensor(np.asarray(a, np.float64)[rows], dtype=torch.float64)  # noqa: E731
    q = torch.tensor(np.nan_to_num(c["q"].astype(np.float64)[rows], nan=0.0, posinf=0.0, neginf=0.0), dtype=torch.float64, requires_grad=True)
    qa = q.gather(1, torch.tensor(c["action"][rows])[:, None])[:, 0]
    if mode == "y":
        target = t(c["y"])
    else:
        s = (c["q_select"] if mode == "double" else c["q_next"])[rows]
        a_star = np.where(np.isnan(s[:, 0]), 0, np.nan_to_num(s, nan=-np.inf).argmax(axis=1))
        qn = c["q_next"].astype(np.float64)[rows][np.arange(len(a_star)), a_star]
        target = t(c["ret"]) + t(c["discount"]) * torch.tensor(qn)
    L = F.mse_loss(qa, target, reduction="none") if delta == 0 else F.huber_loss(qa, target, reduction="none", delta=delta)
    total = t(c["weight"]) * L if weighted else L
    (scale * total).sum().backward()
    return L.detach().numpy(), total.detach().numpy(), q.grad.numpy()


def test_loss_and_gradient_stay_within_the_derived_bound_of_float64_torch_and_autograd():
    """The bound is derived, not fitted to what is seen (which is printed).  There is no EXP or LOG here: every difference is a float64
    rounding, 2^-53 relative each.  With M = |qa| + |ret| + |discount qn| (mode Y: |qa| + |y|), the target carries at most two roundings
    and td = qa - yv a third: |err td| <= 3 * 2^-53 M.  From it
        L     = td^2, 0.5 td^2 or delta (|td| - 0.5 delta):   |err L| <= (2 |td| + delta) |err td| + 3 * 2^-53 L
        total = w L:                                           w times that, and one rounding more
        g     = 2 td, td or +-delta (continuous in td):        |err g| <= 2 |err td|;  grad = scale (w g): two roundings more
      loss, total <= ROUND ((|td| + delta) M + L) (w)          grad_q <= |scale| w ROUND (M + |g|)
    with ROUND = 2^-48 = 32 * 2^-53, which covers the reference's own roundings as well.  Huber's loss and gradient are continuous at
    |td| == delta, so no sample needs to be left out there: none is (0 % of the rows, asserted as the bound of 1 % asks)."""
    seen = np.zeros(3)
    rows_seen = 0
    tiny = 1e-300                                                    # 0 / 0 where a sample's numbers are all zero
    for A, c in helpers.cases_per_action(make_case, ACTIONS, len(SORTS) * 240):
        for mode in MODES:
            for weighted in (False, True):
                for delta in DELTAS:
                    for scale in (1.0, 1.0 / 4096.0):
                        out = rule_of(c, mode, weighted, delta, scale)
                        rows = ~out["bad"]                           # every good sample is compared
                        assert (~rows & ~out["bad"]).sum() < 0.01 * len(rows) and rows.sum() >= len(rows) // 2
                        L, total, GQ = _torch_reference(c, mode, weighted, delta, scale, rows)
                        qa = c["q"][np.arange(len(rows)), np.clip(c["action"], 0, A - 1)].astype(np.float64)[rows]
                        yv, r = out["yv"][rows], c["ret"].astype(np.float64)[rows]
                        M = np.abs(qa) + (np.abs(yv) if mode == "y" else np.abs(r) + np.abs(yv - r))
                        td, w, g = np.abs(out["td"][rows]), out["w"][rows], np.abs(out["g"][rows])
                        b_l = ROUND * ((td + delta) * M + out["L"][rows]) + tiny
                        b_g = abs(scale) * w * ROUND * (M + g) + tiny
                        ratios = (np.abs(out["L"][rows] - L) / b_l, np.abs(out["total"][rows] - total) / (b_l * np.maximum(w, tiny)),
                                  (np.abs(out["GQ"][rows] - GQ) / b_g[:, None]).max(axis=1))
                        seen = np.maximum(seen, [x.max() for x in ratios])
                        rows_seen += int(rows.sum())
                        for name, x in zip(("loss", "total", "grad_q"), ratios):
                            assert x.max() <= 1.0, (A, mode, weighted, delta, scale, name, x.max(), c["sort"][rows][x.argmax()])
    print("largest error / bound: loss %.3g, weighted loss %.3g, grad_q %.3g over %d rows" % (seen[0], seen[1], seen[2], rows_seen))


def test_bad_samples_give_zeros_add_nothing_and_are_counted():
    for A, c in helpers.cases_per_action(make_case, ACTIONS, len(SORTS) * 48):
        B = len(c["sort"])
        for mode in MODES:
            for weighted in (False, True):
                out = rule_of(c, mode, weighted, scale=1.0 / B)
                bad = out["bad"]
                assert out["bad_rows"] == bad.sum() == bad_rows_of(B, 0, mode, weighted) > 0
                for k in ("loss", "priority", "y_out", "grad_q"):
                    assert out[k].dtype == np.float32 and not out[k][bad].view(np.uint32).any() and np.isfinite(out[k]).all(), k
                assert not out["u"][bad].any() and out["stats"][6] == B - out["bad_rows"]
                assert (np.count_nonzero(out["grad_q"], axis=1) <= 1).all()                     # the taken action's place alone
                assert out["mean_loss"].dtype == np.float32 and out["mean_loss"][0] == np.float32(out["stats"][0])
                assert abs(out["stats"][0] - out["total"][~bad].sum() / B) <= 1e-12 * np.abs(out["total"][~bad]).sum() / B
                assert np.array_equal(out["priority"][~bad], np.abs(out["td"][~bad]).astype(np.float32))
                if not weighted:
                    assert out["stats"][0] == out["stats"][1] and out["stats"][7] == out["stats"][6] / B


# ---- the C entry point -------------------------------------------------------------------------------------------------------------------
def _td(L, B=4, A=5, q=PH, action=PH, y=None, q_next=PH, q_select=PH, ret=PH, discount=PH, weight=PH, delta=1.0, scale=1.0, loss=PH, prio=PH,
        y_out=PH, gq=PH, stats=PH, mean=PH, partials=PH, bad=PH):
    return L.snac_td_loss(B, A, q, action, y, q_next, q_select, ret, discount, weight, delta, scale, loss, prio, y_out, gq, stats, mean, partials, bad,
                          None)


MODE_Y = dict(y=PH, q_next=None, q_select=None, ret=None, discount=None)


def test_the_library_exports_the_entry_point():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    assert "snac_td_loss" in _lib.EXPORTS and len(L.snac_td_loss.argtypes) == 21 and _lib.Q_STATS == 8
    res, args = _lib.PROTOTYPES["snac_td_loss"]
    assert res == C.c_int and args[:2] == [C.c_int32, C.c_int32] and args[10:12] == [C.c_double] * 2
    assert all(t == C.c_void_p for t in args[2:10] + args[12:])


def test_td_loss_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _err(L, _td(L, q=None), -1, b"null q")
    _err(L, _td(L, action=None), -1, b"null action")
    for B in (0, -1, -(1 << 31)):
        _err(L, _td(L, B=B), -1, b"B must be >= 1")
    # the either-or of the target modes
    for k in ("q_next", "q_select", "ret", "discount"):
        _err(L, _td(L, **dict(MODE_Y, **{k: PH})), -1, b"one target")
    _err(L, _td(L, q_next=None, q_select=None, ret=None, discount=None), -1, b"a target is needed")
    _err(L, _td(L, q_next=None, ret=None, discount=None), -1, b"q_select belongs to")
    for k in ("q_next", "ret", "discount"):
        _err(L, _td(L, **{k: None}), -1, b"q_next, ret and discount are needed together")
    for delta in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        _err(L, _td(L, delta=delta), -1, b"delta must be finite and >= 0")
    for x in (float("nan"), float("inf"), float("-inf")):
        _err(L, _td(L, scale=x), -1, b"scale must be finite")
    _err(L, _td(L, partials=None), -1, b"partials are needed for stats")
    _err(L, _td(L, stats=None), -1, b"stats is needed")
    _err(L, _td(L, action=C.c_void_p((1 << 20) + 4)), -1, b"action must be 8-byte aligned")
    _err(L, _td(L, stats=C.c_void_p((1 << 20) + 4)), -1, b"stats and partials must be 8-byte aligned")
    _err(L, _td(L, partials=C.c_void_p((1 << 20) + 4)), -1, b"stats and partials must be 8-byte aligned")
    for A in (0, 1, 2, 4, 6, 7, 9, -3):
        _err(L, _td(L, A=A), -3, b"num_actions must be 3, 5 or 8")
    # no output: no launch, although no device exists to launch on -- but the checks come first
    none = dict(loss=None, prio=None, y_out=None, gq=None, stats=None, mean=None, bad=None)
    for A in ACTIONS:
        assert _td(L, A=A, **none) == 0 and _td(L, A=A, partials=None, **none) == 0
        assert _td(L, A=A, q_select=None, weight=None, delta=0.0, **none) == 0 and _td(L, A=A, **dict(MODE_Y, **none)) == 0
    _err(L, _td(L, B=0, **none), -1, b"B must be >= 1")
    _err(L, _td(L, A=4, **none), -3, b"num_actions must be")
    _err(L, _td(L, delta=-1.0, **none), -1, b"delta must be finite")
    _err(L, _td(L, y=PH, **none), -1, b"one target")


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------------
def test_td_loss_checks_its_arguments_before_it_touches_a_device():
    import torch
    from snac_amd import TDLoss

    ok = dict(num_actions=5, device="cuda:0")
    for bad in (dict(num_actions=4), dict(num_actions=True), dict(num_actions="5"), dict(num_actions=5.0), dict(device="cpu"), dict(device=None),
                dict(huber=0.0), dict(huber=-1.0), dict(huber=float("nan")), dict(huber=float("inf")), dict(huber="1"), dict(huber=True)):
        with pytest.raises(ValueError):
            TDLoss(**dict(ok, **bad))
    td = TDLoss(5, device="cuda:0")
    assert td.num_actions == 5 and td.device == torch.device("cuda:0") and td.env is None and td.stats is None and td.delta == 0.0
    assert TDLoss(3, huber=1, device="cuda:0").delta == 1.0 and TDLoss(8, 0.5, "cuda:0").delta == 0.5
    with pytest.raises(ValueError, match="no loss"):
        td.stats_dict()
    q, v, a = torch.zeros(4, 5), torch.zeros(4), torch.zeros(4, dtype=torch.int64)
    for kw in (dict(), dict(q_next=q), dict(q_next=q, ret=v), dict(ret=v, discount=v), dict(q_select=q), dict(weight=v)):
        with pytest.raises(ValueError, match="a target is needed"):
            td.loss(q, a, **kw)
    for kw in (dict(q_next=q), dict(ret=v), dict(discount=v), dict(q_select=q), dict(q_next=q, ret=v, discount=v)):
        with pytest.raises(ValueError, match="one target"):
            td.loss(q, a, v, **kw)
    with pytest.raises(ValueError, match=r"q must have shape \(B, 5\), got \(4, 3\)"):
        td.loss(torch.zeros(4, 3), a, v)
    with pytest.raises(ValueError, match="q must have shape"):
        td.loss(torch.zeros(0, 5), a[:0], v[:0])
    with pytest.raises(ValueError, match="q must be a contiguous torch.float32 tensor"):
        td.loss(q.double(), a, v)
    with pytest.raises(ValueError, match="q must be a contiguous torch.float32 tensor"):
        td.loss(torch.zeros(4, 10)[:, ::2], a, v)
    with pytest.raises(ValueError, match="q must be on cuda:0"):
        td.loss(q, a, v)
    with pytest.raises(ValueError, match="q must be on cuda:0"):
        td.loss(q.requires_grad_(), a, q_next=q, ret=v, discount=v)


# ---- the kernel's code on the host -------------------------------------------------------------------------------------------------------
OUTPUTS = ("loss", "priority", "y_out", "grad_q", "stats", "mean_loss", "partials")
HOST_SRC = os.path.join(helpers.TESTS, "native", "td_host.cpp")
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", _lib.CSRC, HOST_SRC]


def test_the_kernels_code_compiled_for_the_host_equals_the_rule_byte_for_byte(tmp_path):
    fn = load_shared(tmp_path, "td_host", ["-O2", "-fPIC", "-shared"] + HOST_FLAGS, timeout=600).td_host
    fn.restype, fn.argtypes = C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 8 + [C.c_double] * 2 + [C.c_void_p] * 7
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def ins(c, mode, weighted):
        y = mode == "y"
        return [vp(c["q"]), vp(c["action"]), vp(c["y"]) if y else None, None if y else vp(c["q_next"]), vp(c["q_select"]) if mode == "double" else None,
                None if y else vp(c["ret"]), None if y else vp(c["discount"]), vp(c["weight"]) if weighted else None]
    for A in ACTIONS:
        for B in (1, 64, 65, 4097, 8193):
            shifts = range(len(SORTS)) if B == 1 else (B % len(SORTS),)
            for shift in shifts:
                c = make_case(np.random.default_rng(100 * A + B + shift), B, A, shift)
                for mode in MODES:
                    for weighted, delta in ((True, DELTA), (False, 0.0)) if B > 65 else ((True, DELTA), (False, 0.0), (True, 0.0), (False, DELTA)):
                        want = rule_of(c, mode, weighted, delta, 1.0 / B)
                        W = (B + 63) // 64
                        got = dict(loss=np.full(B, 7, np.float32), priority=np.full(B, 7, np.float32), y_out=np.full(B, 7, np.float32),
                                   grad_q=np.full((B, A), 7, np.float32), stats=np.full(8, 7, np.float64), mean_loss=np.full(1, 7, np.float32),
                                   partials=np.full((W, 8), 7, np.float64))
                        bad = fn(B, A, *ins(c, mode, weighted), delta, 1.0 / B, *[vp(got[k]) for k in OUTPUTS])
                        assert bad == want["bad_rows"] == bad_rows_of(B, shift, mode, weighted), (A, B, shift, mode, weighted, bad, want["bad_rows"])
                        for k in OUTPUTS:
                            _same(got[k], want[k], (A, B, shift, mode, weighted, delta, k))
    # no statistics asked for: stats, mean_loss and partials are not touched
    prio = np.full(B, 7, np.float32)
    assert fn(B, A, *ins(c, "next", False), 0.0, 1.0, None, vp(prio), None, None, None, None, None) == bad_rows_of(B, shift, "next", False)
    _same(prio, rule_of(c, "next", False, 0.0)["priority"], "the priorities alone")


def test_the_kernels_code_runs_clean_under_the_host_sanitizers_with_actions_out_of_range(tmp_path):
    """A stand-alone program (td_host.cpp with its main), not code loaded into python."""
    r = run_sanitized(tmp_path, "td_host_main", ["-DTD_HOST_MAIN"] + HOST_FLAGS, probe_timeout=300, build_timeout=600, run_timeout=300)
    assert r.stdout.count("bad ") == 54 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ==== snac_c51_loss ======================================================================================================================
C51_STATS = ("total", "ce", "H", "M", "zero4", "zero5", "good", "w")
C51_INPUTS = ("logits", "action", "m", "weight")


def tree64(v):
    """TREE of the header over rows of 64 terms: [B, 64] -> [B]."""
    for s in (32, 16, 8, 4, 2, 1):
        v = v[:, :s] + v[:, s:2 * s]
    return v[:, 0]


def c51_loss_rule(logits, action, m, weight=None, scale=1.0):
    """-> dict(loss float32 [B], grad float32 [B, A, K], stats, mean_loss, partials, bad_rows; and before the rounding to float32: ce,
    total, G [B, K] (the taken action's row of the gradient); u [B, 8]; S, H, M, p, lp, e, bad)."""
    logits = np.asarray(logits, np.float32)
    B, A, K = logits.shape
    action, m = np.asarray(action, np.int64), np.asarray(m, np.float32)
    rows = np.arange(B)
    bad = (action < 0) | (action >= A)
    act = np.where(bad, 0, action)
    l = np.where(bad[:, None], np.float32(0.0), logits[rows, act])   # nothing is read through an action out of range
    bad = bad | ~np.isfinite(l).all(axis=1) | ~np.isfinite(m).all(axis=1)
    if weight is not None:
        w32 = np.asarray(weight, np.float32)
        bad = bad | ~np.isfinite(w32) | (w32 < 0)
    good = ~bad
    l = np.where(good[:, None], l, np.float32(0.0))                  # (bad samples are zeroed below)
    mj = np.where(good[:, None], m, np.float32(0.0)).astype(np.float64)
    w = np.where(good, w32, np.float32(1.0)).astype(np.float64) if weight is not None else np.ones(B)
    pad = lambda v: np.concatenate([v, np.zeros((B, 64 - K))], axis=1)  # noqa: E731
    mx = l.max(axis=1)
    x = l.astype(np.float64) - mx.astype(np.float64)[:, None]
    e = spec_exp(x)
    S = tree64(pad(e))
    T = tree64(pad(np.where(e == 0.0, 0.0, e * x)))
    Lg = spec_log(S)
    lp = x - Lg[:, None]
    p = e / S[:, None]
    ce = -tree64(pad(mj * lp))
    M = tree64(pad(mj))
    H = Lg - T / S
    total = w * ce
    G = np.float64(scale) * (w[:, None] * (M[:, None] * p - mj))
    u = np.stack([total, ce, H, M, np.zeros(B), np.zeros(B), np.ones(B), w], axis=1)
    u = np.where(good[:, None], u, 0.0)
    loss = np.where(good, ce.astype(np.float32), np.float32(0.0))
    grad = np.zeros((B, A, K), np.float32)
    grad[rows, act] = np.where(good[:, None], G.astype(np.float32), np.float32(0.0))
    partials, sums = tree_sums(u)
    stats = np.array([s if C51_STATS[k] == "good" else s / np.float64(B) for k, s in enumerate(sums)], np.float64)
    return dict(loss=loss, grad=grad, stats=stats, mean_loss=np.array([stats[0]], np.float32), partials=partials, bad_rows=int(bad.sum()), bad=bad,
                ce=ce, total=total, G=G, u=u, S=S, H=H, M=M, p=p, lp=lp, e=e, w=w, mj=mj)


C51_SORTS = ("normal", "peaked", "flat", "equal", "far_below", "m_first", "m_last", "m_mass", "logit_bad_first", "logit_bad_last", "m_bad_first",
             "m_bad_last", "action_bad", "weight_bad", "weight_zero", "other_row")
C51_BAD = ("logit_bad_first", "logit_bad_last", "m_bad_first", "m_bad_last", "action_bad")


def make_c51_case(rng, B, A, K, shift=0):
    """dict(logits float32 [B, A, K], action int64 [B], m float32 [B, K], weight float32 [B], sort)."""
    logits = (1.5 * rng.normal(size=(B, A, K))).astype(np.float32)
    t = rng.normal(size=(B, K))
    m = (np.exp(t) / np.exp(t).sum(axis=1, keepdims=True)).astype(np.float32)
    action = rng.integers(0, A, size=B).astype(np.int64)
    weight = (0.1 + 0.9 * rng.random(size=B)).astype(np.float32)
    sorts = [C51_SORTS[(i + shift) % len(C51_SORTS)] for i in range(B)]
    for i, sort in enumerate(sorts):
        turn = i // len(C51_SORTS)
        a = int(action[i])
        if sort == "peaked":
            logits[i, a, rng.integers(K)] += np.float32(20.0)
        elif sort == "flat":
            logits[i, a] *= np.float32(0.01)
        elif sort == "equal":
            logits[i, a] = logits[i, a, 0]
        elif sort == "far_below":                                    # finite, and more than 45 below the largest: no weight
            top = int(logits[i, a].argmax())
            j = (top + 1 + int(rng.integers(K - 1))) % K
            logits[i, a, j] = logits[i, a, top] - np.float32((45.5, 60.0, 300.0)[turn % 3])
        elif sort in ("m_first", "m_last"):                          # one-hot at the first and at the last atom
            m[i] = 0.0
            m[i, 0 if sort == "m_first" else K - 1] = 1.0
        elif sort == "m_mass":                                       # a mass that is not 1, and no mass at all
            m[i] *= np.float32((0.5, 2.0, 0.0)[turn % 3])
        elif sort in ("logit_bad_first", "logit_bad_last"):
            logits[i, a, 0 if sort == "logit_bad_first" else K - 1] = NOT_FINITE[turn % 3]
        elif sort in ("m_bad_first", "m_bad_last"):
            m[i, 0 if sort == "m_bad_first" else K - 1] = NOT_FINITE[turn % 3]
        elif sort == "action_bad":
            action[i] = (-1, A, 1 << 32, -(1 << 63))[turn % 4]
        elif sort == "weight_bad":
            weight[i] = (np.nan, np.inf, -np.inf, -0.5)[turn % 4]
        elif sort == "weight_zero":
            weight[i] = 0.0
        elif sort == "other_row":                                    # the rows of the actions not taken are never read
            logits[i, (a + 1 + int(rng.integers(A - 1))) % A] = NOT_FINITE[turn % 3]
    return dict(logits=logits, action=action, m=m, weight=weight, sort=np.array(sorts))


def c51_bad_rows_of(B, shift=0, weighted=True):
    bad = C51_BAD + (("weight_bad",) if weighted else ())
    return sum(C51_SORTS[(i + shift) % len(C51_SORTS)] in bad for i in range(B))


def c51_rule_of(c, weighted=True, scale=1.0):
    return c51_loss_rule(c["logits"], c["action"], c["m"], c["weight"] if weighted else None, scale)


def _c51_cases(rows=len(C51_SORTS) * 24):
    for A, K in ((3, 51), (5, 51), (8, 51), (5, 2), (5, 33), (5, 64)):
        yield A, K, make_c51_case(np.random.default_rng(10 * A + K), rows, A, K)


def test_the_generated_c51_inputs_contain_every_sort_in_its_branch_and_the_order_of_the_sums_shows():
    for A, K, c in _c51_cases():
        sort = c["sort"]
        B = len(sort)
        n = B // len(C51_SORTS)
        assert set(sort) == set(C51_SORTS)
        for weighted in (False, True):
            out = c51_rule_of(c, weighted)
            want = C51_BAD + (("weight_bad",) if weighted else ())
            assert out["bad_rows"] == c51_bad_rows_of(B, 0, weighted) == n * len(want) and set(sort[out["bad"]]) == set(want)
            good = ~out["bad"]
            assert np.isfinite(out["u"]).all() and (out["S"][good] >= 1.0).all() and (out["S"][good] <= K).all()
            assert (out["S"][sort == "equal"] == K).all() and np.allclose(out["H"][sort == "equal"], np.log(K), rtol=0, atol=1e-11)
            if K > 2:
                assert (out["H"][sort == "peaked"] < 0.5 * out["H"][sort == "flat"]).all()
            far = sort == "far_below"
            assert ((out["e"][far] == 0.0).sum(axis=1) >= 1).all() and np.isfinite(out["lp"][far]).all()
            assert not out["G"][far][out["e"][far] == 0.0][out["mj"][far][out["e"][far] == 0.0] == 0.0].any()
            assert (out["M"][sort == "m_first"] == 1.0).all() and (out["M"][sort == "m_last"] == 1.0).all()
            assert np.array_equal(out["ce"][sort == "m_first"], -out["lp"][sort == "m_first", 0])
            assert np.array_equal(out["ce"][sort == "m_last"], -out["lp"][sort == "m_last", K - 1])
            mass = out["M"][sort == "m_mass"]
            assert (mass == 0.0).any() and (np.abs(mass - 0.5) < 1e-6).any() and (np.abs(mass - 2.0) < 1e-6).any()
            assert good[sort == "other_row"].all() and (~np.isfinite(c["logits"][sort == "other_row"])).any(axis=(1, 2)).all()
            if weighted:
                assert not out["total"][sort == "weight_zero"].any() and out["ce"][sort == "weight_zero"].all()
        for k, first, last in (("logits", "logit_bad_first", "logit_bad_last"), ("m", "m_bad_first", "m_bad_last")):
            v = c[k][np.arange(B), np.clip(c["action"], 0, A - 1)] if k == "logits" else c[k]
            assert (~np.isfinite(v[sort == first, 0])).all() and (~np.isfinite(v[sort == last, K - 1])).all()
        assert {int(x) for x in c["action"][sort == "action_bad"]} == {-1, A, 1 << 32, -(1 << 63)}
    B = 4097
    for A in ACTIONS:
        out = c51_rule_of(make_c51_case(np.random.default_rng(100 * A + B), B, A, 51, B % len(C51_SORTS)))
        plain = np.float64(0.0)
        for t in out["u"][:, 0]:
            plain = plain + t
        tree = tree_sums(out["u"])[1][0]
        assert np.float64(plain).tobytes() != np.float64(tree).tobytes(), (A, plain, tree)
        assert abs(plain - tree) <= 1e-9 * np.abs(out["u"][:, 0]).sum()


def test_log_stays_within_1e_12_of_the_long_double_logarithm_over_1_to_64():
    rng = np.random.default_rng(7)
    s = np.concatenate([np.linspace(1.0, 64.0, 1 << 20), 1.0 + 63.0 * rng.random(1 << 20), 2.0 ** np.arange(7), np.nextafter(2.0 ** np.arange(1, 7), 0)])
    err = np.abs(spec_log(s).astype(np.longdouble) - np.log(s.astype(np.longdouble)))
    print("LOG over [1, 64]: largest error %.3g" % float(err.max()))
    assert np.finfo(np.longdouble).eps < 1e-18 and float(err.max()) <= 1e-12


EPS_EXP, DELTA_LOG = 2e-12, 1e-12


def test_c51_loss_and_gradient_stay_within_the_derived_bound_of_float64_log_softmax_and_autograd():
    """Derived as PPO's bound, from the header's 1e-12 on EXP and LOG (LOG over [1, 64]: the test above): EXP is within eps = 2e-12
    relative, so S is (a sum of positive terms), and Lg = LOG(S) and every lp_j = x_j - Lg are within err_l = delta + 2 eps absolute;
    p_j = e_j / S is within 2 eps relative.  With Mabs = sum |m_j|:
        ce   = -sum m_j lp_j:            <= Mabs err_l + ROUND (sum |m_j lp_j| + 1)
        grad = scale w (M p_j - m_j):    <= |scale| w (2 eps |M| p_j + ROUND (Mabs p_j + |m_j|))
    with ROUND = 2^-48 for the few dozen roundings (the tree's and the reference's sums of up to 64 terms among them)."""
    import torch

    seen = np.zeros(2)
    rows_seen = 0
    err_l = DELTA_LOG + 2.0 * EPS_EXP
    for A, K, c in _c51_cases(len(C51_SORTS) * 64):
        for weighted in (False, True):
            for scale in (1.0, 1.0 / 4096.0):
                out = c51_rule_of(c, weighted, scale)
                rows = ~out["bad"]
                assert rows.sum() >= len(rows) // 2
                l = torch.tensor(np.nan_to_num(c["logits"].astype(np.float64)[rows], nan=0.0, posinf=0.0, neginf=0.0), requires_grad=True)
                idx = torch.arange(int(rows.sum()))
                logp = torch.log_softmax(l, dim=2)[idx, torch.tensor(c["action"][rows])]
                ce = -(torch.tensor(c["m"].astype(np.float64)[rows]) * logp).sum(dim=1)
                total = torch.tensor(out["w"][rows]) * ce
                (scale * total).sum().backward()
                G = l.grad.numpy()[np.arange(int(rows.sum())), c["action"][rows]]
                assert np.count_nonzero(l.grad.numpy()) == np.count_nonzero(G)                   # the other rows: exactly zero
                mabs = np.abs(out["mj"][rows]).sum(axis=1)
                b_ce = mabs * err_l + ROUND * (np.abs(out["mj"][rows] * out["lp"][rows]).sum(axis=1) + 1.0)
                w, p = out["w"][rows], out["p"][rows]
                b_g = abs(scale) * w[:, None] * (2.0 * EPS_EXP * np.abs(out["M"][rows])[:, None] * p + ROUND * (mabs[:, None] * p + np.abs(out["mj"][rows]))) + 1e-300
                ratios = (np.abs(out["ce"][rows] - ce.detach().numpy()) / b_ce, (np.abs(out["G"][rows] - G) / b_g).max(axis=1))
                seen = np.maximum(seen, [x.max() for x in ratios])
                rows_seen += int(rows.sum())
                for name, x in zip(("ce", "grad"), ratios):
                    assert x.max() <= 1.0, (A, K, weighted, scale, name, x.max(), c["sort"][rows][x.argmax()])
    print("largest error / bound: cross-entropy %.3g, grad %.3g over %d rows" % (seen[0], seen[1], rows_seen))


def test_bad_c51_samples_give_zeros_add_nothing_and_are_counted():
    for A, K, c in _c51_cases():
        B = len(c["sort"])
        for weighted in (False, True):
            out = c51_rule_of(c, weighted, 1.0 / B)
            bad = out["bad"]
            assert out["bad_rows"] == bad.sum() == c51_bad_rows_of(B, 0, weighted) > 0
            for k in ("loss", "grad"):
                assert out[k].dtype == np.float32 and not out[k][bad].view(np.uint32).any() and np.isfinite(out[k]).all(), k
            assert not out["u"][bad].any() and out["stats"][6] == B - out["bad_rows"] and not out["stats"][4:6].any()
            taken = np.zeros((B, A), bool)
            taken[np.arange(B), np.clip(c["action"], 0, A - 1)] = True
            assert not out["grad"][~taken].view(np.uint32).any()     # the rows of the other actions: exactly +0.0
            assert out["mean_loss"][0] == np.float32(out["stats"][0])
            # the gradient of a row sums to zero where the target has mass 1, up to the roundings of 64 terms
            unit = ~bad & (np.abs(out["M"] - 1.0) < 1e-6)
            assert unit.sum() > B // 4 and (np.abs(out["G"][unit].sum(axis=1)) <= 1e-6 / B).all()


def _c51(L, B=4, A=5, K=51, logits=PH, action=PH, m=PH, weight=PH, scale=1.0, loss=PH, grad=PH, stats=PH, mean=PH, partials=PH, bad=PH):
    return L.snac_c51_loss(B, A, K, logits, action, m, weight, scale, loss, grad, stats, mean, partials, bad, None)


def test_the_library_exports_c51_loss():
    L = _lib.lib()
    assert "snac_c51_loss" in _lib.EXPORTS and len(L.snac_c51_loss.argtypes) == 15 and L.snac_version() == 12
    res, args = _lib.PROTOTYPES["snac_c51_loss"]
    assert res == C.c_int and args[:3] == [C.c_int32] * 3 and args[7] == C.c_double and all(t == C.c_void_p for t in args[3:7] + args[8:])


def test_c51_loss_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    for k in ("logits", "action", "m"):
        _err(L, _c51(L, **{k: None}), -1, b"null logits/action/m")
    for B in (0, -1, -(1 << 31)):
        _err(L, _c51(L, B=B), -1, b"B must be >= 1")
    for K in (1, 0, -1, 65, 1 << 20):
        _err(L, _c51(L, K=K), -1, b"atoms must be in [2, 64]")
    for x in (float("nan"), float("inf"), float("-inf")):
        _err(L, _c51(L, scale=x), -1, b"scale must be finite")
    _err(L, _c51(L, partials=None), -1, b"partials are needed for stats")
    _err(L, _c51(L, stats=None), -1, b"stats is needed")
    _err(L, _c51(L, action=C.c_void_p((1 << 20) + 4)), -1, b"action must be 8-byte aligned")
    _err(L, _c51(L, stats=C.c_void_p((1 << 20) + 4)), -1, b"stats and partials must be 8-byte aligned")
    _err(L, _c51(L, partials=C.c_void_p((1 << 20) + 4)), -1, b"stats and partials must be 8-byte aligned")
    for A in (0, 1, 2, 4, 6, 7, 9, -3):
        _err(L, _c51(L, A=A), -3, b"num_actions must be 3, 5 or 8")
    none = dict(loss=None, grad=None, stats=None, mean=None, bad=None)
    for A in ACTIONS:
        for K in (2, 51, 64):
            assert _c51(L, A=A, K=K, **none) == 0 and _c51(L, A=A, K=K, partials=None, weight=None, **none) == 0
    _err(L, _c51(L, K=65, **none), -1, b"atoms must be")
    _err(L, _c51(L, A=4, **none), -3, b"num_actions must be")


def test_categorical_support_loss_checks_its_arguments_before_it_touches_a_device():
    import torch
    from snac_amd import CategoricalSupport

    sup = CategoricalSupport(5, atoms=51, device="cuda:0")
    assert sup.stats is None
    with pytest.raises(ValueError, match="no loss"):
        sup.stats_dict()
    l, a, m, w = torch.zeros(4, 5, 51), torch.zeros(4, dtype=torch.int64), torch.zeros(4, 51), torch.zeros(4)
    with pytest.raises(ValueError, match=r"logits must have shape \(B, 5, 51\), got \(4, 5, 50\)"):
        sup.loss(torch.zeros(4, 5, 50), a, m)
    with pytest.raises(ValueError, match="logits must be a contiguous torch.float32 tensor"):
        sup.loss(l.double(), a, m, w)
    with pytest.raises(ValueError, match="logits must be a contiguous torch.float32 tensor"):
        sup.loss(torch.zeros(4, 5, 102)[:, :, ::2], a, m)
    with pytest.raises(ValueError, match="logits must be on cuda:0"):
        sup.loss(l, a, m, w, want_per_sample=True)
