"""Host: the rule of include/snac_hip.h, "PPO loss (the reference's script/PPO)", restated in numpy (ppo_rule), independently of the
kernels (tests/test_gpu_ppo_loss.py compares them with it byte for byte): its entropy against soft_rule's bytes, its loss and gradients
before the rounding to float32 against a float64 torch composition and torch autograd, bad samples, both stages of the batch reduction,
and the inputs the GPU test runs on (make_case: that they contain every sort, and that the stated order of the sums can be told from a
plain index-order sum, is asserted here).  Then snac_ppo_loss is exported and checks every argument before any HIP call -- each failing
call below fails its checks first, so the placeholder pointers are never dereferenced -- and PPOLoss checks its arguments before it
touches a device.  Last, the per-sample function the kernel runs (snac_amd/csrc/ppo_rule.h) and a C++ restatement of the reduction are
compiled for the host with the system compiler and compared with ppo_rule byte for byte, and the same source runs once as a program
under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os

import numpy as np
import pytest

from cabi_checks import PH, _err_code as _err
import helpers
from hostcode import load_shared, run_sanitized
from snac_amd import _lib
from specmath import _same, spec_exp, spec_log, tree_sums
from test_sac_host import soft_rule

ACTIONS = (3, 5, 8)
CLIP, VF_COEF, ENT_COEF = 0.2, 0.5, 0.01
CLIP_VFS = (-1.0, 0.2)                                               # off, on
LOGRATIO_MAX = 20.0
STATS = ("total", "Lpi", "Lv", "H", "kl", "clipped", "good", "clamped")


# ---- the rule, in numpy: every ufunc call below is one float64 operation, rounded on its own --------------------------------------------
def ppo_rule(logits, action, logp_old, adv, value, value_old, ret, clip=CLIP, clip_vf=-1.0, vf_coef=VF_COEF, ent_coef=ENT_COEF, scale=1.0):
    """-> dict(loss float32 [B], grad_logits float32 [B, A], grad_value float32 [B], stats float64 [8], mean_loss float32 [1], partials
    float64 [W, 8], bad_rows int; and before the rounding to float32: total, GL, GV; u [B, 8] the contributions; r, d, H, Lpi, Lv [B];
    second, clamped, vsecond, vclamped, live, bad).  value_old is read only when clip_vf >= 0."""
    l = np.asarray(logits, np.float32)
    B, A = l.shape
    action = np.asarray(action, np.int64)
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    logp_old, adv, value, ret = f32(logp_old), f32(adv), f32(value), f32(ret)
    clip_v = clip_vf >= 0
    m = l[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for a in range(1, A):
            m = np.where(l[:, a] > m, l[:, a], m)
        bad = np.isnan(l).any(axis=1) | (l == np.inf).any(axis=1) | (m == -np.inf)
    bad = bad | (action < 0) | (action >= A)
    bad = bad | ~np.isfinite(logp_old) | ~np.isfinite(adv) | ~np.isfinite(value) | ~np.isfinite(ret)
    if clip_v:
        value_old = f32(value_old)
        bad = bad | ~np.isfinite(value_old)
    l, m = l.copy(), m.copy()
    l[bad], m[bad] = 0.0, 0.0                                        # (bad samples are zeroed below)
    act = np.where(bad, 0, action)
    x = l.astype(np.float64) - m.astype(np.float64)[:, None]
    e = spec_exp(x)
    S, T = np.zeros(B), np.zeros(B)
    with np.errstate(invalid="ignore"):
        for a in range(A):
            S = S + e[:, a]
            T = T + np.where(e[:, a] == 0.0, 0.0, e[:, a] * x[:, a])
    L = spec_log(S)
    H = L - T / S
    live = e != 0.0
    rows = np.arange(B)
    bad = bad | (e[rows, act] == 0.0)                                # the taken action has no weight
    z = lambda a: np.where(bad, 0.0, np.asarray(a, np.float32).astype(np.float64))  # noqa: E731
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pi = e / S[:, None]
        lpa = x - L[:, None]
        lp = np.where(bad, 0.0, lpa[rows, act])
        d = lp - z(logp_old)
        clamped = np.abs(d) > LOGRATIO_MAX
        dc = np.where(d < -LOGRATIO_MAX, -LOGRATIO_MAX, np.where(d > LOGRATIO_MAX, LOGRATIO_MAX, d))
        r = np.where(dc <= 0.0, spec_exp(np.minimum(dc, 0.0)), 1.0 / spec_exp(-np.maximum(dc, 0.0)))
        lo, hi = 1.0 - np.float64(clip), 1.0 + np.float64(clip)
        rc = np.where(r < lo, lo, np.where(r > hi, hi, r))
        ad = z(adv)
        s1, s2 = r * ad, rc * ad
        second = s2 < s1
        Lpi = -np.where(second, s2, s1)
        g = np.where(~second & ~clamped, -(ad * r), 0.0)
        dv = z(value) - z(ret)
        if clip_v:
            cv = np.float64(clip_vf)
            u_ = z(value) - z(value_old)
            uc = np.where(u_ < -cv, -cv, np.where(u_ > cv, cv, u_))
            dc2 = (z(value_old) + uc) - z(ret)
            q1, q2 = dv * dv, dc2 * dc2
            vsecond, vclamped = q2 > q1, u_ != uc
            Lv = np.where(vsecond, 0.5 * q2, 0.5 * q1)
            gv = np.where(vsecond, np.where(vclamped, 0.0, dc2), dv)
        else:
            vsecond = vclamped = np.zeros(B, bool)
            Lv, gv = 0.5 * (dv * dv), dv
        kl = 0.5 * (dc * dc)
        clipped = np.abs(r - 1.0) > np.float64(clip)
        vf, ent, sc = np.float64(vf_coef), np.float64(ent_coef), np.float64(scale)
        total = (Lpi + vf * Lv) - ent * H
        onehot = (np.arange(A)[None, :] == act[:, None]).astype(np.float64)
        GL = np.where(live, sc * (g[:, None] * (onehot - pi) + ent * (pi * (lpa + H[:, None]))), 0.0)
        GV = sc * (vf * gv)
    good = ~bad
    u = np.stack([total, Lpi, Lv, H, kl, clipped.astype(np.float64), np.ones(B), clamped.astype(np.float64)], axis=1)
    u = np.where(good[:, None], u, 0.0)
    loss, grad_logits, grad_value = total.astype(np.float32), GL.astype(np.float32), GV.astype(np.float32)
    loss[bad], grad_logits[bad], grad_value[bad] = 0.0, 0.0, 0.0
    partials, sums = tree_sums(u)
    stats = np.array([s if STATS[k] in ("good", "clamped") else s / np.float64(B) for k, s in enumerate(sums)], np.float64)
    return dict(loss=loss, grad_logits=grad_logits, grad_value=grad_value, stats=stats, mean_loss=np.array([stats[0]], np.float32), partials=partials,
                bad_rows=int(bad.sum()), bad=bad, live=live, total=total, GL=GL, GV=GV, u=u, r=r, d=d, H=H, Lpi=Lpi, Lv=Lv, second=second,
                clamped=clamped, vsecond=vsecond, vclamped=vclamped, pi=pi, g=g)


# ---- the inputs of tests/test_gpu_ppo_loss.py: the sorts of sample take turns, sample i of sort (i + shift) % len(SORTS) ------------------
SIDES = {"below": np.log(0.5), "inside": np.log(1.05), "above": np.log(1.6)}      # log r: below, inside and above [0.8, 1.2]
SORTS = ("normal", "pos_below", "pos_inside", "pos_above", "neg_below", "neg_inside", "neg_above", "d_above_20", "d_below_20", "masked", "far_below",
         "action_masked", "action_minus_1", "action_A", "nan_logit", "inf_logit", "all_masked", "logp_bad", "adv_bad", "value_bad", "ret_bad",
         "value_old_bad", "vclip_active", "vclip_inactive", "vclip_inside", "adv_big", "adv_big_neg", "equal")
BAD_ALWAYS = ("action_masked", "action_minus_1", "action_A", "nan_logit", "inf_logit", "all_masked", "logp_bad", "adv_bad", "value_bad", "ret_bad")
BAD_CLIP_VF = ("value_old_bad",)                                     # bad when the value function is clipped: value_old is read
NOT_FINITE = (np.nan, np.inf, -np.inf)


def _logp(row, a):
    """The taken action's log-probability in plain float64 numpy (to place logp_old near it; not the rule)."""
    with np.errstate(divide="ignore"):
        x = row.astype(np.float64)
        x = x - x.max()
        return x[a] - np.log(np.exp(x).sum())


def make_case(rng, B, A, shift=0):
    """dict(logits float32 [B, A], action int64 [B], logp, adv, value, value_old, ret float32 [B], sort: the samples' sorts)."""
    logits = (2.0 * rng.normal(size=(B, A))).astype(np.float32)
    action = rng.integers(0, A, size=B).astype(np.int64)
    adv = rng.normal(size=B).astype(np.float32)
    value_old = rng.normal(size=B).astype(np.float32)
    value = (value_old + 0.3 * rng.normal(size=B)).astype(np.float32)
    ret = (value_old + rng.normal(size=B)).astype(np.float32)
    offset = 0.15 * rng.normal(size=B)                               # log r of a normal sample
    sorts = [SORTS[(i + shift) % len(SORTS)] for i in range(B)]
    logp = np.zeros(B, np.float32)
    for i, sort in enumerate(sorts):
        turn = i // len(SORTS)
        a = int(action[i])
        other = (a + 1 + int(rng.integers(A - 1))) % A               # an action that is not the taken one
        if sort in ("masked", "action_masked"):
            logits[i, a if sort == "action_masked" else other] = -np.inf
        elif sort == "far_below":                                    # finite, and more than 45 below the largest: no weight
            logits[i, other] = np.delete(logits[i], other).max() - np.float32((45.5, 60.0, 300.0)[turn % 3])
        elif sort == "nan_logit":
            logits[i, rng.integers(A)] = np.nan
        elif sort == "inf_logit":
            logits[i, rng.integers(A)] = np.inf
        elif sort == "all_masked":
            logits[i] = -np.inf
        elif sort == "equal":
            logits[i] = logits[i, 0]
        elif sort == "action_minus_1":
            action[i] = (-1, -2, -(1 << 40), -(1 << 63))[turn % 4]
        elif sort == "action_A":
            action[i] = (A, A + 1, 1 << 32, (1 << 63) - 1)[turn % 4]  # 1 << 32: its low word is a valid action
        with np.errstate(invalid="ignore"):
            fine = 0 <= action[i] < A and np.isfinite(logits[i, a]) and not (np.isnan(logits[i]).any() or (logits[i] == np.inf).any())
        lp = _logp(logits[i], a) if fine else -1.0
        if sort[:4] in ("pos_", "neg_"):
            sign, side = (1.0 if sort[:3] == "pos" else -1.0), SIDES[sort[4:]]
            adv[i] = np.float32(sign * (0.5 + abs(adv[i])))
            logp[i] = np.float32(lp - side * (1.0 + 0.1 * rng.random()))
        elif sort == "d_above_20":
            logp[i] = np.float32(lp - (20.5, 25.0, 80.0)[turn % 3])
        elif sort == "d_below_20":
            logp[i] = np.float32(lp + (20.5, 25.0, 80.0)[turn % 3])
        else:
            logp[i] = np.float32(lp - offset[i])
        if sort == "logp_bad":
            logp[i] = NOT_FINITE[turn % 3]
        elif sort == "adv_bad":
            adv[i] = NOT_FINITE[turn % 3]
        elif sort == "value_bad":
            value[i] = NOT_FINITE[turn % 3]
        elif sort == "ret_bad":
            ret[i] = NOT_FINITE[turn % 3]
        elif sort == "value_old_bad":
            value_old[i] = NOT_FINITE[turn % 3]
        elif sort == "vclip_active":                                 # value moved past the range towards ret: the clipped error is the larger
            s = 1.0 if turn % 2 else -1.0
            value[i] = np.float32(value_old[i] + s * (0.3 + rng.random()))
            ret[i] = np.float32(value_old[i] + s * (2.0 + rng.random()))
        elif sort == "vclip_inactive":                               # past the range, away from ret: the plain error is the larger
            s = 1.0 if turn % 2 else -1.0
            value[i] = np.float32(value_old[i] + s * (1.0 + rng.random()))
            ret[i] = np.float32(value_old[i] - s * (0.5 + rng.random()))
        elif sort == "vclip_inside":                                 # u == uc
            value[i] = np.float32(value_old[i] + 0.15 * (2.0 * rng.random() - 1.0))
        elif sort in ("adv_big", "adv_big_neg"):                     # magnitudes 1 and 1e3 in one sum: the order of the additions shows
            adv[i] = np.float32((1.0 if sort == "adv_big" else -1.0) * 1e3 * (1.0 + rng.random()))
    return dict(logits=logits, action=action, logp=logp, adv=adv, value=value, value_old=value_old, ret=ret, sort=np.array(sorts))


def bad_rows_of(B, shift=0, clip_v=True):
    bad = BAD_ALWAYS + (BAD_CLIP_VF if clip_v else ())
    return sum(SORTS[(i + shift) % len(SORTS)] in bad for i in range(B))


def rule_of(c, clip_vf=CLIP_VFS[1], scale=1.0, **kw):
    return ppo_rule(c["logits"], c["action"], c["logp"], c["adv"], c["value"], c["value_old"] if clip_vf >= 0 else None, c["ret"],
                    clip_vf=clip_vf, scale=scale, **kw)


def test_the_generated_inputs_contain_every_sort_and_the_order_of_the_sums_shows():
    for A, c in helpers.cases_per_action(make_case, ACTIONS, len(SORTS) * 48):
        sort = c["sort"]
        B = len(sort)
        on, off = rule_of(c, CLIP_VFS[1]), rule_of(c, CLIP_VFS[0])
        assert set(sort) == set(SORTS)
        assert on["bad_rows"] == bad_rows_of(B) == B // len(SORTS) * 11 and off["bad_rows"] == bad_rows_of(B, clip_v=False) == B // len(SORTS) * 10
        assert set(sort[on["bad"]]) == set(BAD_ALWAYS + BAD_CLIP_VF) and set(sort[off["bad"]]) == set(BAD_ALWAYS)
        r, lo, hi = on["r"], 1.0 - CLIP, 1.0 + CLIP
        for sign, name in ((1, "pos"), (-1, "neg")):                 # all six cases of the sign of adv and the side of r
            for side, where in (("below", r < lo), ("inside", (r > lo) & (r < hi)), ("above", r > hi)):
                rows = sort == "%s_%s" % (name, side)
                assert rows.sum() >= 3 and where[rows].all() and (np.sign(c["adv"][rows]) == sign).all(), (name, side)
        # the clipped branch is the smaller one exactly for (adv > 0, above) and (adv < 0, below)
        assert on["second"][(sort == "pos_above") | (sort == "neg_below")].all()
        assert not on["second"][(sort == "pos_below") | (sort == "neg_above") | (sort == "pos_inside") | (sort == "neg_inside")].any()
        assert on["clamped"][(sort == "d_above_20") | (sort == "d_below_20")].all() and (on["d"][sort == "d_above_20"] > 20).all()
        assert (on["d"][sort == "d_below_20"] < -20).all() and not on["clamped"][sort == "normal"].any()
        assert on["stats"][7] == on["clamped"][~on["bad"]].sum() == B // len(SORTS) * 2
        live, l = on["live"], c["logits"]
        good = ~on["bad"]
        assert (np.isneginf(l) & ~live)[good].any() and (np.isfinite(l) & ~live)[good].any()      # masked, and far below
        assert (~np.isfinite(l[np.arange(B), np.clip(c["action"], 0, A - 1)]))[sort == "action_masked"].all()
        assert (c["action"] < 0).any() and (c["action"] >= A).any() and (c["action"] == 1 << 32).any() == (B // len(SORTS) > 2)
        assert np.isnan(l).any() and (l == np.inf).any() and np.isneginf(l).all(axis=1).any()
        for k in ("logp", "adv", "value", "ret", "value_old"):
            assert np.isnan(c[k]).any() and (c[k] == np.inf).any() and (c[k] == -np.inf).any(), k
        assert on["vsecond"][sort == "vclip_active"].all() and on["vclamped"][sort == "vclip_active"].all()
        assert not on["vsecond"][sort == "vclip_inactive"].any() and on["vclamped"][sort == "vclip_inactive"].all()
        assert not on["vclamped"][sort == "vclip_inside"].any() and not off["vsecond"].any() and not off["vclamped"].any()
        assert not on["GV"][sort == "vclip_active"].any() and on["GV"][sort == "vclip_inactive"].all()
        big = np.abs(c["adv"][good])
        assert (big > 1e3).any() and (big < 2.0).any()
        assert ((l == l[:, :1]).all(axis=1) & good).any()
    # the stated tree against a plain sum in index order: at B = 4097 they differ in at least one bit, so the GPU test can tell them apart
    for A in ACTIONS:
        for clip_vf in CLIP_VFS:
            out = rule_of(make_case(np.random.default_rng(100 * A + 4097 + 4097 % len(SORTS)), 4097, A, 4097 % len(SORTS)), clip_vf)
            plain = np.float64(0.0)
            for t in out["u"][:, 0]:
                plain = plain + t
            tree = tree_sums(out["u"])[1][0]
            assert np.float64(plain).tobytes() != np.float64(tree).tobytes(), (A, clip_vf, plain, tree)
            assert abs(plain - tree) <= 1e-9 * np.abs(out["u"][:, 0]).sum()                      # the same sum, in another order


# ---- properties --------------------------------------------------------------------------------------------------------------------------
def test_the_entropy_has_soft_rules_bytes_on_good_samples():
    for A, c in helpers.cases_per_action(make_case, ACTIONS, len(SORTS) * 48):
        for clip_vf in CLIP_VFS:
            out = rule_of(c, clip_vf)
            want = soft_rule(c["logits"])["entropy"]
            good = ~out["bad"]
            assert good.sum() > len(good) // 2
            assert out["H"][good].astype(np.float32).tobytes() == want[good].tobytes()
            assert np.array_equal(out["u"][good, 3], out["H"][good]) and not out["u"][~good].any()


def test_the_reduction_is_the_stated_tree():
    rng = np.random.default_rng(3)
    for B in (1, 2, 63, 64, 65, 4095, 4096, 4097, 8193):
        u = rng.normal(size=(B, 8)) * 10.0 ** rng.integers(-3, 4, size=(B, 8))
        partials, sums = tree_sums(u)
        W = (B + 63) // 64
        assert partials.shape == (W, 8)
        for k in (0, 7):                                             # the same order, written with scalars
            col = np.zeros(W * 64)
            col[:B] = u[:, k]
            want_p = []
            for w in range(W):
                v = list(col[64 * w:64 * w + 64])
                for off in (32, 16, 8, 4, 2, 1):
                    v = [v[j] + v[j ^ off] for j in range(64)]
                assert len(set(np.float64(x).tobytes() for x in v)) == 1      # every lane holds the sum: a + b == b + a
                want_p.append(v[0])
            assert np.array(want_p).tobytes() == np.ascontiguousarray(partials[:, k]).tobytes()
            t = []
            for j in range(64):
                s = np.float64(0.0)
                for w in range(j, W, 64):
                    s = s + want_p[w]
                t.append(s)
            for off in (32, 16, 8, 4, 2, 1):
                t = [t[j] + t[j ^ off] for j in range(64)]
            assert np.float64(t[0]).tobytes() == np.float64(sums[k]).tobytes(), (B, k)


EPS_EXP, DELTA_LOG = 2e-12, 1e-12
ROUND = 2.0 ** -48                                                   # a few dozen float64 roundings, each 2^-53 relative


def _bounds(out, c, scale, ent_coef=ENT_COEF):
    """The bounds of the test below, per row: (loss [B], grad_logits [B], grad_value [B])."""
    err_l = DELTA_LOG + 2.0 * EPS_EXP                                # L, and so every lp_a
    err_h = err_l + 2.0 * EPS_EXP * 2.0 * np.log(8.0)
    rho = err_l + EPS_EXP                                            # r, relative
    ra = np.abs(out["r"] * c["adv"].astype(np.float64))
    ent = abs(ent_coef)
    loss = rho * ra + ent * err_h + ROUND * (np.abs(out["Lpi"]) + VF_COEF * out["Lv"] + ent * np.abs(out["H"]) + 1.0)
    gl = abs(scale) * (ra * (rho + 2.0 * EPS_EXP) + ent * (6.2 * EPS_EXP + err_l + err_h) + ROUND * (ra + 3.0 * ent + 1.0))
    gv = ROUND * (np.abs(out["GV"]) + abs(scale))
    return loss, gl, gv


def _torch_reference(c, out, clip_vf, scale, rows):
    """(total, d total / d logits, d total / d value) of `rows`, scaled, in float64 torch: log_softmax, exp, clamp, minimum / maximum and
    autograd.  A masked logit becomes -1e4 (probability exactly 0 with a finite log, so that autograd's products stay finite)."""
    import torch

    t = lambda a: torch.tensor(np.asarray(a, np.float64)[rows], dtype=torch.float64)  # noqa: E731
    l = torch.tensor(np.where(np.isneginf(c["logits"]), -1e4, c["logits"].astype(np.float64))[rows], dtype=torch.float64, requires_grad=True)
    value = t(c["value"]).requires_grad_()
    logp_all = torch.log_softmax(l, dim=1)
    lp = logp_all.gather(1, torch.tensor(c["action"][rows])[:, None])[:, 0]
    ratio = torch.exp((lp - t(c["logp"])).clamp(-LOGRATIO_MAX, LOGRATIO_MAX))
    adv = t(c["adv"])
    lpi = -torch.minimum(ratio * adv, ratio.clamp(1.0 - CLIP, 1.0 + CLIP) * adv)
    h = -(logp_all.exp() * logp_all).sum(dim=1)
    ret = t(c["ret"])
    if clip_vf >= 0:
        old = t(c["value_old"])
        lv = 0.5 * torch.maximum((value - ret) ** 2, ((old + (value - old).clamp(-clip_vf, clip_vf)) - ret) ** 2)
    else:
        lv = 0.5 * (value - ret) ** 2
    total = lpi + VF_COEF * lv - ENT_COEF * h
    (scale * total).sum().backward()
    return total.detach().numpy(), l.grad.numpy(), value.grad.numpy()


def test_loss_and_gradients_stay_within_the_derived_bound_of_float64_torch_and_autograd():
    """The bound is derived from the header's 1e-12 on EXP and LOG, not fitted to what is seen (which is printed: some 1e-4 of it).
    EXP is ldexp(p, k) with p in [0.707, 1.415): the header's absolute 1e-12 at k = 0 is a relative 1.42e-12 of p, the scaling is
    exact and the reduced argument carries some 1e-15 more, so EXP and 1 / EXP are within eps = 2e-12 relative.  LOG is within
    delta = 1e-12 absolute.  From these, per sample:
        S: eps relative;  L = LOG(S) and every lp_a = x_a - L:  err_l = delta + 2 eps  absolute;  pi_a: 2 eps relative
        H = L - sum pi_a x_a, with sum pi_a |x_a| <= H + L <= 2 ln 8:  err_h = err_l + 2 eps * 2 ln 8
        r = EXP(lp - logp_old):  rho = err_l + eps  relative;  Lpi = -min(r adv, rc adv):  rho * r |adv|  (min and the clamp are 1-Lipschitz)
        Lv, gv: float64 operations on float32 inputs, roundings only
      loss        <= rho r |adv| + |ent_coef| err_h + ROUND (|Lpi| + vf_coef Lv + |ent_coef| H + 1)
      grad_logits <= scale (r |adv| (rho + 2 eps) + |ent_coef| (6.2 eps + err_l + err_h) + ROUND (r |adv| + 3 |ent_coef| + 1))
                     (g (onehot - pi_a): rho on g, 2 eps on pi_a;  pi_a (lp_a + H): 2 eps (pi_a |lp_a| + pi_a H <= 1 + ln 8 <= 3.1), and err_l + err_h)
      grad_value  <= ROUND (|grad_value| + scale)
    with ROUND = 2^-48 for the few dozen roundings.  Samples exactly on a clip boundary (r within 1e-9 of 1 +- clip, where the two sides'
    gradients differ and a last-bit difference of r picks the side; or the value's two squared errors equal with the value clipped) are
    left out of the comparison: under 1 % of the rows."""
    seen = np.zeros(3)
    rows_seen = 0
    for A, c in helpers.cases_per_action(make_case, ACTIONS, len(SORTS) * 240):
        for clip_vf in CLIP_VFS:
            for scale in (1.0, 1.0 / 4096.0):
                out = rule_of(c, clip_vf, scale)
                good = ~out["bad"]
                edge = (np.abs(out["r"] - (1.0 - CLIP)) < 1e-9) | (np.abs(out["r"] - (1.0 + CLIP)) < 1e-9)
                if clip_vf >= 0:
                    dv = c["value"].astype(np.float64) - c["ret"]
                    uc = np.clip(c["value"].astype(np.float64) - c["value_old"], -clip_vf, clip_vf)
                    with np.errstate(invalid="ignore"):
                        edge |= out["vclamped"] & (dv * dv == ((c["value_old"] + uc) - c["ret"]) ** 2)
                assert (edge & good).sum() < 0.01 * len(good)
                rows = good & ~edge
                assert rows.sum() >= len(rows) // 2
                total, GL, GV = _torch_reference(c, out, clip_vf, scale, rows)
                b_loss, b_gl, b_gv = (b[rows] for b in _bounds(out, c, scale))
                ratios = (np.abs(out["total"][rows] - total) / b_loss, (np.abs(out["GL"][rows] - GL) / b_gl[:, None]).max(axis=1),
                          np.abs(out["GV"][rows] - GV) / b_gv)
                seen = np.maximum(seen, [x.max() for x in ratios])
                rows_seen += int(rows.sum())
                for name, x in zip(("loss", "grad_logits", "grad_value"), ratios):
                    assert x.max() <= 1.0, (A, clip_vf, scale, name, x.max(), c["sort"][rows][x.argmax()])
    print("largest error / bound: loss %.3g, grad_logits %.3g, grad_value %.3g over %d rows" % (seen[0], seen[1], seen[2], rows_seen))


def test_bad_samples_give_zeros_add_nothing_and_are_counted():
    for A, c in helpers.cases_per_action(make_case, ACTIONS, len(SORTS) * 48):
        B = len(c["sort"])
        for clip_vf in CLIP_VFS:
            out = rule_of(c, clip_vf, 1.0 / B)
            bad = out["bad"]
            assert out["bad_rows"] == bad.sum() == bad_rows_of(B, clip_v=clip_vf >= 0) > 0
            for k in ("loss", "grad_logits", "grad_value"):
                assert out[k].dtype == np.float32 and not out[k][bad].view(np.uint32).any() and np.isfinite(out[k]).all(), k
            assert not out["u"][bad].any() and out["stats"][6] == B - out["bad_rows"]
            assert not out["grad_logits"][~out["live"]].view(np.uint32).any()                   # a masked action: exactly +0.0
            only_good = {k: (v[~bad] if k != "sort" else v) for k, v in c.items() if k != "sort"}
            alone = ppo_rule(only_good["logits"], only_good["action"], only_good["logp"], only_good["adv"], only_good["value"],
                             only_good["value_old"] if clip_vf >= 0 else None, only_good["ret"], clip_vf=clip_vf)
            assert alone["bad_rows"] == 0 and np.allclose(alone["stats"][:6] * len(alone["loss"]), out["stats"][:6] * B, rtol=1e-12, atol=1e-9)
            assert out["mean_loss"].dtype == np.float32 and out["mean_loss"][0] == np.float32(out["stats"][0])
            assert abs(out["stats"][0] - out["total"][~bad].sum() / B) <= 1e-12 * np.abs(out["total"][~bad]).sum() / B
            # the gradient of a sample's logits sums to zero (both parts do), up to the bound of the comparison above
            assert (np.abs(out["GL"][~bad].sum(axis=1)) <= A * _bounds(out, c, 1.0 / B)[1][~bad]).all()


# ---- the C entry point -------------------------------------------------------------------------------------------------------------------
def _ppo(L, B=4, A=5, logits=PH, action=PH, logp=PH, adv=PH, value=PH, value_old=PH, ret=PH, clip=0.2, clip_vf=0.2, vf_coef=0.5, ent_coef=0.01,
         scale=1.0, loss=PH, gl=PH, gv=PH, stats=PH, mean=PH, partials=PH, bad=PH):
    return L.snac_ppo_loss(B, A, logits, action, logp, adv, value, value_old, ret, clip, clip_vf, vf_coef, ent_coef, scale, loss, gl, gv, stats, mean,
                           partials, bad, None)


def test_the_library_exports_the_entry_point():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    assert "snac_ppo_loss" in _lib.EXPORTS and len(L.snac_ppo_loss.argtypes) == 22 and _lib.PPO_STATS == 8
    res, args = _lib.PROTOTYPES["snac_ppo_loss"]
    assert res == C.c_int and args[:2] == [C.c_int32, C.c_int32] and args[9:14] == [C.c_double] * 5
    assert all(t == C.c_void_p for t in args[2:9] + args[14:])


def test_ppo_loss_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _err(L, _ppo(L, logits=None), -1, b"null logits")
    _err(L, _ppo(L, action=None), -1, b"null action")
    for k in ("logp", "adv", "value", "ret"):
        _err(L, _ppo(L, **{k: None}), -1, b"logp_old, adv, value and ret are needed")
    for B in (0, -1, -(1 << 31)):
        _err(L, _ppo(L, B=B), -1, b"B must be >= 1")
    for clip in (0.0, -0.2, float("nan"), float("inf"), float("-inf")):
        _err(L, _ppo(L, clip=clip), -1, b"clip must be finite and > 0")
    for k, word in (("clip_vf", b"clip_vf must be finite"), ("vf_coef", b"vf_coef must be finite"), ("ent_coef", b"ent_coef must be finite"),
                    ("scale", b"scale must be finite")):
        for x in (float("nan"), float("inf"), float("-inf")):
            _err(L, _ppo(L, **{k: x}), -1, word)
    for clip_vf in (0.0, 0.2, 5.0):
        _err(L, _ppo(L, clip_vf=clip_vf, value_old=None), -1, b"value_old is needed when clip_vf >= 0")
    for clip_vf in (-1.0, -1e-30):
        _err(L, _ppo(L, clip_vf=clip_vf), -1, b"value_old belongs to clip_vf >= 0")
    _err(L, _ppo(L, partials=None), -1, b"partials are needed for stats")
    _err(L, _ppo(L, stats=None), -1, b"stats is needed")
    _err(L, _ppo(L, action=C.c_void_p((1 << 20) + 4)), -1, b"action must be 8-byte aligned")
    _err(L, _ppo(L, stats=C.c_void_p((1 << 20) + 4)), -1, b"stats and partials must be 8-byte aligned")
    _err(L, _ppo(L, partials=C.c_void_p((1 << 20) + 4)), -1, b"stats and partials must be 8-byte aligned")
    for A in (0, 1, 2, 4, 6, 7, 9, -3):
        _err(L, _ppo(L, A=A), -3, b"num_actions must be 3, 5 or 8")
    # no output: no launch, although no device exists to launch on -- but the checks come first
    none = dict(loss=None, gl=None, gv=None, stats=None, mean=None, bad=None)
    for A in ACTIONS:
        assert _ppo(L, A=A, **none) == 0 and _ppo(L, A=A, partials=None, **none) == 0
        assert _ppo(L, A=A, clip_vf=-1.0, value_old=None, **none) == 0
    _err(L, _ppo(L, B=0, **none), -1, b"B must be >= 1")
    _err(L, _ppo(L, A=4, **none), -3, b"num_actions must be")
    _err(L, _ppo(L, clip=0.0, **none), -1, b"clip must be finite")


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------------
def test_ppo_loss_checks_its_arguments_before_it_touches_a_device():
    import torch
    from snac_amd import PPOLoss

    ok = dict(num_actions=5, device="cuda:0")
    for bad in (dict(num_actions=4), dict(num_actions=True), dict(num_actions="5"), dict(num_actions=5.0), dict(device="cpu"), dict(device=None),
                dict(clip=0.0), dict(clip=-0.1), dict(clip=float("nan")), dict(clip="0.2"), dict(clip_vf=float("inf")), dict(vf_coef=float("nan")),
                dict(ent_coef=None), dict(vf_coef=True)):
        with pytest.raises(ValueError):
            PPOLoss(**dict(ok, **bad))
    ppo = PPOLoss(5, device="cuda:0")
    assert ppo.num_actions == 5 and ppo.device == torch.device("cuda:0") and ppo.env is None and ppo.stats is None
    assert (ppo.clip, ppo.clip_vf, ppo.vf_coef, ppo.ent_coef) == (0.2, 0.2, 0.5, 0.01)      # clip_vf None: PPO2's default, the policy's range
    assert PPOLoss(3, clip=0.1, device="cuda:0").clip_vf == 0.1 and PPOLoss(3, clip_vf=-1, device="cuda:0").clip_vf == -1.0
    with pytest.raises(ValueError, match="no loss"):
        ppo.stats_dict()
    l, v, a = torch.zeros(4, 5), torch.zeros(4), torch.zeros(4, dtype=torch.int64)
    mb = dict(action=a, logp=v, adv=v, ret=v, value=v)
    with pytest.raises(ValueError, match=r"logits must have shape \(B, 5\), got \(4, 3\)"):
        ppo.loss(torch.zeros(4, 3), v, mb)
    with pytest.raises(ValueError, match="logits must have shape"):
        ppo.loss(torch.zeros(0, 5), torch.zeros(0), mb)
    with pytest.raises(ValueError, match="logits must be a contiguous torch.float32 tensor"):
        ppo.loss(l.double(), v, mb)
    with pytest.raises(ValueError, match="logits must be a contiguous torch.float32 tensor"):
        ppo.loss(torch.zeros(4, 10)[:, ::2], v, mb)
    with pytest.raises(ValueError, match="logits must be on cuda:0"):
        ppo.loss(l, v, mb)
    with pytest.raises(ValueError, match="logits must be on cuda:0"):
        ppo.loss(l.requires_grad_(), v, (a, v, v, v, v))


# ---- the kernel's code on the host -------------------------------------------------------------------------------------------------------
OUTPUTS = ("loss", "grad_logits", "grad_value", "stats", "mean_loss", "partials")
HOST_SRC = os.path.join(helpers.TESTS, "native", "ppo_host.cpp")
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", _lib.CSRC, HOST_SRC]


def test_the_kernels_code_compiled_for_the_host_equals_the_rule_byte_for_byte(tmp_path):
    fn = load_shared(tmp_path, "ppo_host", ["-O2", "-fPIC", "-shared"] + HOST_FLAGS, timeout=600).ppo_host
    fn.restype, fn.argtypes = C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 7 + [C.c_double] * 5 + [C.c_void_p] * 6
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for A in ACTIONS:
        for B in (1, 64, 65, 4097, 8193):
            shifts = range(len(SORTS)) if B == 1 else (B % len(SORTS),)
            for shift in shifts:
                c = make_case(np.random.default_rng(100 * A + B + shift), B, A, shift)
                for clip_vf in CLIP_VFS:
                    want = rule_of(c, clip_vf, 1.0 / B)
                    W = (B + 63) // 64
                    got = dict(loss=np.full(B, 7, np.float32), grad_logits=np.full((B, A), 7, np.float32), grad_value=np.full(B, 7, np.float32),
                               stats=np.full(8, 7, np.float64), mean_loss=np.full(1, 7, np.float32), partials=np.full((W, 8), 7, np.float64))
                    bad = fn(B, A, vp(c["logits"]), vp(c["action"]), vp(c["logp"]), vp(c["adv"]), vp(c["value"]),
                             vp(c["value_old"]) if clip_vf >= 0 else None, vp(c["ret"]), CLIP, clip_vf, VF_COEF, ENT_COEF, 1.0 / B,
                             *[vp(got[k]) for k in OUTPUTS])
                    assert bad == want["bad_rows"] == bad_rows_of(B, shift, clip_vf >= 0), (A, B, shift, bad, want["bad_rows"])
                    for k in OUTPUTS:
                        _same(got[k], want[k], (A, B, shift, clip_vf, k))
    # no statistics asked for: stats, mean_loss and partials are not touched
    loss, stats = np.full(B, 7, np.float32), np.full(8, 7, np.float64)
    assert fn(B, A, vp(c["logits"]), vp(c["action"]), vp(c["logp"]), vp(c["adv"]), vp(c["value"]), None, vp(c["ret"]), CLIP, -1.0, VF_COEF, ENT_COEF,
              1.0, vp(loss), None, None, None, None, None) == bad_rows_of(B, shift, False)
    _same(loss, rule_of(c, -1.0)["loss"], "the losses alone")


def test_the_kernels_code_runs_clean_under_the_host_sanitizers_with_actions_out_of_range(tmp_path):
    """A stand-alone program (ppo_host.cpp with its main), not code loaded into python."""
    r = run_sanitized(tmp_path, "ppo_host_main", ["-DPPO_HOST_MAIN"] + HOST_FLAGS, probe_timeout=300, build_timeout=600, run_timeout=300)
    assert r.stdout.count("bad ") == 18 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
