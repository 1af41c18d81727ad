"""Host: the rule of include/snac_hip.h, "Soft values (discrete SAC)", restated in numpy (soft_rule), independently of the kernel
(tests/test_gpu_sac.py compares the kernel with it byte for byte): its entropy against policy_rule's bytes, its value and gradient before
the rounding to float32 against a float64 torch log_softmax computation and torch autograd, masking, the gradient's sum, bad samples, and
the inputs the GPU test runs on (make_case: that they contain every sort is asserted here).  Then snac_soft_value is exported and checks
every argument before any HIP call -- each failing call below fails its checks first, so the placeholder pointers are never dereferenced --
and SoftValue checks its tensors before it touches a device.  Last, the per-sample function the kernel runs (snac_amd/csrc/soft_rule.h)
is compiled for the host with the system compiler and compared with soft_rule byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cabi_checks import PH, _err_code as _err
import helpers
from hostcode import _compiler
from snac_amd import _lib
from specmath import _same, spec_exp, spec_log
from test_policy_act_host import CATEGORICAL, policy_rule

ACTIONS = (3, 5, 8)
ALPHAS = (0.0, 0.2, 1.0)


# ---- the rule, in numpy: every ufunc call below is one float64 operation, rounded on its own --------------------------------------------
def soft_rule(logits, q1=None, q2=None, alpha=None, ret=None, discount=None, scale=1.0):
    """-> dict(v, y, entropy float32 [B], grad float32 [B, A], bad_rows int; and before the rounding to float32: V, G float64, dmax [B] =
    max |d_a| over the live actions, live bool [B, A], bad bool [B]).  q1 None: the entropy alone (q1, q2 and alpha are not read; v, y
    and grad are None).  ret None: no y."""
    l = np.asarray(logits, np.float32)
    B, A = l.shape
    use_q, want_y = q1 is not None, ret is not None
    m = l[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for a in range(1, A):
            m = np.where(l[:, a] > m, l[:, a], m)
        bad = np.isnan(l).any(axis=1) | (l == np.inf).any(axis=1) | (m == -np.inf)
        if use_q:
            al32 = np.float32(alpha)
            if not np.isfinite(al32) or al32 < 0:
                bad = np.ones(B, bool)
        if want_y:
            ret, discount = np.asarray(ret, np.float32), np.asarray(discount, np.float32)
            bad = bad | ~np.isfinite(ret) | ~np.isfinite(discount) | (discount < 0)
    l, m = l.copy(), m.copy()
    l[bad], m[bad] = 0.0, 0.0                                        # (bad samples are zeroed below)
    x = l.astype(np.float64) - m.astype(np.float64)[:, None]
    e = spec_exp(x)
    S, T = np.zeros(B), np.zeros(B)
    with np.errstate(invalid="ignore"):
        for a in range(A):
            S = S + e[:, a]
            T = T + np.where(e[:, a] == 0.0, 0.0, e[:, a] * x[:, a])
    L = spec_log(S)
    entropy = (L - T / S).astype(np.float32)
    entropy[bad] = 0.0
    out = dict(v=None, y=None, entropy=entropy, grad=None, bad_rows=int(bad.sum()), bad=bad, live=e != 0.0)
    if not use_q:
        return out
    q1 = np.asarray(q1, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        qm = (q1 if q2 is None else np.where(np.asarray(q2, np.float32) < q1, np.asarray(q2, np.float32), q1)).astype(np.float64)
        live = e != 0.0
        pi = e / S[:, None]
        lp = x - L[:, None]
        al = np.float64(np.float32(0.0) if bad.all() else al32)
        d = np.where(live, qm - al * lp, 0.0)
        V = np.zeros(B)
        for a in range(A):
            V = V + np.where(live[:, a], pi[:, a] * d[:, a], 0.0)
        G = np.where(live, np.float64(scale) * (pi * (V[:, None] - d)), 0.0)
        v, grad = V.astype(np.float32), G.astype(np.float32)
        v[bad], grad[bad] = 0.0, 0.0
        out.update(v=v, grad=grad, V=V, G=G, dmax=np.abs(d).max(axis=1))
        if want_y:
            y = (np.where(bad, 0.0, ret.astype(np.float64)) + np.where(bad, 0.0, discount.astype(np.float64)) * V).astype(np.float32)
            y[bad] = 0.0
            out["y"] = y
    return out


# ---- the inputs of tests/test_gpu_sac.py: the sorts of sample take turns, sample i of sort (i + shift) % len(SORTS) -----------------------
SORTS = ("normal", "equal", "one_masked", "several_masked", "far_below", "nan_logit", "inf_logit", "all_masked", "q_nan_masked", "q_nan_live",
         "q2_below", "q1_below", "q_tie", "ret_inf", "ret_nan", "discount_negative", "discount_0", "discount_1", "discount_3_steps", "one_live",
         "scaled")
BAD_LOGITS = ("nan_logit", "inf_logit", "all_masked")                # bad in every call
BAD_Y = ("ret_inf", "ret_nan", "discount_negative")                  # bad when y is asked for


def make_case(rng, B, A, shift=0):
    """dict(logits, q1, q2 float32 [B, A], ret, discount float32 [B], sort: the samples' sorts)."""
    logits = (3.0 * rng.normal(size=(B, A))).astype(np.float32)
    q1, q2 = (5.0 * rng.normal(size=(B, A))).astype(np.float32), (5.0 * rng.normal(size=(B, A))).astype(np.float32)
    ret = rng.uniform(-5.0, 5.0, size=B).astype(np.float32)
    discount = np.full(B, 0.95, np.float32)
    sorts = [SORTS[(i + shift) % len(SORTS)] for i in range(B)]
    for i, sort in enumerate(sorts):
        turn = i // len(SORTS)
        if sort == "equal":
            logits[i] = logits[i, 0]
        elif sort == "one_masked":
            logits[i, rng.integers(A)] = -np.inf
        elif sort == "several_masked":
            logits[i, rng.choice(A, size=2 if A == 3 else A - 2, replace=False)] = -np.inf
        elif sort == "far_below":                                    # finite, and more than 45 below the largest: no weight
            a = rng.integers(A)
            logits[i, a] = logits[i].max() - np.float32((45.5, 60.0, 300.0)[turn % 3])
        elif sort == "nan_logit":
            logits[i, rng.integers(A)] = np.nan
        elif sort == "inf_logit":
            logits[i, rng.integers(A)] = np.inf
        elif sort == "all_masked":
            logits[i] = -np.inf
        elif sort == "q_nan_masked":                                 # a NaN (or an infinity) where the action is masked: it must not show
            a = rng.integers(A)
            logits[i, a] = -np.inf
            q1[i, a], q2[i, a] = ((np.nan, np.nan), (np.inf, np.nan), (np.nan, -np.inf))[turn % 3]
        elif sort == "q_nan_live":                                   # in q1 it shows; in q2 alone it never wins the minimum
            a = rng.integers(A)
            if turn % 2 == 0:
                q1[i, a] = np.nan
            else:
                q2[i, a] = np.nan
        elif sort == "q2_below":
            q2[i] = q1[i] - np.float32(1.0)
        elif sort == "q1_below":
            q1[i] = q2[i] - np.float32(1.0)
        elif sort == "q_tie":
            q2[i] = q1[i]
        elif sort == "ret_inf":
            ret[i] = (np.inf, -np.inf)[turn % 2]
        elif sort == "ret_nan":
            ret[i] = np.nan
        elif sort == "discount_negative":
            discount[i] = (-0.5, np.nan, np.inf)[turn % 3]
        elif sort == "discount_0":
            discount[i] = 0.0
        elif sort == "discount_1":
            discount[i] = 1.0
        elif sort == "discount_3_steps":
            discount[i] = 0.95 ** 3
        elif sort == "one_live":
            keep = rng.integers(A)
            logits[i, np.arange(A) != keep] = -np.inf
        elif sort == "scaled":
            logits[i] = logits[i] * np.float32(10.0)
    return dict(logits=logits, q1=q1, q2=q2, ret=ret, discount=discount, sort=np.array(sorts))


def bad_rows_of(B, shift=0, want_y=True):
    bad = BAD_LOGITS + (BAD_Y if want_y else ())
    return sum(SORTS[(i + shift) % len(SORTS)] in bad for i in range(B))


def _rule(c, alpha=0.2, two=True, want_y=True, scale=1.0, q1=None, q2=None):
    q1, q2 = c["q1"] if q1 is None else q1, c["q2"] if q2 is None else q2
    return soft_rule(c["logits"], q1, q2 if two else None, alpha, c["ret"] if want_y else None, c["discount"] if want_y else None, scale)


def test_the_generated_inputs_contain_every_sort():
    for A, c in helpers.cases_per_action(make_case, ACTIONS, len(SORTS) * 48):
        l, q1, q2, ret, discount, sort = (c[k] for k in ("logits", "q1", "q2", "ret", "discount", "sort"))
        B = len(ret)
        assert set(sort) == set(SORTS) and bad_rows_of(B) == B // len(SORTS) * 6 and bad_rows_of(B, want_y=False) == B // len(SORTS) * 3
        assert bad_rows_of(1, SORTS.index("ret_nan")) == 1 and bad_rows_of(1, SORTS.index("ret_nan"), want_y=False) == 0 and bad_rows_of(1) == 0
        out = _rule(c)
        assert set(sort[out["bad"]]) == set(BAD_LOGITS + BAD_Y) and out["bad_rows"] == bad_rows_of(B)
        assert set(sort[_rule(c, want_y=False)["bad"]]) == set(BAD_LOGITS)
        good, live = ~out["bad"], out["live"]
        with np.errstate(invalid="ignore"):
            top = np.where(np.isfinite(l), l, -np.inf).max(axis=1)
            far = np.isfinite(l) & (l.astype(np.float64) - top[:, None] < -45.0)
        assert (far & ~live)[good].any() and set(sort[far.any(axis=1) & good]) >= {"far_below", "scaled"}      # finite, and no weight
        assert (np.isneginf(l) & ~live)[good].any() and np.isnan(l).any() and (l == np.inf).any() and np.isneginf(l).all(axis=1).any()
        assert ((l == l[:, :1]).all(axis=1) & good).any()                                                      # equal logits
        assert (live[sort == "one_live"].sum(axis=1) == 1).all() and (live[sort == "several_masked"].sum(axis=1) <= max(1, A - 2)).all()
        masked_nan = (np.isnan(q1) | np.isnan(q2) | np.isinf(q1) | np.isinf(q2)) & ~live
        live_nan1, live_nan2 = np.isnan(q1) & live, np.isnan(q2) & live
        assert masked_nan[sort == "q_nan_masked"].any(axis=1).all() and np.isnan(q1[masked_nan]).any() and np.isinf(q1[masked_nan]).any()
        assert live_nan1[good].any() and live_nan2[good].any() and not (live_nan1 & live_nan2).any()
        assert np.isnan(out["v"][live_nan1.any(axis=1) & good]).all() and np.isfinite(out["v"][live_nan2.any(axis=1) & good]).all()
        assert np.isfinite(out["v"][sort == "q_nan_masked"]).all() and np.isfinite(out["grad"][sort == "q_nan_masked"]).all()
        assert (q2 < q1).all(axis=1).any() and (q1 < q2).all(axis=1).any() and (q1 == q2).all(axis=1).any()
        assert (ret == np.inf).any() and (ret == -np.inf).any() and np.isnan(ret).any()
        assert (discount[~np.isnan(discount)] < 0).any() and np.isnan(discount).any() and np.isinf(discount).any()
        for d in (0.0, 1.0, 0.95 ** 3, 0.95):
            assert (discount == np.float32(d)).any(), d


# ---- properties --------------------------------------------------------------------------------------------------------------------------
def test_the_entropy_is_snac_policy_acts_byte_for_byte():
    """On every sample that is not bad: snac_policy_act draws a bad row as if its scores were 0 and so gives it log(A); here a bad sample
    gives 0.  The logits alone decide the entropy: q, alpha and y change no byte of it."""
    for A, c in helpers.cases_per_action(make_case, ACTIONS, len(SORTS) * 48):
        B = len(c["ret"])
        want = policy_rule(1, np.arange(B), 0, CATEGORICAL, c["logits"])["entropy"]
        alone = soft_rule(c["logits"])
        assert alone["v"] is None and alone["grad"] is None and alone["bad_rows"] == bad_rows_of(B, want_y=False)
        good = ~alone["bad"]
        assert alone["entropy"][good].tobytes() == want[good].tobytes() and not alone["entropy"][~good].any()
        for alpha in ALPHAS:
            full = _rule(c, alpha)
            assert full["entropy"][~full["bad"]].tobytes() == want[~full["bad"]].tobytes() and not full["entropy"][full["bad"]].any()


def _torch_reference(c, alpha, two):
    """(V, dV/dlogits with the sign of the actor loss -V, rows compared) in float64 torch: log_softmax, exp, minimum, autograd.  A masked
    logit becomes -1e4 (its probability is exactly 0 and its log finite, so that autograd's products stay finite) and a q-value at an
    action without weight 0.0: the rule never reads those."""
    import torch

    out = _rule(c, alpha, two, want_y=False)
    rows = ~out["bad"] & np.isfinite(out["V"])
    l = torch.tensor(np.where(np.isneginf(c["logits"]), -1e4, c["logits"].astype(np.float64))[rows], dtype=torch.float64, requires_grad=True)
    with np.errstate(invalid="ignore"):
        qm = np.where(c["q2"] < c["q1"], c["q2"], c["q1"]) if two else c["q1"]
    qm = torch.tensor(np.where(out["live"], qm.astype(np.float64), 0.0)[rows], dtype=torch.float64)
    logp = torch.log_softmax(l, dim=1)
    V = (logp.exp() * (qm - float(np.float32(alpha)) * logp)).sum(dim=1)
    (-V).sum().backward()
    return out, rows, V.detach().numpy(), l.grad.numpy()


def test_value_and_gradient_stay_within_1e_12_of_float64_torch_and_autograd():
    """The bound is the header's 1e-12 on EXP and LOG carried through to V and to the gradient, relative to 1 + max |d_a|; it is derived,
    not measured.  What is seen is printed: about 1e-15."""
    seen_v = seen_g = 0.0
    rows_seen = 0
    for A, c in helpers.cases_per_action(make_case, ACTIONS, len(SORTS) * 320):
        for alpha in ALPHAS:
            for two in (True, False):
                out, rows, V, G = _torch_reference(c, alpha, two)
                assert rows.sum() >= len(rows) * 12 // len(SORTS)
                bound = 1e-12 * (1.0 + out["dmax"][rows])
                err_v, err_g = np.abs(out["V"][rows] - V) / bound, (np.abs(out["G"][rows] - G) / bound[:, None]).max(axis=1)
                seen_v, seen_g, rows_seen = max(seen_v, err_v.max() * 1e-12), max(seen_g, err_g.max() * 1e-12), rows_seen + int(rows.sum())
                assert err_v.max() <= 1.0 and err_g.max() <= 1.0, (A, alpha, two, err_v.max(), err_g.max())
    print("largest |V - torch| / (1 + max|d|) %.3g, largest |grad - autograd| / (1 + max|d|) %.3g over %d rows" % (seen_v, seen_g, rows_seen))


def test_masked_actions_get_no_gradient_and_their_q_values_change_no_byte():
    rng = np.random.default_rng(7)
    for A, c in helpers.cases_per_action(make_case, ACTIONS, len(SORTS) * 48):
        for alpha in ALPHAS:
            out = _rule(c, alpha)
            assert not out["grad"][~out["live"]].any()               # exactly 0, +0.0 bytes
            assert out["grad"][~out["live"]].tobytes() == bytes(4 * int((~out["live"]).sum()))
            junk = np.where(rng.random(c["q1"].shape) < 0.5, np.nan, 1e30 * rng.normal(size=c["q1"].shape)).astype(np.float32)
            other = _rule(c, alpha, q1=np.where(out["live"], c["q1"], junk), q2=np.where(out["live"], c["q2"], -junk))
            for k in ("v", "y", "entropy", "grad"):
                assert out[k].tobytes() == other[k].tobytes(), (A, alpha, k)
            one = c["sort"] == "one_live"                            # one live action: V is its minimum of the critics, exactly
            at = out["live"][one].argmax(axis=1)
            qm = np.minimum(c["q1"], c["q2"])[one, at].astype(np.float64)
            assert one.sum() >= 3 and np.array_equal(out["V"][one], qm) and not out["grad"][one].any() and not out["G"][one].any()
            assert not out["entropy"][one].any()


def test_the_gradient_of_a_sample_sums_to_zero():
    for A, c in helpers.cases_per_action(make_case, ACTIONS, len(SORTS) * 48):
        for alpha in ALPHAS:
            for scale in (1.0, 1.0 / 2048.0):
                out = _rule(c, alpha, want_y=False, scale=scale)
                rows = ~out["bad"] & np.isfinite(out["V"])
                total = np.abs(out["G"][rows].sum(axis=1)) / scale
                assert (total <= 1e-12 * (1.0 + out["dmax"][rows])).all(), (A, alpha, total.max())


def test_bad_samples_give_zeros_and_the_exact_count():
    for A, c in helpers.cases_per_action(make_case, ACTIONS, len(SORTS) * 48):
        B = len(c["ret"])
        out = _rule(c)
        bad = out["bad"]
        assert out["bad_rows"] == bad.sum() == bad_rows_of(B) > 0
        for k in ("v", "y", "entropy"):
            assert not out[k][bad].any() and out[k].dtype == np.float32
        assert not out["grad"][bad].any() and out["grad"].dtype == np.float32
        assert np.isfinite(out["entropy"]).all() and (out["entropy"] >= 0).all()
        assert _rule(c, want_y=False)["bad_rows"] == bad_rows_of(B, want_y=False) < out["bad_rows"]
        for alpha in (np.nan, np.inf, -np.inf, -0.1, -1e-30):        # a bad temperature: every sample of the call
            out = _rule(c, alpha)
            assert out["bad_rows"] == B and not out["v"].any() and not out["y"].any() and not out["entropy"].any() and not out["grad"].any()
        assert soft_rule(c["logits"])["bad_rows"] == bad_rows_of(B, want_y=False)      # the entropy alone reads no alpha
        # y is the combine of ret, discount and V
        out, good = _rule(c), ~_rule(c)["bad"] & np.isfinite(_rule(c)["V"])
        want = (c["ret"][good].astype(np.float64) + c["discount"][good].astype(np.float64) * out["V"][good]).astype(np.float32)
        assert out["y"][good].tobytes() == want.tobytes()
        zero = good & (c["discount"] == 0)
        assert zero.any() and np.array_equal(out["y"][zero], c["ret"][zero])


# ---- the C entry point -------------------------------------------------------------------------------------------------------------------
def _soft(L, B=4, A=5, logits=PH, q1=PH, q2=PH, alpha=PH, ret=PH, discount=PH, scale=1.0, v=PH, y=PH, entropy=PH, grad=PH, bad=PH):
    return L.snac_soft_value(B, A, logits, q1, q2, alpha, ret, discount, scale, v, y, entropy, grad, bad, None)


def test_the_library_exports_the_entry_point():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    assert "snac_soft_value" in _lib.EXPORTS and len(L.snac_soft_value.argtypes) == 15
    args = _lib.PROTOTYPES["snac_soft_value"][1]
    assert args[:2] == [C.c_int32, C.c_int32] and args[8] == C.c_double and all(t == C.c_void_p for t in args[2:8] + args[9:])


def test_soft_value_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _err(L, _soft(L, logits=None), -1, b"null logits")
    for B in (0, -1, -(1 << 31)):
        _err(L, _soft(L, B=B), -1, b"B must be >= 1")
    for scale in (float("nan"), float("inf"), float("-inf")):
        _err(L, _soft(L, scale=scale), -1, b"scale must be finite")
    for outs in (dict(), dict(y=None, ret=None, discount=None), dict(v=None, grad=None), dict(v=None, y=None, ret=None, discount=None, entropy=None)):
        _err(L, _soft(L, q1=None, **outs), -1, b"q1 and alpha are needed")
        _err(L, _soft(L, alpha=None, **outs), -1, b"q1 and alpha are needed")
    _err(L, _soft(L, ret=None), -1, b"ret and discount are needed for y")
    _err(L, _soft(L, discount=None), -1, b"ret and discount are needed for y")
    _err(L, _soft(L, y=None), -1, b"ret and discount belong to y")
    _err(L, _soft(L, y=None, ret=None), -1, b"ret and discount belong to y")
    for A in (0, 1, 2, 4, 6, 7, 9, -3):
        _err(L, _soft(L, A=A), -3, b"num_actions must be 3, 5 or 8")
        _err(L, _soft(L, A=A, v=None, y=None, ret=None, discount=None, grad=None, q1=None, q2=None, alpha=None), -3, b"num_actions must be 3, 5 or 8")
    # no value output: no launch, although no device exists to launch on -- but the checks come first
    none = dict(v=None, y=None, entropy=None, grad=None, ret=None, discount=None)
    for A in ACTIONS:
        assert _soft(L, A=A, **none) == 0 and _soft(L, A=A, q1=None, q2=None, alpha=None, bad=None, **none) == 0
    _err(L, _soft(L, B=0, **none), -1, b"B must be >= 1")
    _err(L, _soft(L, A=4, **none), -3, b"num_actions must be")
    _err(L, _soft(L, scale=float("nan"), **none), -1, b"scale must be finite")


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------------
def test_soft_value_checks_its_arguments_before_it_touches_a_device():
    import torch
    from snac_amd import SoftValue

    for bad in (dict(num_actions=4), dict(num_actions=True), dict(num_actions="5"), dict(num_actions=5.0), dict(device="cpu"), dict(device=None)):
        with pytest.raises(ValueError):
            SoftValue(**dict(dict(num_actions=5, device="cuda:0"), **bad))
    sv = SoftValue(5, device="cuda:0")
    assert sv.num_actions == 5 and sv.device == torch.device("cuda:0") and sv.env is None
    l, v = torch.zeros(4, 5), torch.zeros(4)
    with pytest.raises(ValueError, match=r"logits must have shape \(B, 5\), got \(4, 3\)"):
        sv.entropy(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="logits must have shape"):
        sv.entropy(torch.zeros(20))
    with pytest.raises(ValueError, match="logits must have shape"):
        sv.value(torch.zeros(0, 5), torch.zeros(0, 5))
    with pytest.raises(ValueError, match="logits must be a contiguous torch.float32 tensor"):
        sv.entropy(l.double())
    with pytest.raises(ValueError, match="logits must be a contiguous torch.float32 tensor"):
        sv.policy_loss(torch.zeros(4, 10)[:, ::2], l, l, 0.2)
    with pytest.raises(ValueError, match="logits must be a contiguous torch.float32 tensor"):
        sv.entropy(l.numpy())
    with pytest.raises(ValueError, match="logits must be on cuda:0"):
        sv.entropy(l)
    with pytest.raises(ValueError, match="logits must be on cuda:0"):
        sv.target(l, l, l, 0.2, v, v)
    with pytest.raises(ValueError, match="logits must be on cuda:0"):
        sv.policy_loss(l.requires_grad_(), l, None, 0.2)


# ---- the kernel's code on the host -------------------------------------------------------------------------------------------------------
def test_the_kernels_per_sample_function_compiled_for_the_host_equals_the_rule_byte_for_byte(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = str(tmp_path / "soft_host.so")
    cmd = [cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", _lib.CSRC, os.path.join(helpers.TESTS, "native", "soft_host.cpp"), "-o", so]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    fn = C.CDLL(so).soft_host
    fn.restype, fn.argtypes = C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_double] + [C.c_void_p] * 4
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rows = 0
    for A in ACTIONS:
        B = len(SORTS) * 640                                         # 13 440 rows per A: more than 40 000 in all
        c = make_case(np.random.default_rng(50 + A), B, A, shift=A)
        rows += B
        for alpha, two, want_y, scale in ((0.2, True, True, 1.0), (0.0, False, True, 1.0 / B), (1.0, True, False, 3.0), (np.nan, True, True, 1.0)):
            want = _rule(c, alpha, two, want_y, scale)
            got = dict(v=np.full(B, 7, np.float32), y=np.full(B, 7, np.float32) if want_y else None, entropy=np.full(B, 7, np.float32),
                       grad=np.full((B, A), 7, np.float32))
            al = np.array([alpha], np.float32)
            bad = fn(B, A, vp(c["logits"]), vp(c["q1"]), vp(c["q2"]) if two else None, vp(al), vp(c["ret"]) if want_y else None,
                     vp(c["discount"]) if want_y else None, scale, vp(got["v"]), vp(got["y"]), vp(got["entropy"]), vp(got["grad"]))
            assert bad == want["bad_rows"], (A, alpha, bad, want["bad_rows"])
            for k, g in got.items():
                if g is not None:
                    _same(g, want[k], (A, alpha, two, want_y, k))
        h = np.full(B, 7, np.float32)                                # the entropy alone: q1, q2 and alpha are not read
        assert fn(B, A, vp(c["logits"]), None, None, None, None, None, 1.0, None, None, vp(h), None) == bad_rows_of(B, A, want_y=False)
        _same(h, soft_rule(c["logits"])["entropy"], (A, "entropy alone"))
    assert rows >= 40000
