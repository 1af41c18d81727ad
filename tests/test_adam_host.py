"""Host: the rule of include/snac_hip.h, "Optimiser step of the device network", restated in numpy (adam_rule, lerp_rule), independently
of the kernels (tests/test_gpu_adam.py compares them byte for byte): the sum of squares by the xor butterfly per 64 values and the second
stage over the partials, the clip, then Adam and the target per parameter, one ufunc per float64 operation.  Then the inputs the GPU tests
run on (make_adam_case, order_case, subnormal_case, bad_case), with what they are for asserted here: that the stated order of the sum can
be told from a sequential sum and from another pairwise tree, that the clip cases lie on both sides of max_norm, that the subnormal case
stores a float32 subnormal and that a bad step writes nothing.  The rule against float64 torch.optim.Adam with clip_grad_norm_ within a
derived bound, both entry points' argument checks -- each failing call fails its checks first, so the placeholder pointers are never
dereferenced -- and DeviceAdam's refusals before it touches a device.  Last, the code the kernels run (snac_amd/csrc/adam_rule.h) is
compiled for the host with the system compiler and compared with adam_rule byte for byte, and the same source runs once as a program
under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os

import numpy as np
import pytest

from cabi_checks import PH, _err_code as _err, _net
import helpers
from hostcode import _vp, load_shared, run_sanitized
from snac_amd import _lib
from specmath import butterfly
from test_mlp_backward_host import hostless_mlp, num_params

F32, F64 = np.float32, np.float64
U24, U53 = 2.0 ** -24, 2.0 ** -53
# the networks of the GPU tests, chosen by P: 2; 32, under one wave; 3718, W = 59, the last wave partly filled; segment boundaries inside
# waves and a layer of one unit; 7878, W = 124 > 64: stage two's lanes add two partials; 196 102: every block of a large grid redoes stage two
ADAM_NETS = ((1, 1), (7, 4), (51, 64, 6), (51, 65, 1, 9), (51, 64, 64, 6), (502, 256, 256, 6))
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
CLIPS = ("off", "clipped", "loose")
TAUS = (None, 0.005, 1.0)


# ---- the rule, in numpy: every ufunc call below is one float64 operation, rounded on its own ----------------------------------------------
def sumsq_rule(g):
    """(ss, partials float64 [W]) of the float32 gradient g [P] in the stated order."""
    P = len(g)
    W = -(-P // 64)
    with np.errstate(all="ignore"):
        g64 = np.zeros(W * 64)
        g64[:P] = g.astype(F64)
        partials = butterfly((g64 * g64).reshape(W, 64))[:, 0].copy()     # the product of two float32 is exact
        s = np.zeros(64)
        for w0 in range(0, W, 64):
            part = partials[w0:w0 + 64]
            s[:len(part)] = s[:len(part)] + part                     # lane j: partials[j], partials[j + 64], .. ascending
        return butterfly(s)[0], partials


def coef_rule(ss, max_norm):
    with np.errstate(all="ignore"):
        if max_norm == 0:
            return F64(1.0)
        c = F64(max_norm) / (np.sqrt(F64(ss)) + F64(1e-6))
        return c if c < 1.0 else F64(1.0)


def lerp_rule(tgt, theta, tau):
    """The target's rule for float32 arrays: tau == 1.0 copies the bits."""
    if tau == 1.0:
        return theta.copy()
    with np.errstate(all="ignore"):
        t64 = tgt.astype(F64)
        return (t64 + F64(tau) * (theta.astype(F64) - t64)).astype(F32)


def adam_rule(theta, g, m, v, lr, beta1, beta2, eps, bias1, bias2, max_norm, tgt=None, tau=1.0, ss=None):
    """-> dict(theta, m, v, tgt (None without one), norm_out float64 [2], partials float64 [W], bad, ss): one step on flat float32 arrays
    [P].  ss: another sum of squares to go on from (for the assertion that the order shows in the outputs)."""
    lr, beta1, beta2, eps, bias1, bias2 = (F64(x) for x in (lr, beta1, beta2, eps, bias1, bias2))
    own_ss, partials = sumsq_rule(g)
    ss = own_ss if ss is None else F64(ss)
    with np.errstate(all="ignore"):
        norm = np.sqrt(ss)
        if not np.isfinite(ss):
            return dict(theta=theta.copy(), m=m.copy(), v=v.copy(), tgt=None if tgt is None else tgt.copy(), norm_out=np.array([norm, 0.0]),
                        partials=partials, bad=True, ss=ss)
        coef = coef_rule(ss, max_norm)
        gd = coef * g.astype(F64)
        m1 = (beta1 * m.astype(F64) + (F64(1.0) - beta1) * gd).astype(F32)
        v1 = (beta2 * v.astype(F64) + (F64(1.0) - beta2) * (gd * gd)).astype(F32)
        denom = np.sqrt(v1.astype(F64)) / np.sqrt(bias2) + eps
        theta1 = (theta.astype(F64) - (lr / bias1) * (m1.astype(F64) / denom)).astype(F32)
        tgt1 = None if tgt is None else lerp_rule(tgt, theta1, tau)
    return dict(theta=theta1, m=m1, v=v1, tgt=tgt1, norm_out=np.array([norm, coef]), partials=partials, bad=False, ss=ss)


def step_of(c, **kw):
    return adam_rule(c["theta"], c["g"], c["m"], c["v"], c["lr"], c["beta1"], c["beta2"], c["eps"], c["bias1"], c["bias2"], c["max_norm"],
                     c["tgt"], c["tau"], **kw)


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------------
def split(dims, flat):
    """[(w [d_{l+1}, d_l], b [d_{l+1}])]: the layers' arrays of a flat parameter vector, as contiguous copies."""
    out, at = [], 0
    for l in range(len(dims) - 1):
        K, N = dims[l], dims[l + 1]
        out.append((flat[at:at + N * K].reshape(N, K).copy(), flat[at + N * K:at + N * K + N].copy()))
        at += N * (K + 1)
    return out


def flatten(layers):
    return np.concatenate([np.concatenate([w.ravel(), b]) for w, b in layers])


def biases_of(t, beta1, beta2):
    """bias1 = 1 - beta1^t and bias2 = 1 - beta2^t as DeviceAdam.step computes them: python floats."""
    return 1.0 - float(beta1) ** t, 1.0 - float(beta2) ** t


def make_adam_case(rng, dims, t=1, clip="off", tau=None, scale=1.0):
    """One step's inputs on flat float32 arrays.  t == 1: zero moments; else random m and v >= 0.  clip: "off" (max_norm 0), "clipped"
    (max_norm a quarter of the gradient's norm) or "loose" (four times it) -- from the gradient alone, not from the rule.  tau: None (no
    target) or the target's tau."""
    dims = tuple(dims)
    P = num_params(dims)
    theta = (rng.normal(size=P) / 8).astype(F32)
    g = (scale * rng.normal(size=P)).astype(F32)
    if t == 1:
        m, v = np.zeros(P, F32), np.zeros(P, F32)
    else:
        m, v = (0.1 * scale * rng.normal(size=P)).astype(F32), ((0.3 * scale * rng.normal(size=P)) ** 2).astype(F32)
    norm = float(np.sqrt((g.astype(F64) ** 2).sum()))
    max_norm = {"off": 0.0, "clipped": norm / 4, "loose": norm * 4}[clip]
    bias1, bias2 = biases_of(t, HYPER["beta1"], HYPER["beta2"])
    tgt = None if tau is None else (rng.normal(size=P) / 8).astype(F32)
    return dict(HYPER, dims=dims, P=P, theta=theta, g=g, m=m, v=v, t=t, bias1=bias1, bias2=bias2, max_norm=max_norm, clip=clip, tgt=tgt,
                tau=1.0 if tau is None else tau)


def adam_seed(dims, t, clip, tau):
    return 4100 + 1000 * sum(dims) + 10 * t + CLIPS.index(clip) + 3 * TAUS.index(tau)


ORDER_DIMS = (12, 64)                                                # P = 832: thirteen waves, all full
ORDER_BIG_AT = 0                                                     # lane 0 of wave 0


def order_case(clip):
    """One value 2^30 among 831 values 1.0.  Its square 2^60 has an ulp of 256 in float64: ones that reach it a few at a time are lost,
    ones that reach it as a sum of more than 128 are not, so the association of the sum shows in ss.  In the stated order the wave's own
    63 ones are lost, and of the other twelve waves' 64s the butterfly of stage two brings 64, 128, 192 and 384 to the lane of 2^60:
    ss = 2^60 + 512, whose root is one ulp above 2^30; a chain in index order loses every one, and the tree of halves of the index range keeps 768."""
    rng = np.random.default_rng(17)
    c = make_adam_case(rng, ORDER_DIMS, t=7, clip="off", tau=0.005)
    c["g"] = np.ones(c["P"], F32)
    c["g"][ORDER_BIG_AT] = 2.0 ** 30
    c["max_norm"] = {"off": 0.0, "clipped": 0.5, "loose": 2.0 ** 31}[clip]
    return dict(c, clip=clip)


def sequential_ss(g):
    return np.cumsum(g.astype(F64) * g.astype(F64))[-1]              # np.add.accumulate: one chain in index order


def pairwise_ss(g):
    """Another pairwise tree: halves of the index range, recursively."""
    u = g.astype(F64) * g.astype(F64)

    def tree(lo, hi):
        if hi - lo == 1:
            return u[lo]
        mid = (lo + hi) // 2
        return tree(lo, mid) + tree(mid, hi)
    return tree(0, len(u))


def subnormal_case():
    """Gradients near 1e-21 from zero moments, no clip: v' = (1 - beta2) g^2 is near 1e-44 .. 1e-43, a float32 subnormal of three to six
    bits."""
    rng = np.random.default_rng(23)
    c = make_adam_case(rng, (51, 64, 6), t=1, clip="off", tau=0.005)
    c["g"] = (1.0e-21 * (1.0 + 4.0 * rng.random(c["P"])) * np.where(rng.random(c["P"]) < 0.5, -1.0, 1.0)).astype(F32)
    c.update(beta2=0.99, bias2=biases_of(1, 0.9, 0.99)[1], eps=0.0)      # eps = 0: the root of the subnormal alone divides, and shows in theta'
    return c


def bad_case():
    """A NaN at the last flat index and an infinity at index 0, with a target and a clip."""
    c = make_adam_case(np.random.default_rng(29), (51, 64, 6), t=7, clip="clipped", tau=0.005)
    c["g"][-1], c["g"][0] = np.nan, np.inf
    return c


# ---- what the inputs are for -------------------------------------------------------------------------------------------------------------
def test_the_stated_order_of_the_sum_shows_in_the_constructed_gradient():
    c = order_case("clipped")
    g = c["g"]
    assert (g == 1.0).sum() == c["P"] - 1 == 831 and g[ORDER_BIG_AT] == 2.0 ** 30
    ss, partials = sumsq_rule(g)
    exact = 2 ** 60 + 831
    seq, pair = sequential_ss(g), pairwise_ss(g)
    assert len({float(ss), float(seq), float(pair)}) == 3, (ss - 2.0 ** 60, seq - 2.0 ** 60, pair - 2.0 ** 60)
    assert all(abs(int(x) - exact) <= 831 for x in (ss, seq, pair))          # each is a sum of these terms, rounded along its own way
    assert ss == 2.0 ** 60 + 512 and seq == 2.0 ** 60 and pair == 2.0 ** 60 + 768
    assert partials[0] == 2.0 ** 60 and (partials[1:] == 64.0).all()          # the wave's own 63 ones reach 2^60 in pieces below 128
    # and the difference reaches an output: going on from the sequential sum gives another norm and another coefficient (a float32
    # parameter does not show one ulp of a float64 coefficient: norm_out is where the GPU test sees stage two's order)
    want, other = step_of(c), step_of(c, ss=seq)
    assert want["norm_out"][0] == 2.0 ** 30 + 2.0 ** -22 and other["norm_out"][0] == 2.0 ** 30 and want["norm_out"][1] != other["norm_out"][1]


def test_the_clip_cases_lie_on_both_sides_of_max_norm():
    seen = set()
    for clip in CLIPS:
        out = step_of(order_case(clip))
        seen.add((clip, bool(out["norm_out"][1] < 1.0)))
    for dims in ADAM_NETS[:4]:
        for clip in CLIPS:
            c = make_adam_case(np.random.default_rng(adam_seed(dims, 7, clip, None)), dims, t=7, clip=clip)
            out = step_of(c)
            coef = out["norm_out"][1]
            assert (coef < 1.0) == (clip == "clipped") and (coef == 1.0) == (clip != "clipped"), (dims, clip, coef)
            assert 0.2 < coef <= 1.0 and not out["bad"]
            seen.add((clip, bool(coef < 1.0)))
    assert seen == {("off", False), ("clipped", True), ("loose", False)}


def test_the_subnormal_case_stores_a_float32_subnormal_and_keeps_it():
    c = subnormal_case()
    out = step_of(c)
    tiny = np.finfo(F32).tiny
    assert ((out["v"] > 0) & (out["v"] < tiny)).all()                # every v' is a subnormal, none was flushed to zero
    assert (out["m"] != 0).all() and (out["theta"] != c["theta"]).any()
    flushed = dict(c, v=np.zeros_like(c["v"]))
    again = adam_rule(out["theta"], c["g"], out["m"], out["v"], c["lr"], c["beta1"], c["beta2"], c["eps"], *biases_of(2, c["beta1"], c["beta2"]), 0.0)
    lost = adam_rule(out["theta"], c["g"], out["m"], flushed["v"], c["lr"], c["beta1"], c["beta2"], c["eps"], *biases_of(2, c["beta1"], c["beta2"]), 0.0)
    assert again["v"].tobytes() != lost["v"].tobytes()               # a second step reads the stored subnormal: flushing it would show


def test_a_bad_step_leaves_every_arrays_bytes_as_they_were():
    c = bad_case()
    out = step_of(c)
    assert out["bad"] and np.isnan(out["norm_out"][0]) and out["norm_out"][1] == 0.0
    for k in ("theta", "m", "v", "tgt"):
        assert out[k].tobytes() == c[k].tobytes(), k
    for g in (np.array([np.inf, 1.0], F32), np.array([1.0, -np.inf], F32), np.array([3.0e38, 3.0e38], F32)):
        ss, _ = sumsq_rule(g)
        assert np.isfinite(ss) == bool(np.isfinite(g).all())         # the square of a finite float32 does not overflow float64


def test_the_second_stage_adds_a_lanes_partials_in_ascending_order():
    """W = 124 > 64: lane j < 60 adds partials[j] and then partials[j + 64]."""
    rng = np.random.default_rng(31)
    g = rng.normal(size=7878).astype(F32)
    ss, partials = sumsq_rule(g)
    assert len(partials) == 124
    s = np.zeros(64)
    s[:64] = partials[:64]
    s[:60] = s[:60] + partials[64:]
    assert butterfly(s)[0] == ss and abs(ss - partials.sum()) <= 200 * U53 * ss


def test_lerp_copies_the_bits_at_tau_one_and_rounds_once_otherwise():
    theta = np.array([np.nan, -0.0, 1.0, 2.0 ** -140, 3.0], F32)
    tgt = np.array([1.0, 1.0, 1.0 + 2.0 ** -23, 0.0, -5.0], F32)
    assert lerp_rule(tgt, theta, 1.0).tobytes() == theta.tobytes()
    got = lerp_rule(tgt, theta, 0.005)
    assert np.isnan(got[0]) and got[4] == F32(-5.0 + 0.005 * 8.0) and got[2] == F32(1.0 + 2.0 ** -23)     # one rounding, from float64


# ---- against torch -----------------------------------------------------------------------------------------------------------------------
def torch_reference(c):
    """One step of torch.optim.Adam after clip_grad_norm_ in float64 on the CPU, over the layers' arrays, from the case's float32 state.
    -> the flat float64 parameters."""
    import torch

    layers = split(c["dims"], c["theta"].astype(F64))
    params = [torch.tensor(a, requires_grad=True) for wb in layers for a in wb]
    for p, a in zip(params, [a for wb in split(c["dims"], c["g"].astype(F64)) for a in wb]):
        p.grad = torch.tensor(a)
    opt = torch.optim.Adam(params, lr=c["lr"], betas=(c["beta1"], c["beta2"]), eps=c["eps"])
    if c["t"] > 1:
        ms = [a for wb in split(c["dims"], c["m"].astype(F64)) for a in wb]
        vs = [a for wb in split(c["dims"], c["v"].astype(F64)) for a in wb]
        for p, m, v in zip(params, ms, vs):
            opt.state[p] = dict(step=torch.tensor(float(c["t"] - 1)), exp_avg=torch.tensor(m), exp_avg_sq=torch.tensor(v))
    if c["max_norm"] > 0:
        torch.nn.utils.clip_grad_norm_(params, c["max_norm"])
    opt.step()
    return np.concatenate([p.detach().numpy().ravel() for p in params])


def adam_bound(c):
    """The bound on |theta' of the rule - theta' of float64 torch| per parameter, from the rule (the docstring of the test derives it)."""
    with np.errstate(all="ignore"):
        g, m, v, theta = (c[k].astype(F64) for k in ("g", "m", "v", "theta"))
        P = c["P"]
        norm = np.sqrt((g * g).sum())
        coef = 1.0 if c["max_norm"] == 0 else min(c["max_norm"] / (norm + 1e-6), 1.0)
        gd = coef * g
        m64 = c["beta1"] * m + (1 - c["beta1"]) * gd
        v64 = c["beta2"] * v + (1 - c["beta2"]) * gd * gd
        denom = np.sqrt(v64) / np.sqrt(c["bias2"]) + c["eps"]
        step = c["lr"] / c["bias1"]
        r = np.abs(m64) / denom
        theta64 = theta - step * m64 / denom
        rounded = step * r * (U24 + U24 / 2) * (1 + 2.0 ** -20)
        noise = step * (8 * U53 * (np.abs(m) + np.abs(gd)) / denom + (2 * P + 32) * U53 * 2 * r) + 4 * U53 * (np.abs(theta) + step * r)
        return theta64, U24 * (np.abs(theta64) + rounded + noise) + rounded + noise, m64, v64


def test_one_step_stays_within_the_derived_bound_of_float64_torch_adam():
    """The reference is torch.optim.Adam after clip_grad_norm_ in float64 on the CPU from the same float32 state.  The bound is derived
    from the rule, not fitted to what is seen (which is printed).  In exact arithmetic both sides compute the same step.  The rule differs
    from it by three float32 roundings: m' and v' are stored rounded, each within 2^-24 relative (the case keeps them normal, asserted),
    so sqrt(v') is within 2^-25 and, eps >= 0 only shrinking a relative error, so is denom; the ratio m' / denom is then within
    2^-24 + 2^-25 of the reference's, to first order (the factor 1 + 2^-20 covers the second).  That moves theta' by at most
        (lr / bias1) |m / denom| (2^-24 + 2^-25)
    and the last rounding to float32 adds half an ulp of theta', at most 2^-24 |theta'|.  The float64 operations of both sides add noise:
    the moment m in torch is a lerp, whose error is relative to |m| + |gd| and not to the result (8 x 2^-53 of it, through 1 / denom); the
    two sums of squares differ in order, each within P 2^-53 relative, and the coefficient carries that into gd and into both moments
    (a factor 2 on |m / denom| bounds its effect); a handful of further operations are each within 2^-53 of theta or the move."""
    worst = 0.0
    for dims in ADAM_NETS[:5]:
        for t, clip, scale in ((1, "off", 0.01), (1, "clipped", 10.0), (7, "clipped", 0.01), (7, "loose", 10.0), (7, "off", 1.0)):
            c = make_adam_case(np.random.default_rng(adam_seed(dims, t, clip, None) + 1), dims, t=t, clip=clip, scale=scale)
            out = step_of(c)
            tiny = np.finfo(F32).tiny
            assert (np.abs(out["m"]) >= tiny).all() and (out["v"] >= tiny).all(), "the bound is for normal moments"
            _, err, _, _ = adam_bound(c)
            ref = torch_reference(c)
            ratio = np.abs(out["theta"].astype(F64) - ref) / err
            assert ratio.max() <= 1.0, (dims, t, clip, ratio.max(), int(ratio.argmax()))
            assert (out["theta"] != c["theta"]).mean() > 0.5         # and it is a step: most parameters moved
            worst = max(worst, ratio.max())
    print("largest error / bound against float64 torch Adam: %.3g" % worst)


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------
G, M, V = C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20)      # distinct aligned placeholders: never dereferenced


def _tgt(dims=(51, 64, 6), **kw):
    L = len(dims) - 1
    kw.setdefault("w", [(5 << 20) + 4096 * l for l in range(L)])
    kw.setdefault("b", [(6 << 20) + 4096 * l for l in range(L)])
    return _net(dims, **kw)


def _step(L, net=None, grad=G, m=M, v=V, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, bias1=0.1, bias2=0.001, max_norm=0.5, target=None, tau=1.0,
          norm_out=PH, partials=PH, bad=PH):
    return L.snac_mlp_adam_step(C.byref(net) if net is not None else None, grad, m, v, lr, beta1, beta2, eps, bias1, bias2, max_norm,
                                C.byref(target) if target is not None else None, tau, norm_out, partials, bad, None)


def _lerp(L, target=None, net=None, tau=1.0):
    return L.snac_mlp_lerp(C.byref(target) if target is not None else None, C.byref(net) if net is not None else None, tau, None)


def test_the_library_exports_the_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    vp, net, d = C.c_void_p, C.POINTER(_lib.Mlp), C.c_double
    P = _lib.PROTOTYPES
    assert P["snac_mlp_adam_step"] == (C.c_int, [net, vp, vp, vp, d, d, d, d, d, d, d, net, d, vp, vp, vp, vp])
    assert P["snac_mlp_lerp"] == (C.c_int, [net, net, d, vp])
    assert all(n in _lib.EXPORTS for n in ("snac_mlp_adam_step", "snac_mlp_lerp"))


def _network_refusals(L, call):
    """The network's checks, as in snac_mlp_forward; call(net) makes the call with every other argument in order."""
    _err(L, call(None), -1, b"null net")
    for layers in (0, -1, 5):
        _err(L, call(_net(layers=layers)), -1, b"layers must be 1 .. 4")
    for d0 in (0, -1, 513):
        _err(L, call(_net((d0, 64, 6))), -1, b"dim[0]")
    for hidden in (0, 257, -4):
        _err(L, call(_net((51, hidden, 6))), -1, b"a hidden width must be 1 .. 256")
    for last in (0, 65, -1):
        _err(L, call(_net((51, 64, last))), -1, b"dim[layers]")
    _err(L, call(_net(w=[1 << 20, 0])), -1, b"null weights / bias")
    _err(L, call(_net(b=[0, 1 << 20])), -1, b"null weights / bias")
    _err(L, call(_net(w=[(1 << 20) + 2, 1 << 20])), -1, b"4-byte aligned")
    _err(L, call(_net(b=[1 << 20, (1 << 20) + 1])), -1, b"4-byte aligned")


def _target_refusals(L, call):
    """The target's checks; call(target, tau) makes the call with the network _net() and every other argument in order."""
    _err(L, call(_tgt(layers=1), 1.0), -1, b"the network's layers")
    _err(L, call(_tgt((51, 64, 64, 6)), 1.0), -1, b"the network's layers")
    for dims in ((50, 64, 6), (51, 63, 6), (51, 64, 5)):
        _err(L, call(_tgt(dims), 1.0), -1, b"the network's dims")
    _err(L, call(_tgt(w=[5 << 20, 0]), 1.0), -1, b"null weights / bias of a layer of the target")
    _err(L, call(_tgt(b=[0, 6 << 20]), 1.0), -1, b"null weights / bias of a layer of the target")
    _err(L, call(_tgt(w=[(5 << 20) + 2, 5 << 20]), 1.0), -1, b"the target's weights and biases must be 4-byte aligned")
    _err(L, call(_tgt(b=[6 << 20, (6 << 20) + 1]), 1.0), -1, b"the target's weights and biases must be 4-byte aligned")
    _err(L, call(_tgt(w=[1 << 20, (5 << 20) + 4096]), 1.0), -1, b"shares an array")       # _net()'s placeholder
    _err(L, call(_tgt(b=[6 << 20, 1 << 20]), 1.0), -1, b"shares an array")
    _err(L, call(_net(), 1.0), -1, b"shares an array")
    for tau in (0.0, -0.5, 1.0 + 2.0 ** -52, 2.0, float("nan"), float("inf")):
        _err(L, call(_tgt(), tau), -1, b"tau must be in (0, 1]")


def test_adam_step_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    odd4, odd8 = C.c_void_p((1 << 20) + 2), C.c_void_p((1 << 20) + 4)
    nan, inf = float("nan"), float("inf")
    ok = _net()
    _network_refusals(L, lambda net: _step(L, net))
    for k in ("grad", "m", "v"):
        _err(L, _step(L, ok, **{k: None}), -1, b"null grad / m / v")
        _err(L, _step(L, ok, **{k: odd4}), -1, b"grad, m and v must be 4-byte aligned")
    for kw in (dict(grad=M), dict(grad=V), dict(m=V), dict(m=G), dict(v=G), dict(v=M)):
        _err(L, _step(L, ok, **kw), -1, b"grad, m and v must be distinct")
    _err(L, _step(L, ok, partials=None), -1, b"null partials")
    _err(L, _step(L, ok, partials=odd8), -1, b"partials must be 8-byte aligned")
    _err(L, _step(L, ok, norm_out=odd8), -1, b"norm_out must be 8-byte aligned")
    _err(L, _step(L, ok, bad=odd4), -1, b"bad_steps must be 4-byte aligned")
    for bad in (-1e-3, nan, inf, -inf):
        _err(L, _step(L, ok, lr=bad), -1, b"lr must be finite and >= 0")
        _err(L, _step(L, ok, eps=bad), -1, b"eps must be finite and >= 0")
        _err(L, _step(L, ok, max_norm=bad), -1, b"max_norm must be finite and >= 0")
    for bad in (-0.1, 1.0, 1.5, nan, inf):
        _err(L, _step(L, ok, beta1=bad), -1, b"beta1 must be in [0, 1)")
        _err(L, _step(L, ok, beta2=bad), -1, b"beta2 must be in [0, 1)")
    for bad in (0.0, -0.1, 1.0 + 2.0 ** -52, nan, inf):
        _err(L, _step(L, ok, bias1=bad), -1, b"bias1 must be in (0, 1]")
        _err(L, _step(L, ok, bias2=bad), -1, b"bias2 must be in (0, 1]")
    _target_refusals(L, lambda target, tau: _step(L, ok, target=target, tau=tau))
    # the values at the edges of the ranges pass those checks: the call then fails a later one
    _err(L, _step(L, ok, lr=0.0, eps=0.0, beta1=0.0, beta2=0.0, bias1=1.0, bias2=1.0, max_norm=0.0, norm_out=None, bad=None, target=_tgt(), tau=0.0),
         -1, b"tau must be in (0, 1]")


def test_lerp_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _network_refusals(L, lambda net: _lerp(L, _tgt(), net))
    _err(L, _lerp(L, None, _net()), -1, b"null target")
    _target_refusals(L, lambda target, tau: _lerp(L, target, _net(), tau))


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------------
def test_device_adam_refuses_before_it_touches_a_device():
    import torch
    from snac_amd import DeviceAdam

    dims = (51, 64, 6)
    mlp, other = hostless_mlp(dims), hostless_mlp(dims)
    P = num_params(dims)
    with pytest.raises(ValueError, match="mlp must be a DeviceMLP"):
        DeviceAdam(torch.nn.Linear(3, 4))
    with pytest.raises(ValueError, match="target must be a DeviceMLP or None"):
        DeviceAdam(mlp, target=torch.nn.Linear(3, 4))
    with pytest.raises(ValueError, match="the target's dims"):
        DeviceAdam(mlp, target=hostless_mlp((51, 65, 6)))
    with pytest.raises(ValueError, match="shares a parameter"):
        DeviceAdam(mlp, target=mlp)
    shared = hostless_mlp(dims)
    shared._params[1] = (shared._params[1][0], mlp._params[1][1])
    with pytest.raises(ValueError, match="shares a parameter"):
        DeviceAdam(mlp, target=shared)
    for bad in (-1e-3, float("nan"), float("inf"), "1e-3", None, True):
        with pytest.raises(ValueError, match="lr must be a finite number >= 0"):
            DeviceAdam(mlp, lr=bad)
        with pytest.raises(ValueError, match="eps must be a finite number >= 0"):
            DeviceAdam(mlp, eps=bad)
    for bad in ((0.9,), (0.9, 1.0), (-0.1, 0.999), (1.0, 0.5), 0.9, (0.9, float("nan")), ("a", "b")):
        with pytest.raises(ValueError, match="betas must be two numbers in"):
            DeviceAdam(mlp, betas=bad)
    for bad in (-0.5, float("nan"), float("inf"), "0.5"):
        with pytest.raises(ValueError, match="max_norm must be None or a finite number >= 0"):
            DeviceAdam(mlp, max_norm=bad)
    for bad in (0.0, -1.0, 1.5, float("nan"), None):
        with pytest.raises(ValueError, match=r"tau must be in \(0, 1\]"):
            DeviceAdam(mlp, target=other, tau=bad)
    opt = DeviceAdam(mlp, lr=3e-4, betas=(0.5, 0.75), max_norm=0.5, target=other, tau=0.005)
    assert (opt.lr, opt.betas, opt.eps, opt.max_norm, opt.tau, opt.t) == (3e-4, (0.5, 0.75), 1e-8, 0.5, 0.005, 0) and opt.device == mlp.device
    assert DeviceAdam(mlp).max_norm == 0.0 and DeviceAdam(mlp).target is None
    for bad in (torch.zeros(P + 1), torch.zeros(P, dtype=torch.float64), torch.zeros(2 * P)[::2], torch.zeros(1, P), [0.0] * P, None):
        with pytest.raises(ValueError, match=r"flat must be a contiguous torch.float32 tensor of shape \(%d,\)" % P):
            opt.step(bad)
    with pytest.raises(ValueError, match="flat must be on cuda:0"):
        opt.step(torch.zeros(P))                                     # everything else is in order: the gradient is on the host
    opt.lr = -1.0
    with pytest.raises(ValueError, match="lr must be a finite number >= 0"):
        opt.step(torch.zeros(P))
    assert opt.t == 0                                                # a refused call is no step
    with pytest.raises(ValueError, match="sync_target needs a target"):
        DeviceAdam(mlp).sync_target()
    for bad in (0.0, 2.0, float("nan")):
        with pytest.raises(ValueError, match=r"tau must be in \(0, 1\]"):
            opt.sync_target(bad)
    for bad, words in (({}, "must hold t, m and v"), (None, "must hold t, m and v"), (dict(t=-1, m=torch.zeros(P), v=torch.zeros(P)), "t must be an integer"),
                       (dict(t=1.5, m=torch.zeros(P), v=torch.zeros(P)), "t must be an integer"),
                       (dict(t=1, m=torch.zeros(P + 1), v=torch.zeros(P)), "m must be a torch.float32 tensor"),
                       (dict(t=1, m=torch.zeros(P), v=torch.zeros(P, dtype=torch.float64)), "v must be a torch.float32 tensor")):
        with pytest.raises(ValueError, match=words):
            opt.load_state_dict(bad)


# ---- the kernels' code on the host -------------------------------------------------------------------------------------------------------
HOST_SRC = os.path.join(helpers.TESTS, "native", "adam_host.cpp")
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", _lib.CSRC, HOST_SRC]
MAIN_SIZES, MAIN_RUNS = 11, 2                                        # adam_host.cpp's main: sizes x (without, with a target)


def _host_fn(tmp_path):
    lib = load_shared(tmp_path, "adam_host", ["-O2", "-fPIC", "-shared"] + HOST_FLAGS, timeout=600)
    vp, d = C.c_void_p, C.c_double
    lib.adam_host.restype, lib.adam_host.argtypes = C.c_int, [C.c_int64, vp, vp, vp, vp, d, d, d, d, d, d, d, vp, d, vp, vp]
    lib.lerp_host.restype, lib.lerp_host.argtypes = C.c_int, [C.c_int64, vp, vp, d]
    return lib


def _run_host(lib, c, norm=True):
    theta, m, v = c["theta"].copy(), c["m"].copy(), c["v"].copy()
    tgt = None if c["tgt"] is None else c["tgt"].copy()
    W = -(-c["P"] // 64)
    partials, norm_out = np.full(W, -7.0), np.full(2, -7.0)
    rc = lib.adam_host(c["P"], _vp(theta), _vp(c["g"]), _vp(m), _vp(v), c["lr"], c["beta1"], c["beta2"], c["eps"], c["bias1"], c["bias2"], c["max_norm"],
                       _vp(tgt), c["tau"], _vp(norm_out) if norm else None, _vp(partials))
    return rc, dict(theta=theta, m=m, v=v, tgt=tgt, norm_out=norm_out, partials=partials)


def same_step(got, want, what):
    """Byte for byte; norm_out as values where the norm is a NaN (any NaN is the rule's NaN)."""
    for k in ("theta", "m", "v", "tgt", "partials"):
        if want[k] is None:
            assert got[k] is None, (what, k)
            continue
        nan = np.isnan(want[k])
        assert np.array_equal(np.isnan(got[k]), nan), (what, k, "NaNs")
        assert np.where(nan, 0, got[k]).astype(want[k].dtype).tobytes() == np.where(nan, 0, want[k]).astype(want[k].dtype).tobytes(), (
            what, k, np.nonzero(~nan & (got[k] != want[k]))[0][:8])
    assert np.array_equal(got["norm_out"], want["norm_out"], equal_nan=True), (what, got["norm_out"], want["norm_out"])


def test_the_kernels_code_compiled_for_the_host_equals_the_rule_byte_for_byte(tmp_path):
    lib = _host_fn(tmp_path)
    cases = [(("order", clip), order_case(clip)) for clip in CLIPS] + [("subnormal", subnormal_case()), ("bad", bad_case())]
    for dims in ADAM_NETS[:5]:
        for t, clip, tau in ((1, "off", None), (7, "clipped", 0.005), (7, "loose", 1.0), (1, "clipped", 1.0), (7, "off", 0.005)):
            cases.append(((dims, t, clip, tau), make_adam_case(np.random.default_rng(adam_seed(dims, t, clip, tau)), dims, t=t, clip=clip, tau=tau)))
    for what, c in cases:
        want = step_of(c)
        rc, got = _run_host(lib, c)
        assert rc == int(want["bad"]), what
        same_step(got, want, what)
        rc, got = _run_host(lib, c, norm=False)                      # norm_out NULL: the same step
        assert rc == int(want["bad"]) and (got["norm_out"] == -7.0).all() and got["theta"].tobytes() == want["theta"].tobytes()
    for tau in TAUS[1:]:
        c = cases[-1][1]
        tgt = c["tgt"].copy()
        assert lib.lerp_host(c["P"], _vp(tgt), _vp(c["theta"]), tau) == 0
        assert tgt.tobytes() == lerp_rule(c["tgt"], c["theta"], tau).tobytes()
    assert lib.adam_host(0, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, 0.0, None, 1.0, None, None) == -1


def test_the_kernels_code_runs_clean_under_the_host_sanitizers(tmp_path):
    """A stand-alone program (adam_host.cpp with its main), not code loaded into python."""
    r = run_sanitized(tmp_path, "adam_host_main", ["-DADAM_HOST_MAIN"] + HOST_FLAGS, probe_timeout=300, build_timeout=600, run_timeout=300)
    assert r.stdout.count(", off 0") == MAIN_SIZES * MAIN_RUNS and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
