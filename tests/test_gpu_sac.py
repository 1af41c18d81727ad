"""GPU: snac_soft_value, SoftValue and examples/sac_batched.py.

The kernel through the C ABI on the generated inputs of tests/test_sac_host.py (make_case: masked and far-away logits, bad logits, NaNs in
q at masked and at live actions, both orders of the critics and ties, bad and special ret / discount; that they contain every sort is
asserted there, on the host), byte for byte against soft_rule, at batch sizes with a ragged wave, a full wave, one lane in the second
block and many blocks, the three action counts, with and without q2, and three temperatures.  Every output is carved from a guard arena:
nothing lands outside the outputs, the inputs keep their bytes, a NULL output is not written and the others do not change; inputs and
outputs are also taken one float into a larger tensor (a base aligned to 4 bytes only).  Where the rule gives a NaN (a q-value that is
not finite at a live action) the kernel must give a NaN too; which NaN is not part of the rule, so those four bytes are not compared.
Then the entropy against env.sample_actions, repeatability, the Python surface and the example."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from devmem import _place_floats, _shifts, _vp, short_env
import guard
import helpers
from test_sac_host import ACTIONS, ALPHAS, SORTS, bad_rows_of, make_case, soft_rule

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257, 1031)                                # a block is one wave of 64 samples
VALUES = ("v", "y", "entropy", "grad")
INPUTS = ("logits", "q1", "q2", "ret", "discount")


def _call(case, alpha, two=True, want=VALUES + ("bad_rows",), offset=False, scale=1.0):
    """One snac_soft_value call with its outputs in a guard arena -> dict of numpy arrays (None where not asked for)."""
    import torch
    from snac_amd import _lib

    L, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    B, A = case["logits"].shape
    ins = {k: _place_floats(case[k], offset, dev) for k in INPUTS}
    ins["alpha"] = _place_floats(np.array([alpha], np.float32), offset, dev)
    before = {k: flat.clone() for k, (flat, _) in ins.items()}
    arena = guard.Arena(B * (4 * A + 12) + 4 + 7 * (guard.BAND + 1024), dev)
    off4 = 4 if offset else 0
    out = dict(v=arena.carve((B,), torch.float32, offset=off4, name="v"), y=arena.carve((B,), torch.float32, offset=off4, name="y"),
               entropy=arena.carve((B,), torch.float32, offset=off4, name="entropy"), grad=arena.carve((B, A), torch.float32, offset=off4, name="grad"),
               bad_rows=arena.carve((1,), torch.int32, name="bad_rows"))
    if "bad_rows" in want:
        out["bad_rows"].zero_()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = {k: _vp(view) for k, (_, view) in ins.items()}
    use_q, want_y = any(k in want for k in ("v", "y", "grad")), "y" in want
    _lib.check(L.snac_soft_value(B, A, p["logits"], p["q1"] if use_q else None, p["q2"] if use_q and two else None, p["alpha"] if use_q else None,
                                 p["ret"] if want_y else None, p["discount"] if want_y else None, scale,
                                 *[_vp(out[k]) if k in want else None for k in VALUES + ("bad_rows",)], stream))
    if any(k in want for k in VALUES):
        assert L.snac_last_kernel() == b"k_soft_value"
    arena.check()
    for k in out:
        if k not in want:
            guard.view_untouched(out[k], k + " (NULL in the call)")
    for k, (flat, _) in ins.items():
        assert torch.equal(flat.view(torch.int32), before[k].view(torch.int32)), k + " was written"      # bytes: the rows hold NaNs
    return {k: (t.cpu().numpy() if k in want else None) for k, t in out.items()}


def _rule(case, alpha, two=True, want=VALUES, scale=1.0):
    use_q, want_y = any(k in want for k in ("v", "y", "grad")), "y" in want
    return soft_rule(case["logits"], case["q1"] if use_q else None, case["q2"] if use_q and two else None, alpha if use_q else None,
                     case["ret"] if want_y else None, case["discount"] if want_y else None, scale)


def _same(got, want, what):
    """Byte for byte, but a NaN of the rule is any NaN."""
    for k in VALUES + ("bad_rows",):
        g, w = got[k], want[k]
        if g is None:
            continue
        if k == "bad_rows":
            assert int(g[0]) == w, (what, k, int(g[0]), w)
            continue
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape, (what, k)
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (what, k, "NaNs")
        g, w = np.where(nan, np.float32(0), g), np.where(nan, np.float32(0), w)
        diff = np.nonzero((g.view(np.uint32).reshape(len(g), -1) != w.view(np.uint32).reshape(len(w), -1)).any(axis=1))[0]
        assert diff.size == 0, (what, k, "first sample that differs", int(diff[0]), g[diff[0]], w[diff[0]])


# ---- the kernel against the rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("A", ACTIONS)
def test_the_kernel_equals_the_rule_byte_for_byte_and_writes_nothing_else(A, B):
    for shift in _shifts(B, SORTS):
        case = make_case(np.random.default_rng(100 * A + B + shift), B, A, shift)
        for n, alpha in enumerate(ALPHAS):
            for two in (True, False):
                offset = bool((n + two) % 2)                         # both placements for every alpha and for both forms
                want = _rule(case, alpha, two, scale=1.0 / B)
                assert want["bad_rows"] == bad_rows_of(B, shift)
                _same(_call(case, alpha, two, offset=offset, scale=1.0 / B), want, (A, B, shift, alpha, two, offset))
    # any subset of the outputs: the ones left out are not written, the others do not change; without y, ret and discount are not read
    # (they are NULL), and the entropy alone reads neither q nor alpha
    for subset in (("v",), ("y",), ("entropy",), ("grad",), ("bad_rows",), ("v", "grad", "entropy"), ("entropy", "bad_rows"), ("y", "bad_rows"), ()):
        want = _rule(case, 0.2, True, subset)
        assert want["bad_rows"] == bad_rows_of(B, shift, want_y="y" in subset)
        if not any(k in subset for k in VALUES):
            want["bad_rows"] = 0                                     # no value output: nothing is launched, nothing is counted
        _same(_call(case, 0.2, True, want=subset, offset=True), want, (A, B, subset))
    for alpha in (float("nan"), float("inf"), -0.5):                 # a bad temperature: every sample of the call
        got = _call(case, alpha)
        assert int(got["bad_rows"][0]) == B and not any(got[k].view(np.uint32).any() for k in VALUES)


def test_the_entropy_is_sample_actions_and_two_runs_give_the_same_bytes():
    import torch

    for kind, A in ((1, 3), (2, 5), (3, 8)):
        B = 1031
        env, _ = short_env(kind, B, True, seed=5)
        case = make_case(np.random.default_rng(kind), B, A)
        first, second = (_call(case, 0.2, offset=bool(j)) for j in range(2))
        for k in first:
            assert first[k].tobytes() == second[k].tobytes(), (A, k)
        _, _, h = env.sample_actions(torch.from_numpy(case["logits"]).to(env.device), want_logp=False, want_entropy=True)
        good = ~soft_rule(case["logits"])["bad"]                     # snac_policy_act draws a bad row as if its scores were 0: log(A), here 0
        assert good.sum() == B - bad_rows_of(B, want_y=False)
        assert _call(case, 0.2, want=("entropy",))["entropy"][good].tobytes() == h.cpu().numpy()[good].tobytes()
        good = ~_rule(case, 0.2)["bad"]                              # with y asked for, a bad ret or discount zeroes the sample's entropy too
        assert good.sum() == B - bad_rows_of(B) and h.cpu().numpy()[good].tobytes() == first["entropy"][good].tobytes()


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", ACTIONS)
def test_soft_value_follows_the_rule_and_its_loss_carries_the_closed_form_gradient(A):
    import torch
    from snac_amd import SoftValue, _lib

    B = 257
    dev = torch.device("cuda", torch.cuda.current_device())
    sv = SoftValue(A, device=dev)
    case = make_case(np.random.default_rng(A), B, A)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in INPUTS}
    alpha = torch.tensor([0.2], dtype=torch.float32, device=dev)
    none = dict(v=None, y=None, entropy=None, grad=None, bad_rows=None)
    _same(dict(none, v=sv.value(t["logits"], t["q1"], t["q2"], alpha).cpu().numpy()), _rule(case, 0.2, want=("v",)), "value")
    _same(dict(none, v=sv.value(t["logits"], t["q1"], alpha=0.2).cpu().numpy()), _rule(case, 0.2, False, want=("v",)), "value, one critic, a number")
    y_out = torch.empty((B,), dtype=torch.float32, device=dev)
    assert sv.target(t["logits"], t["q1"], t["q2"], alpha, t["ret"], t["discount"], out=y_out) is y_out
    _same(dict(none, y=y_out.cpu().numpy()), _rule(case, 0.2, want=("y",)), "target")
    _same(dict(none, entropy=sv.entropy(t["logits"]).cpu().numpy()), _rule(case, 0.2, want=("entropy",)), "entropy")
    assert int(sv.bad_rows.cpu()[0]) == 3 * bad_rows_of(B, want_y=False) + bad_rows_of(B)      # a counter: it adds up over the calls

    # the loss: one launch forward, and logits.grad is the rule's grad with scale 1 / B up to the float32 product by grad_output
    logits = t["logits"].clone().requires_grad_()
    q1, q2 = t["q1"].clone().requires_grad_(), t["q2"].clone().requires_grad_()
    loss, entropy = sv.policy_loss(logits, q1, q2, alpha, want_entropy=True)
    assert _lib.lib().snac_last_kernel() == b"k_soft_value" and loss.requires_grad and not entropy.requires_grad
    one, want = (_rule(case, 0.2, want=("v", "grad", "entropy"), scale=scale) for scale in (1.0, 1.0 / B))      # no y: ret and discount are not read
    _same(dict(none, entropy=entropy.cpu().numpy(), v=(-loss.detach()).cpu().numpy()), one, "policy_loss")
    fine = torch.from_numpy(~one["bad"] & np.isfinite(one["V"])).to(dev)      # the mean of the samples whose loss is a number
    (loss[fine].sum() / B).backward()
    assert q1.grad is None and q2.grad is None                       # constants of this loss
    got, rows = logits.grad.cpu().numpy(), fine.cpu().numpy()
    assert not got[one["bad"]].any()                                 # (a sample whose loss is a NaN keeps its NaN: 0 * NaN)
    product = one["grad"][rows] * np.float32(1.0 / B)                # float32: grad_output times the kernel's grad
    assert got[rows].tobytes() == product.tobytes()
    assert np.abs(got[rows].astype(np.float64) - want["G"][rows]).max() <= 2.0 ** -22 * np.abs(want["G"][rows]).max()      # two float32 roundings

    # against torch autograd on the float32 composition.  The margin below is the composition's own rounding in float32 (its softmax,
    # its products and its backward pass), not the kernel's: the kernel's grad is the float64 rule's, rounded once.
    l32 = t["logits"].clamp(min=-1e4).requires_grad_()              # a masked logit: probability exactly 0 with a finite log, no 0 * inf
    logp = torch.log_softmax(l32, dim=1)
    pi = logp.exp()
    qm = torch.where(t["q2"] < t["q1"], t["q2"], t["q1"])           # the rule's minimum: a NaN in q2 never wins (torch.minimum would carry it)
    terms = pi * (0.2 * logp - torch.where(pi > 0, qm, torch.zeros_like(qm)))
    terms.sum(dim=1)[fine].sum().div(B).backward()
    err = np.abs(l32.grad.cpu().numpy()[rows].astype(np.float64) - got[rows])
    print("A %d: largest |kernel grad - float32 autograd| %.3g, largest |grad| %.3g" % (A, err.max(), np.abs(got[rows]).max()))
    assert err.max() <= 2.0 ** -22 * np.abs(got[rows]).max() + 1e-6

    with pytest.raises(ValueError, match="q1 must have shape"):
        sv.value(t["logits"], t["q1"][:-1])
    with pytest.raises(ValueError, match="ret must have shape"):
        sv.target(t["logits"], t["q1"], t["q2"], alpha, t["ret"][:-1], t["discount"])
    with pytest.raises(ValueError, match="alpha must be a one-element"):
        sv.value(t["logits"], t["q1"], t["q2"], alpha.double())
    with pytest.raises(ValueError, match="alpha must be a one-element"):
        sv.value(t["logits"], t["q1"], t["q2"], float("nan"))
    with pytest.raises(ValueError, match="logits must be on"):
        sv.entropy(t["logits"].cpu())


def test_soft_value_takes_an_envs_actions_device_and_stream():
    import torch
    from snac_amd import SoftValue

    for kind, A in ((1, 3), (2, 5), (3, 8)):
        env, _ = short_env(kind, 65, True, seed=3)
        sv = SoftValue(env)
        assert sv.num_actions == env.num_actions == A and sv.device == env.device and sv.env is env
        case = make_case(np.random.default_rng(kind), 65, A)
        v = sv.value(*(torch.from_numpy(case[k]).to(env.device) for k in ("logits", "q1", "q2")), alpha=1.0)
        _same(dict(v=v.cpu().numpy(), y=None, entropy=None, grad=None, bad_rows=None), _rule(case, 1.0, want=("v",)), kind)
        with pytest.raises(ValueError, match="device is the env's"):
            SoftValue(env, device=env.device)


# ---- the example -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("composition", [False, True], ids=["device", "composition"])
def test_the_sac_example_trains(composition):
    spec = importlib.util.spec_from_file_location("sac_batched", os.path.join(helpers.ROOT, "examples", "sac_batched.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    info = {}
    losses, _ = mod.run(envs=256, ticks=24, batch=256, composition=composition, info=info, log=lambda line: None)
    assert len(losses) == 24 and all(np.isfinite(x).all() for x in losses)
    assert info["bad_rows"] == 0
