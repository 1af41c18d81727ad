"""GPU: snac_ppo_loss, PPOLoss and examples/ppo_batched.py with device_loss.

The kernels through the C ABI on the generated inputs of tests/test_ppo_loss_host.py (make_case: both signs of the advantage with the
ratio below, inside and above the clip interval, log-ratios beyond +-20, masked and far-away logits, the action on a masked logit and
outside [0, A), NaNs and infinities in every float input, the value clipped and not, advantages of magnitudes 1 and 1e3; that they
contain every sort, and that the stated order of the sums differs from a plain sum at B = 4097, is asserted there, on the host), byte
for byte against ppo_rule -- the per-sample outputs, the partials of the first stage, the eight statistics and the mean loss -- at batch
sizes with a ragged wave, a full wave, one lane in a second block, and 4097 and 8193 samples, where a lane of the second kernel adds 2 or
3 partials and the last is a partial wave; the three action counts; the value function clipped and not; every array also taken one float
(the float64 ones: one double) into its allocation.  Every output is carved from a guard arena: nothing lands outside the outputs, the
inputs keep their bytes, a NULL output is not written and the others do not change.  Then repeatability, the Python surface against the
rule and against the float32 torch composition, and the example."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest

from devmem import _equal, _place, _shifts, _vp, short_env
import guard
import helpers
from specmath import _same
from test_ppo_loss_host import ACTIONS, CLIP, CLIP_VFS, ENT_COEF, SORTS, VF_COEF, bad_rows_of, make_case, rule_of

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257, 4095, 4096, 4097, 8193)              # a block is one wave of 64 samples; 64 waves fill the second kernel once
OUTPUTS = ("loss", "grad_logits", "grad_value", "stats", "mean_loss", "bad_rows")
INPUTS = ("logits", "action", "logp", "adv", "value", "value_old", "ret")


def _call(case, clip_vf, want=OUTPUTS, offset=False, scale=1.0):
    """One snac_ppo_loss call with its outputs in a guard arena -> dict of numpy arrays (None where not asked for), and the partials."""
    import torch
    from snac_amd import _lib

    L, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    B, A = case["logits"].shape
    W = (B + 63) // 64
    ins = {k: _place(case[k], offset, dev) for k in INPUTS}
    before = {k: flat.clone() for k, (flat, _) in ins.items()}
    arena = guard.Arena(B * (4 * A + 8) + W * 64 + 80 + 9 * (guard.BAND + 1024), dev)
    off4, off8 = (4, 8) if offset else (0, 0)
    out = dict(loss=arena.carve((B,), torch.float32, offset=off4, name="loss"),
               grad_logits=arena.carve((B, A), torch.float32, offset=off4, name="grad_logits"),
               grad_value=arena.carve((B,), torch.float32, offset=off4, name="grad_value"),
               stats=arena.carve((8,), torch.float64, offset=off8, name="stats"),
               mean_loss=arena.carve((1,), torch.float32, offset=off4, name="mean_loss"),
               partials=arena.carve((W, 8), torch.float64, offset=off8, name="partials"),
               bad_rows=arena.carve((1,), torch.int32, name="bad_rows"))
    if "bad_rows" in want:
        out["bad_rows"].zero_()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = {k: _vp(view) for k, (_, view) in ins.items()}
    o = {k: _vp(out[k]) if k in want else None for k in OUTPUTS}
    _lib.check(L.snac_ppo_loss(B, A, p["logits"], p["action"], p["logp"], p["adv"], p["value"], p["value_old"] if clip_vf >= 0 else None, p["ret"],
                               CLIP, clip_vf, VF_COEF, ENT_COEF, scale, o["loss"], o["grad_logits"], o["grad_value"], o["stats"], o["mean_loss"],
                               _vp(out["partials"]), o["bad_rows"], stream))
    if want:
        assert L.snac_last_kernel() == b"k_ppo_loss"
    arena.check()
    for k in out:
        if k not in want and not (k == "partials" and "stats" in want):
            guard.view_untouched(out[k], k + " (NULL in the call)")  # without stats nothing is reduced: the partials stay as they were
    for k, (flat, _) in ins.items():
        assert torch.equal(flat.view(torch.uint8), before[k].view(torch.uint8)), k + " was written"      # bytes: the rows hold NaNs
    got = {k: (t.cpu().numpy() if k in want else None) for k, t in out.items() if k != "partials"}
    got["partials"] = out["partials"].cpu().numpy() if "stats" in want else None
    return got


# ---- the kernels against the rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("A", ACTIONS)
def test_the_kernels_equal_the_rule_byte_for_byte_and_write_nothing_else(A, B):
    for shift in _shifts(B, SORTS):
        case = make_case(np.random.default_rng(100 * A + B + shift), B, A, shift)
        for clip_vf in CLIP_VFS:
            want = rule_of(case, clip_vf, 1.0 / B)
            assert want["bad_rows"] == bad_rows_of(B, shift, clip_vf >= 0)
            first = None
            for offset in (False, True):                             # both placements; and two runs give the same bytes
                got = _call(case, clip_vf, offset=offset, scale=1.0 / B)
                _equal(got, want, (A, B, shift, clip_vf, offset), OUTPUTS)
                if first is not None:
                    for k, g in got.items():
                        assert g.tobytes() == first[k].tobytes(), (A, B, shift, clip_vf, k)
                first = got


def test_every_subset_of_null_outputs_leaves_them_untouched_and_the_others_unchanged():
    A, B = 5, 257
    case = make_case(np.random.default_rng(11), B, A, 3)
    for clip_vf in CLIP_VFS:
        want = rule_of(case, clip_vf, 1.0 / B)
        calls = 0
        for n in range(len(OUTPUTS) + 1):
            for subset in itertools.combinations(OUTPUTS, n):
                if "mean_loss" in subset and "stats" not in subset:
                    continue                                         # mean_loss is stats[0]: refused, on the host
                calls += 1
                expect = dict(want, bad_rows=want["bad_rows"] if subset else 0)      # nothing asked for: nothing is launched, nothing counted
                _equal(_call(case, clip_vf, want=subset, offset=bool(n % 2), scale=1.0 / B), expect, (clip_vf, subset), OUTPUTS)
        assert calls == 48


def test_the_sums_are_the_stated_tree_not_a_plain_sum():
    """At B = 4097 the mean loss in the stated order differs from the index-order sum (asserted on the host for these inputs): the kernels
    give the stated one."""
    B = 4097
    for A in ACTIONS:
        case = make_case(np.random.default_rng(100 * A + B + B % len(SORTS)), B, A, B % len(SORTS))
        for clip_vf in CLIP_VFS:
            want = rule_of(case, clip_vf)
            plain = np.float64(0.0)
            for t in want["u"][:, 0]:
                plain = plain + t
            got = _call(case, clip_vf, want=("stats",))
            assert got["stats"].tobytes() == want["stats"].tobytes() and got["stats"][0] != plain / np.float64(B)


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", ACTIONS)
def test_ppo_loss_follows_the_rule_and_its_backward_gives_the_closed_form_gradient(A):
    import torch
    from snac_amd import PPOLoss, _lib

    B = 4097
    dev = torch.device("cuda", torch.cuda.current_device())
    case = make_case(np.random.default_rng(A), B, A)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in INPUTS}
    mb = dict(action=t["action"], logp=t["logp"], adv=t["adv"], ret=t["ret"], value=t["value_old"], s=None)      # as RolloutBuffer's: value is the old one
    bad = 0
    for clip_vf in (None, -1.0, 0.1):
        ppo = PPOLoss(A, CLIP, clip_vf, VF_COEF, ENT_COEF, device=dev)
        cv = CLIP if clip_vf is None else clip_vf
        want = rule_of(case, cv, 1.0 / B)
        logits, value = t["logits"].clone().requires_grad_(), t["value"].clone().requires_grad_()
        extra = {k: v.clone().requires_grad_() for k, v in t.items() if k in ("logp", "adv", "ret", "value_old")}
        mean, per = ppo.loss(logits, value, dict(mb, logp=extra["logp"], adv=extra["adv"], ret=extra["ret"], value=extra["value_old"]), want_per_sample=True)
        assert _lib.lib().snac_last_kernel() == b"k_ppo_loss" and mean.requires_grad and not per.requires_grad
        assert mean.shape == () and mean.dtype == torch.float32 and ppo.stats.dtype == torch.float64 and ppo.stats.shape == (8,)
        mean.backward()
        assert all(v.grad is None for v in extra.values())           # constants of the loss
        _same(logits.grad.cpu().numpy(), want["grad_logits"], (A, clip_vf, "logits.grad"))
        _same(value.grad.cpu().numpy(), want["grad_value"], (A, clip_vf, "value.grad"))
        _same(per.cpu().numpy(), want["loss"], (A, clip_vf, "loss per sample"))
        assert mean.detach().cpu().numpy().reshape(1).tobytes() == want["mean_loss"].tobytes()
        assert ppo.stats.cpu().numpy().tobytes() == want["stats"].tobytes()
        st = ppo.stats_dict()
        assert list(st) == ["loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "good", "clamped"]
        assert list(st.values()) == list(want["stats"]) and st["good"] == B - want["bad_rows"]
        # the tuple form, a smaller batch after a larger one (the scratch is kept), and a gradient that is not 1
        n = 65
        small = {k: v[:n].contiguous() for k, v in t.items()}
        l2, v2 = small["logits"].clone().requires_grad_(), small["value"].clone().requires_grad_()
        (3.0 * ppo.loss(l2, v2, (small["action"], small["logp"], small["adv"], small["ret"], small["value_old"]))).backward()
        w2 = rule_of({k: case[k][:n] for k in INPUTS}, cv, 1.0 / n)
        assert l2.grad.cpu().numpy().tobytes() == (np.float32(3.0) * w2["grad_logits"]).tobytes()
        assert v2.grad.cpu().numpy().tobytes() == (np.float32(3.0) * w2["grad_value"]).tobytes()
        bad += want["bad_rows"] + w2["bad_rows"]
        assert int(ppo.bad_rows.cpu()[0]) == want["bad_rows"] + w2["bad_rows"]      # a counter: it adds up over the calls
        with pytest.raises(ValueError, match="action must be a contiguous torch.int64"):
            ppo.loss(logits, value, dict(mb, action=t["action"].int()))
        with pytest.raises(ValueError, match="adv must have shape"):
            ppo.loss(logits, value, dict(mb, adv=t["adv"][:-1]))
        with pytest.raises(ValueError, match="is missing"):
            ppo.loss(logits, value, dict(action=t["action"]))
    assert bad > 0


def test_the_device_mean_is_no_farther_from_float64_than_the_float32_composition():
    """On identical inputs, against examples/ppo_batched.py's composition in float32 on the device: the device mean loss is no farther
    from the same composition in float64 than the composition's own float32 mean is, with 2^-24 |reference| of slack (the one rounding
    of mean_loss to float32).  The rows are the good ones with finite logits and |log ratio| <= 20, which the composition can take."""
    import torch
    from snac_amd import PPOLoss

    dev = torch.device("cuda", torch.cuda.current_device())
    for A in ACTIONS:
        full = make_case(np.random.default_rng(40 + A), 8192 + 4 * len(SORTS), A)
        probe = rule_of(full, -1.0)
        rows = ~probe["bad"] & ~probe["clamped"] & np.isfinite(full["logits"]).all(axis=1)
        case = {k: np.ascontiguousarray(full[k][rows]) for k in INPUTS}
        B = int(rows.sum())
        assert B > 4096

        def composition(dtype, where):
            t = {k: torch.from_numpy(case[k]).to(where) for k in INPUTS}
            f = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in t.items()}
            dist = torch.distributions.Categorical(logits=f["logits"])
            ratio = torch.exp(dist.log_prob(f["action"]) - f["logp"])
            surrogate = torch.min(ratio * f["adv"], torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * f["adv"]).mean()
            value_loss = 0.5 * ((f["value"] - f["ret"]) ** 2).mean()
            return float(-surrogate + VF_COEF * value_loss - ENT_COEF * dist.entropy().mean())
        ref, comp = composition(torch.float64, "cpu"), composition(torch.float32, dev)
        t = {k: torch.from_numpy(case[k]).to(dev) for k in INPUTS}
        ppo = PPOLoss(A, CLIP, -1.0, VF_COEF, ENT_COEF, device=dev)
        mine = float(ppo.loss(t["logits"], t["value"], (t["action"], t["logp"], t["adv"], t["ret"], t["value_old"])))
        print("A %d, B %d: reference %.12g, device %+.3g, float32 composition %+.3g" % (A, B, ref, mine - ref, comp - ref))
        assert abs(mine - ref) <= abs(comp - ref) + 2.0 ** -24 * abs(ref), (A, mine, comp, ref)
        assert int(ppo.bad_rows.cpu()[0]) == 0 and ppo.stats_dict()["good"] == B


def test_ppo_loss_takes_an_envs_actions_device_and_stream():
    import torch
    from snac_amd import PPOLoss

    for kind, A in ((1, 3), (2, 5), (3, 8)):
        env, _ = short_env(kind, 65, True, seed=3)
        ppo = PPOLoss(env)
        assert ppo.num_actions == env.num_actions == A and ppo.device == env.device and ppo.env is env
        case = make_case(np.random.default_rng(kind), 65, A)
        t = {k: torch.from_numpy(case[k]).to(env.device) for k in INPUTS}
        mean = ppo.loss(t["logits"], t["value"], dict(action=t["action"], logp=t["logp"], adv=t["adv"], ret=t["ret"], value=t["value_old"]))
        assert mean.cpu().numpy().reshape(1).tobytes() == rule_of(case, CLIP, 1.0 / 65, vf_coef=0.5, ent_coef=0.01)["mean_loss"].tobytes()
        with pytest.raises(ValueError, match="device is the env's"):
            PPOLoss(env, device=env.device)


# ---- the example -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip_vf", [None, 0.2], ids=["value_unclipped", "value_clipped"])
def test_the_ppo_example_trains_with_the_device_loss(clip_vf):
    spec = importlib.util.spec_from_file_location("ppo_batched", os.path.join(helpers.ROOT, "examples", "ppo_batched.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    info = {}
    losses, returns = mod.run(envs=256, iterations=2, horizon=8, epochs=2, batch=512, device_loss=True, clip_vf=clip_vf, info=info, log=lambda line: None)
    assert len(losses) == 2 * 2 * 4 and np.isfinite(losses).all() and len(returns) == 2
    assert info["bad_rows"] == 0 and info["stats"]["good"] == 512 and np.isfinite(list(info["stats"].values())).all()
    with pytest.raises(ValueError, match="clip_vf belongs to device_loss"):
        mod.run(envs=256, iterations=1, clip_vf=0.2, log=lambda line: None)
