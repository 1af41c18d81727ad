"""GPU: snac_search_loss, SearchLoss and examples/alphazero_selfplay.py with device_loss.

The kernel through the C ABI on the generated inputs of tests/test_search_loss_host.py (make_search_case: peaked, flat and equal logits,
finite logits more than 45 below the largest with and without a target on them, masked actions with and without one, one-hot, scaled and
empty targets, negative, -0.0 and non-finite targets, every float input not finite, weights of 0, |value - z| below, at and above
Huber's delta with both signs, magnitudes 1 and 1e3, ties of the largest logits and of the largest targets; that they contain every sort
in its branch, and that the stated order of the sums differs from a plain sum at B = 4097, is asserted there, on the host), byte for byte
against search_rule -- the per-sample outputs, both gradients, the partials of the first stage, the eight statistics and the mean loss --
at batch sizes with a ragged wave, a full wave, one lane in a second block, 64 waves, and 4097 and 8193 samples, where a lane of the
second kernel adds 2 or 3 partials and the last is a partial wave; the three action counts; Huber's and the squared error, with and
without weights; every array also taken one float (the float64 ones: one double) into its allocation.  Every output is carved from a
guard arena: nothing lands outside the outputs, the inputs keep their bytes, a NULL output is not written and the others do not change.
Then repeatability, the Python surface against the rule, the priorities into a PriorityTree, the float32 torch composition, and the
example."""
import ctypes as C

import numpy as np
import pytest

from devmem import _equal, _example, _place, _shifts, _vp, short_env
import guard
from specmath import _same
from test_search_loss_host import ACTIONS, DELTA, INPUTS, SORTS, VF_COEF, bad_rows_of, make_search_case, plain_sum, rule_of

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257, 4095, 4096, 4097, 8193)              # a block is one wave of 64 samples; 64 waves fill the second kernel once
OUTPUTS = ("loss", "priority", "grad_logits", "grad_value", "stats", "mean_loss", "bad_rows")


def _call(case, weighted=True, delta=DELTA, want=OUTPUTS, offset=False, scale=1.0):
    """One snac_search_loss call with its outputs in a guard arena -> dict of numpy arrays (None where not asked for), and the partials."""
    import torch
    from snac_amd import _lib

    L, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    B, A = case["logits"].shape
    W = (B + 63) // 64
    ins = {k: _place(case[k], offset, dev) for k in INPUTS}
    before = {k: flat.clone() for k, (flat, _) in ins.items()}
    arena = guard.Arena(B * (4 * A + 12) + W * 64 + 80 + 10 * (guard.BAND + 1024), dev)
    off4, off8 = (4, 8) if offset else (0, 0)
    out = dict(loss=arena.carve((B,), torch.float32, offset=off4, name="loss"),
               priority=arena.carve((B,), torch.float32, offset=off4, name="priority"),
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
    _lib.check(L.snac_search_loss(B, A, p["logits"], p["value"], p["pi"], p["z"], p["weight"] if weighted else None, VF_COEF, delta, scale, o["loss"],
                                  o["priority"], o["grad_logits"], o["grad_value"], o["stats"], o["mean_loss"], _vp(out["partials"]), o["bad_rows"],
                                  stream))
    if want:
        assert L.snac_last_kernel() == b"k_search_loss"
    arena.check()
    for k in out:
        if k not in want and not (k == "partials" and "stats" in want):
            guard.view_untouched(out[k], k + " (NULL in the call)")  # without stats nothing is reduced: the partials stay as they were
    for k, (flat, _) in ins.items():
        assert torch.equal(flat.view(torch.uint8), before[k].view(torch.uint8)), k + " was written"      # bytes: the rows hold NaNs
    got = {k: (t.cpu().numpy() if k in want else None) for k, t in out.items() if k != "partials"}
    got["partials"] = out["partials"].cpu().numpy() if "stats" in want else None
    return got


# ---- the kernel against the rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("A", ACTIONS)
def test_the_kernel_equals_the_rule_byte_for_byte_and_writes_nothing_else(A, B):
    """Weights and Huber's error at every size; the other three combinations at B = 65 and 4097."""
    combos = [(True, DELTA)]
    if B in (65, 4097):
        combos += [(True, 0.0), (False, DELTA), (False, 0.0)]
    for shift in _shifts(B, SORTS):
        case = make_search_case(np.random.default_rng(100 * A + B + shift), B, A, shift)
        for weighted, delta in combos:
            want = rule_of(case, weighted, delta, 1.0 / B)
            assert want["bad_rows"] == bad_rows_of(B, shift, weighted)
            first = None
            for offset in (False, True):                             # both placements; and two runs give the same bytes
                got = _call(case, weighted, delta, offset=offset, scale=1.0 / B)
                _equal(got, want, (A, B, shift, weighted, delta, offset), OUTPUTS)
                if first is not None:
                    for k, g in got.items():
                        assert g.tobytes() == first[k].tobytes(), (A, B, shift, k)
                first = got


def test_null_outputs_stay_untouched_and_the_others_unchanged():
    A, B = 5, 257
    case = make_search_case(np.random.default_rng(11), B, A, 3)
    subsets = [(), ("priority",), ("bad_rows",), ("grad_logits", "bad_rows"), ("grad_value",), ("stats",), ("stats", "mean_loss"), ("loss", "priority"),
               ("loss", "priority", "grad_logits", "grad_value"), ("priority", "stats", "mean_loss", "bad_rows")] + [tuple(k for k in OUTPUTS if k != o)
                                                                                                                    for o in OUTPUTS if o != "stats"]
    want = rule_of(case, True, DELTA, 1.0 / B)
    for n, subset in enumerate(subsets):
        expect = dict(want, bad_rows=want["bad_rows"] if subset else 0)          # nothing asked for: nothing is launched, nothing counted
        _equal(_call(case, want=subset, offset=bool(n % 2), scale=1.0 / B), expect, subset, OUTPUTS)


def test_the_sums_are_the_stated_tree_not_a_plain_sum():
    """At B = 4097 the mean loss in the stated order differs from the index-order sum (asserted on the host for these inputs): the kernels
    give the stated one."""
    B = 4097
    for A in ACTIONS:
        case = make_search_case(np.random.default_rng(100 * A + B), B, A, B % len(SORTS))
        want = rule_of(case)
        got = _call(case, want=("stats",))
        assert got["stats"].tobytes() == want["stats"].tobytes() and got["stats"][0] != plain_sum(want["u"][:, 0]) / np.float64(B)


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", ACTIONS)
def test_search_loss_follows_the_rule_and_its_backward_gives_the_closed_form_gradients(A):
    import torch
    from snac_amd import SearchLoss, _lib

    B = 4097
    dev = torch.device("cuda", torch.cuda.current_device())
    case = make_search_case(np.random.default_rng(A), B, A)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in INPUTS}
    for huber, weighted, as_dict in ((None, False, True), (DELTA, True, True), (DELTA, True, False)):
        sl = SearchLoss(A, VF_COEF, huber, device=dev)
        delta = 0.0 if huber is None else huber
        want = rule_of(case, weighted, delta, 1.0 / B)
        logits, value = t["logits"].clone().requires_grad_(), t["value"].clone().requires_grad_()
        extra = {k: t[k].clone().requires_grad_() for k in ("pi", "z") + (("weight",) if weighted else ())}
        mb = dict(extra, obs=None, index=None) if as_dict else tuple(extra[k] for k in ("pi", "z", "weight"))
        mean, per, prio = sl.loss(logits, value, mb, want_per_sample=True)
        assert _lib.lib().snac_last_kernel() == b"k_search_loss" and mean.requires_grad and not per.requires_grad and not prio.requires_grad
        assert mean.shape == () and mean.dtype == torch.float32 and sl.stats.dtype == torch.float64 and sl.stats.shape == (8,)
        mean.backward()
        assert all(v.grad is None for v in extra.values())           # constants of the loss
        _same(logits.grad.cpu().numpy(), want["grad_logits"], (A, huber, "logits.grad"))
        _same(value.grad.cpu().numpy(), want["grad_value"], (A, huber, "value.grad"))
        _same(per.cpu().numpy(), want["loss"], (A, huber, "loss per sample"))
        _same(prio.cpu().numpy(), want["priority"], (A, huber, "priority"))
        assert mean.detach().cpu().numpy().reshape(1).tobytes() == want["mean_loss"].tobytes()
        assert sl.stats.cpu().numpy().tobytes() == want["stats"].tobytes()
        st = sl.stats_dict()
        assert list(st) == ["loss", "policy_loss", "value_loss", "entropy", "abs_error", "agreement", "good", "weight"]
        assert list(st.values()) == list(want["stats"]) and st["good"] == B - want["bad_rows"]
        # a smaller batch after a larger one (the scratch is kept), the mean alone, the tuple without weights, a gradient that is not 1
        n = 65
        small = {k: v[:n].contiguous() for k, v in t.items()}
        l2, v2 = small["logits"].clone().requires_grad_(), small["value"].clone().requires_grad_()
        out = sl.loss(l2, v2, (small["pi"], small["z"]))
        assert torch.is_tensor(out) and out.shape == ()
        (3.0 * out).backward()
        w2 = rule_of({k: case[k][:n] for k in INPUTS}, False, delta, 1.0 / n)
        assert l2.grad.cpu().numpy().tobytes() == (np.float32(3.0) * w2["grad_logits"]).tobytes()
        assert v2.grad.cpu().numpy().tobytes() == (np.float32(3.0) * w2["grad_value"]).tobytes()
        assert int(sl.bad_rows.cpu()[0]) == want["bad_rows"] + w2["bad_rows"] > 0        # a counter: it adds up over the calls
        with pytest.raises(ValueError, match="pi must have shape"):
            sl.loss(logits, value, (t["pi"][:-1].contiguous(), t["z"]))
        with pytest.raises(ValueError, match=r"value must have shape \(4097,\)"):
            sl.loss(logits, t["value"][:-1].contiguous(), (t["pi"], t["z"]))
        with pytest.raises(ValueError, match="value must be a contiguous torch.float32"):
            sl.loss(logits, torch.zeros(B, 2, device=dev)[:, 1], (t["pi"], t["z"]))
        with pytest.raises(ValueError, match="weight must have shape"):
            sl.loss(logits, value, dict(pi=t["pi"], z=t["z"], weight=t["weight"][:-1].contiguous()))


def test_search_loss_takes_an_envs_actions_device_and_stream():
    import torch
    from snac_amd import SearchLoss

    for kind, A in ((1, 3), (2, 5), (3, 8)):
        env, _ = short_env(kind, 65, True, seed=3)
        sl = SearchLoss(env, vf_coef=VF_COEF, huber=DELTA)
        assert sl.num_actions == env.num_actions == A and sl.device == env.device and sl.env is env
        case = make_search_case(np.random.default_rng(kind), 65, A)
        t = {k: torch.from_numpy(case[k]).to(env.device) for k in INPUTS}
        mean = sl.loss(t["logits"], t["value"], t)
        assert mean.cpu().numpy().reshape(1).tobytes() == rule_of(case, True, DELTA, 1.0 / 65)["mean_loss"].tobytes()
        with pytest.raises(ValueError, match="device is the env's"):
            SearchLoss(env, device=env.device)


def test_the_priorities_go_into_a_priority_tree_as_they_are():
    """priority from the device and the same values from the host give the same tree."""
    import torch
    from snac_amd import PriorityTree, SearchLoss

    dev = torch.device("cuda", torch.cuda.current_device())
    A, B = 5, 257
    case = make_search_case(np.random.default_rng(5), B, A)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in INPUTS}
    _, _, prio = SearchLoss(A, VF_COEF, DELTA, device=dev).loss(t["logits"], t["value"], t, want_per_sample=True)
    want = rule_of(case, True, DELTA, 1.0 / B)["priority"]
    index = torch.arange(B, dtype=torch.int32, device=dev)
    trees = [PriorityTree(512, device=dev), PriorityTree(512, device=dev)]
    trees[0].update(index, prio)
    trees[1].update(index, torch.from_numpy(want).to(dev))
    w = [tr.weights().view(torch.int32).cpu().numpy() for tr in trees]      # the leaves: rint(priority * 2^16)
    # most sorts have a |value - z| drawn from a continuous distribution (the placed ones share theirs, the bad ones give 0)
    assert w[0].tobytes() == w[1].tobytes() and len(np.unique(w[0][:B])) > B // 4 and not w[0][B:].any()
    assert trees[0].total() == trees[1].total() > 0


def test_the_device_mean_is_no_farther_from_float64_than_the_float32_composition():
    """On identical inputs, against examples/alphazero_selfplay.py's composition in float32 on the device (log_softmax, the product with
    pi, the sums, the squared value error, the weighting, the two means): the device mean loss is no farther from the same composition in
    float64 than the composition's own float32 mean is, with 2^-24 |reference| of slack (the one rounding of mean_loss to float32).  The
    rows are the good ones with finite logits everywhere, which the composition can take."""
    import torch
    from snac_amd import SearchLoss

    dev = torch.device("cuda", torch.cuda.current_device())
    for A in ACTIONS:
        full = make_search_case(np.random.default_rng(40 + A), 8192 + 4 * len(SORTS), A)
        rows = ~rule_of(full, True, 0.0)["bad"] & np.isfinite(full["logits"]).all(axis=1)
        case = {k: np.ascontiguousarray(full[k][rows]) for k in INPUTS}
        B = int(rows.sum())
        assert B > 4096

        def composition(dtype, where):
            b = {k: torch.from_numpy(case[k]).to(where).to(dtype) for k in INPUTS}
            policy_loss = -(b["weight"] * (b["pi"] * torch.log_softmax(b["logits"], 1)).sum(1)).mean()
            value_loss = (b["weight"] * (b["value"] - b["z"]) ** 2).mean()
            return float(policy_loss + value_loss)
        ref, comp = composition(torch.float64, "cpu"), composition(torch.float32, dev)
        t = {k: torch.from_numpy(case[k]).to(dev) for k in INPUTS}
        sl = SearchLoss(A, device=dev)
        mine = float(sl.loss(t["logits"], t["value"], t))
        print("A %d, B %d: reference %.12g, device %+.3g, float32 composition %+.3g" % (A, B, ref, mine - ref, comp - ref))
        assert abs(mine - ref) <= abs(comp - ref) + 2.0 ** -24 * abs(ref), (A, mine, comp, ref)
        assert int(sl.bad_rows.cpu()[0]) == 0 and sl.stats_dict()["good"] == B


# ---- the example -------------------------------------------------------------------------------------------------------------------------
SMALL = dict(envs=16, steps=2, moves=2, iterations=4)


@pytest.mark.parametrize("how", [dict(), dict(prioritized=True), dict(gumbel=4), dict(prioritized=True, per_alpha=0.6, huber=1.0, vf_coef=0.5)],
                         ids=["plain", "prioritized", "gumbel", "prioritized_alpha_huber"])
def test_the_selfplay_example_trains_with_the_device_loss(how):
    import torch

    mod = _example("alphazero_selfplay")
    info = {}
    losses, play = mod.train(device_loss=True, info=info, **SMALL, **how)
    assert len(losses) == 2 and np.isfinite(losses).all() and info["bad_rows"] == 0 and len(play) > 0
    assert info["good"] == 256 and np.isfinite(list(info.values())).all() and info["entropy"] > 0
    if how.get("prioritized"):
        leaves = play.tree.weights().view(torch.int32).cpu().numpy()
        assert len(np.unique(leaves[leaves > 0])) > 8                # 32 to 64 entries, filled with one weight: the updates moved them apart


def test_the_selfplay_example_still_trains_by_default():
    mod = _example("alphazero_selfplay")
    losses, play = mod.train(**SMALL)
    assert len(losses) == 2 and np.isfinite(losses).all() and len(play) > 0
    with pytest.raises(ValueError, match="belong to device_loss"):
        mod.train(huber=1.0, **SMALL)
