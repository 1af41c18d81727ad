"""GPU: snac_td_loss, snac_c51_loss, TDLoss, CategoricalSupport.loss and the examples with device_loss.

The kernels through the C ABI on the generated inputs of tests/test_qloss_host.py (make_case: |td| below, at and above Huber's delta with
both signs, td == 0, ties and NaNs in the choice of the next action, NaNs and infinities at Q-values that are neither taken nor chosen,
actions outside [0, A), every float input not finite, a negative discount, weights of 0, magnitudes 1 and 1e3; that they contain every
sort in its branch, and that the stated order of the sums differs from a plain sum at B = 4097, is asserted there, on the host), byte for
byte against td_rule -- the per-sample outputs, the partials of the first stage, the eight statistics and the mean loss -- at batch
sizes with a ragged wave, a full wave, one lane in a second block, and 4097 and 8193 samples, where a lane of the second kernel adds 2 or
3 partials and the last is a partial wave; the three action counts; the three target modes, Huber's and the squared error, with and
without weights; every array also taken one float (the float64 ones and the actions: one double) into its allocation.  Every output is
carved from a guard arena: nothing lands outside the outputs, the inputs keep their bytes, a NULL output is not written and the others do
not change.  Then repeatability, the Python surface against the rule, the priorities into a PriorityTree, the float32 torch composition,
and the examples.  snac_c51_loss likewise on make_c51_case against c51_loss_rule: a ragged block, a full block, one sample in a second
block, B = 4097 where a lane of the second stage adds two partials; K = 2, 33, 51, 64 and the three action counts."""
import ctypes as C

import numpy as np
import pytest

from devmem import _equal, _example, _place, _shifts, _vp, short_env
import guard
from specmath import _same
from test_qloss_host import (ACTIONS, C51_INPUTS, C51_SORTS, DELTA, INPUTS, MODES, SORTS, bad_rows_of, c51_bad_rows_of, c51_rule_of, make_c51_case, make_case,
                             rule_of)

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257, 4095, 4096, 4097, 8193)              # a block is one wave of 64 samples; 64 waves fill the second kernel once
OUTPUTS = ("loss", "priority", "y_out", "grad_q", "stats", "mean_loss", "bad_rows")


def _call(case, mode="double", weighted=True, delta=DELTA, want=OUTPUTS, offset=False, scale=1.0):
    """One snac_td_loss call with its outputs in a guard arena -> dict of numpy arrays (None where not asked for), and the partials."""
    import torch
    from snac_amd import _lib

    L, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    B, A = case["q"].shape
    W = (B + 63) // 64
    ins = {k: _place(case[k], offset, dev) for k in INPUTS}
    before = {k: flat.clone() for k, (flat, _) in ins.items()}
    arena = guard.Arena(B * (4 * A + 12) + W * 64 + 80 + 10 * (guard.BAND + 1024), dev)
    off4, off8 = (4, 8) if offset else (0, 0)
    out = dict(loss=arena.carve((B,), torch.float32, offset=off4, name="loss"),
               priority=arena.carve((B,), torch.float32, offset=off4, name="priority"),
               y_out=arena.carve((B,), torch.float32, offset=off4, name="y_out"),
               grad_q=arena.carve((B, A), torch.float32, offset=off4, name="grad_q"),
               stats=arena.carve((8,), torch.float64, offset=off8, name="stats"),
               mean_loss=arena.carve((1,), torch.float32, offset=off4, name="mean_loss"),
               partials=arena.carve((W, 8), torch.float64, offset=off8, name="partials"),
               bad_rows=arena.carve((1,), torch.int32, name="bad_rows"))
    if "bad_rows" in want:
        out["bad_rows"].zero_()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = {k: _vp(view) for k, (_, view) in ins.items()}
    y = mode == "y"
    o = {k: _vp(out[k]) if k in want else None for k in OUTPUTS}
    _lib.check(L.snac_td_loss(B, A, p["q"], p["action"], p["y"] if y else None, None if y else p["q_next"], p["q_select"] if mode == "double" else None,
                              None if y else p["ret"], None if y else p["discount"], p["weight"] if weighted else None, delta, scale, o["loss"],
                              o["priority"], o["y_out"], o["grad_q"], o["stats"], o["mean_loss"], _vp(out["partials"]), o["bad_rows"], stream))
    if want:
        assert L.snac_last_kernel() == b"k_td_loss"
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
    """Mode NEXT with q_select, delta = 1 and weights at every size; the other combinations at B = 65 and 4097."""
    combos = [("double", True, DELTA)]
    if B in (65, 4097):
        combos += [("y", True, DELTA), ("next", True, DELTA), ("double", True, 0.0), ("double", False, DELTA), ("y", False, 0.0), ("next", False, 0.0)]
    for shift in _shifts(B, SORTS):
        case = make_case(np.random.default_rng(100 * A + B + shift), B, A, shift)
        for mode, weighted, delta in combos:
            want = rule_of(case, mode, weighted, delta, 1.0 / B)
            assert want["bad_rows"] == bad_rows_of(B, shift, mode, weighted)
            first = None
            for offset in (False, True):                             # both placements; and two runs give the same bytes
                got = _call(case, mode, weighted, delta, offset=offset, scale=1.0 / B)
                _equal(got, want, (A, B, shift, mode, weighted, delta, offset), OUTPUTS)
                if first is not None:
                    for k, g in got.items():
                        assert g.tobytes() == first[k].tobytes(), (A, B, shift, mode, k)
                first = got


def test_null_outputs_stay_untouched_and_the_others_unchanged():
    A, B = 5, 257
    case = make_case(np.random.default_rng(11), B, A, 3)
    subsets = [(), ("priority",), ("bad_rows",), ("grad_q", "bad_rows"), ("stats",), ("stats", "mean_loss"), ("loss", "y_out"),
               ("loss", "priority", "y_out", "grad_q"), ("priority", "stats", "mean_loss", "bad_rows")] + [tuple(k for k in OUTPUTS if k != o)
                                                                                                         for o in OUTPUTS if o != "stats"]
    for mode in MODES:
        want = rule_of(case, mode, True, DELTA, 1.0 / B)
        for n, subset in enumerate(subsets):
            expect = dict(want, bad_rows=want["bad_rows"] if subset else 0)      # nothing asked for: nothing is launched, nothing counted
            _equal(_call(case, mode, want=subset, offset=bool(n % 2), scale=1.0 / B), expect, (mode, subset), OUTPUTS)


def test_the_sums_are_the_stated_tree_not_a_plain_sum():
    """At B = 4097 the mean loss in the stated order differs from the index-order sum (asserted on the host for these inputs): the kernels
    give the stated one."""
    B = 4097
    for A in ACTIONS:
        case = make_case(np.random.default_rng(100 * A + B + B % len(SORTS)), B, A, B % len(SORTS))
        for mode in MODES:
            want = rule_of(case, mode)
            plain = np.float64(0.0)
            for t in want["u"][:, 0]:
                plain = plain + t
            got = _call(case, mode, want=("stats",))
            assert got["stats"].tobytes() == want["stats"].tobytes() and got["stats"][0] != plain / np.float64(B)


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
def _kw(t, mode, weighted=True):
    kw = dict(y=t["y"]) if mode == "y" else dict(q_next=t["q_next"], ret=t["ret"], discount=t["discount"])
    if mode == "double":
        kw["q_select"] = t["q_select"]
    if weighted:
        kw["weight"] = t["weight"]
    return kw


@pytest.mark.parametrize("A", ACTIONS)
def test_td_loss_follows_the_rule_and_its_backward_gives_the_closed_form_gradient(A):
    import torch
    from snac_amd import TDLoss, _lib

    B = 4097
    dev = torch.device("cuda", torch.cuda.current_device())
    case = make_case(np.random.default_rng(A), B, A)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in INPUTS}
    for huber, mode, weighted in ((None, "next", False), (DELTA, "double", True), (DELTA, "y", True)):
        td = TDLoss(A, huber, device=dev)
        delta = 0.0 if huber is None else huber
        want = rule_of(case, mode, weighted, delta, 1.0 / B)
        q = t["q"].clone().requires_grad_()
        extra = {k: v.clone().requires_grad_() for k, v in _kw(t, mode, weighted).items()}
        mean, per, prio, y_out = td.loss(q, t["action"], **extra, want_per_sample=True, want_y=True)
        assert _lib.lib().snac_last_kernel() == b"k_td_loss" and mean.requires_grad and not per.requires_grad and not prio.requires_grad
        assert mean.shape == () and mean.dtype == torch.float32 and td.stats.dtype == torch.float64 and td.stats.shape == (8,) and not y_out.requires_grad
        mean.backward()
        assert all(v.grad is None for v in extra.values())           # constants of the loss
        _same(q.grad.cpu().numpy(), want["grad_q"], (A, mode, "q.grad"))
        _same(per.cpu().numpy(), want["loss"], (A, mode, "loss per sample"))
        _same(prio.cpu().numpy(), want["priority"], (A, mode, "priority"))
        _same(y_out.cpu().numpy(), want["y_out"], (A, mode, "y"))
        assert mean.detach().cpu().numpy().reshape(1).tobytes() == want["mean_loss"].tobytes()
        assert td.stats.cpu().numpy().tobytes() == want["stats"].tobytes()
        st = td.stats_dict()
        assert list(st) == ["loss", "td_loss", "abs_td", "q_taken", "target", "linear_fraction", "good", "weight"]
        assert list(st.values()) == list(want["stats"]) and st["good"] == B - want["bad_rows"]
        # a smaller batch after a larger one (the scratch is kept), the mean alone, with y, and a gradient that is not 1
        n = 65
        small = {k: v[:n].contiguous() for k, v in t.items()}
        q2 = small["q"].clone().requires_grad_()
        out = td.loss(q2, small["action"], **_kw(small, mode, weighted), want_y=True)
        assert len(out) == 2 and out[1].shape == (n,)
        (3.0 * out[0]).backward()
        w2 = rule_of({k: case[k][:n] for k in INPUTS}, mode, weighted, delta, 1.0 / n)
        assert q2.grad.cpu().numpy().tobytes() == (np.float32(3.0) * w2["grad_q"]).tobytes()
        assert torch.is_tensor(td.loss(small["q"], small["action"], **_kw(small, mode, weighted)))
        assert int(td.bad_rows.cpu()[0]) == want["bad_rows"] + 2 * w2["bad_rows"] > 0     # a counter: it adds up over the calls
        with pytest.raises(ValueError, match="action must be a contiguous torch.int64"):
            td.loss(q, t["action"].int(), t["y"])
        with pytest.raises(ValueError, match="weight must have shape"):
            td.loss(q, t["action"], t["y"], weight=t["weight"][:-1])


def test_td_loss_takes_an_envs_actions_device_and_stream():
    import torch
    from snac_amd import TDLoss

    for kind, A in ((1, 3), (2, 5), (3, 8)):
        env, _ = short_env(kind, 65, True, seed=3)
        td = TDLoss(env, huber=DELTA)
        assert td.num_actions == env.num_actions == A and td.device == env.device and td.env is env
        case = make_case(np.random.default_rng(kind), 65, A)
        t = {k: torch.from_numpy(case[k]).to(env.device) for k in INPUTS}
        mean = td.loss(t["q"], t["action"], **_kw(t, "double"))
        assert mean.cpu().numpy().reshape(1).tobytes() == rule_of(case, "double", True, DELTA, 1.0 / 65)["mean_loss"].tobytes()
        with pytest.raises(ValueError, match="device is the env's"):
            TDLoss(env, device=env.device)


def test_the_priorities_go_into_a_priority_tree_as_they_are():
    """priority from the device and the same values from the host give the same tree."""
    import torch
    from snac_amd import PriorityTree, TDLoss

    dev = torch.device("cuda", torch.cuda.current_device())
    A, B = 5, 257
    case = make_case(np.random.default_rng(5), B, A)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in INPUTS}
    _, _, prio = TDLoss(A, DELTA, device=dev).loss(t["q"], t["action"], **_kw(t, "double"), want_per_sample=True)
    want = rule_of(case, "double", True, DELTA, 1.0 / B)["priority"]
    index = torch.arange(B, dtype=torch.int32, device=dev)
    trees = [PriorityTree(512, device=dev), PriorityTree(512, device=dev)]
    trees[0].update(index, prio)
    trees[1].update(index, torch.from_numpy(want).to(dev))
    w = [tr.weights().view(torch.int32).cpu().numpy() for tr in trees]      # the leaves: rint(priority * 2^16)
    # ten of the 25 sorts have a |td| drawn from a continuous distribution (the placed ones share theirs, the bad ones give 0)
    assert w[0].tobytes() == w[1].tobytes() and len(np.unique(w[0][:B])) > B // 4 and not w[0][B:].any()
    assert trees[0].total() == trees[1].total() > 0


def test_the_device_mean_is_no_farther_from_float64_than_the_float32_composition():
    """On identical inputs, against examples/dqn_batched.py's composition in float32 on the device (max, the target arithmetic, gather,
    the weighted squared or Huber error, the mean): the device mean loss is no farther from the same composition in float64 than the
    composition's own float32 mean is, with 2^-24 |reference| of slack (the one rounding of mean_loss to float32).  The rows are the
    good ones with finite Q-values everywhere, which the composition can take."""
    import torch
    import torch.nn.functional as F
    from snac_amd import TDLoss

    dev = torch.device("cuda", torch.cuda.current_device())
    for A in ACTIONS:
        full = make_case(np.random.default_rng(40 + A), 8192 + 4 * len(SORTS), A)
        for huber in (None, DELTA):
            probe = rule_of(full, "next", True, 0.0 if huber is None else huber)
            rows = ~probe["bad"] & np.isfinite(full["q"]).all(axis=1) & np.isfinite(full["q_next"]).all(axis=1)
            case = {k: np.ascontiguousarray(full[k][rows]) for k in INPUTS}
            B = int(rows.sum())
            assert B > 4096

            def composition(dtype, where):
                t = {k: torch.from_numpy(case[k]).to(where) for k in INPUTS}
                f = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in t.items()}
                y = f["ret"] + f["discount"] * f["q_next"].max(dim=1).values
                q = f["q"].gather(1, f["action"][:, None]).squeeze(1)
                err = (q - y) ** 2 if huber is None else F.huber_loss(q, y, reduction="none", delta=huber)
                return float((f["weight"] * err).mean())
            ref, comp = composition(torch.float64, "cpu"), composition(torch.float32, dev)
            t = {k: torch.from_numpy(case[k]).to(dev) for k in INPUTS}
            td = TDLoss(A, huber, device=dev)
            mine = float(td.loss(t["q"], t["action"], **_kw(t, "next")))
            print("A %d, B %d, huber %s: reference %.12g, device %+.3g, float32 composition %+.3g" % (A, B, huber, ref, mine - ref, comp - ref))
            assert abs(mine - ref) <= abs(comp - ref) + 2.0 ** -24 * abs(ref), (A, huber, mine, comp, ref)
            assert int(td.bad_rows.cpu()[0]) == 0 and td.stats_dict()["good"] == B


# ---- snac_c51_loss -----------------------------------------------------------------------------------------------------------------------
C51_OUTPUTS = ("loss", "grad", "stats", "mean_loss", "bad_rows")
C51_SHAPES = [(5, 51, B) for B in (1, 2, 63, 64, 65, 129, 4097)] + [(A, K, B) for A, K in ((5, 2), (5, 33), (5, 64), (3, 51), (8, 51)) for B in (65, 129)]


def _c51_call(case, weighted=True, want=C51_OUTPUTS, offset=False, scale=1.0):
    """One snac_c51_loss call with its outputs in a guard arena -> dict of numpy arrays (None where not asked for), and the partials."""
    import torch
    from snac_amd import _lib

    L, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    B, A, K = case["logits"].shape
    W = (B + 63) // 64
    ins = {k: _place(case[k], offset, dev) for k in C51_INPUTS}
    before = {k: flat.clone() for k, (flat, _) in ins.items()}
    arena = guard.Arena(B * (4 * A * K + 4) + W * 64 + 80 + 7 * (guard.BAND + 1024), dev)
    off4, off8 = (4, 8) if offset else (0, 0)
    out = dict(loss=arena.carve((B,), torch.float32, offset=off4, name="loss"),
               grad=arena.carve((B, A, K), torch.float32, offset=off4, name="grad"),
               stats=arena.carve((8,), torch.float64, offset=off8, name="stats"),
               mean_loss=arena.carve((1,), torch.float32, offset=off4, name="mean_loss"),
               partials=arena.carve((W, 8), torch.float64, offset=off8, name="partials"),
               bad_rows=arena.carve((1,), torch.int32, name="bad_rows"))
    if "bad_rows" in want:
        out["bad_rows"].zero_()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = {k: _vp(view) for k, (_, view) in ins.items()}
    o = {k: _vp(out[k]) if k in want else None for k in C51_OUTPUTS}
    _lib.check(L.snac_c51_loss(B, A, K, p["logits"], p["action"], p["m"], p["weight"] if weighted else None, scale, o["loss"], o["grad"], o["stats"],
                               o["mean_loss"], _vp(out["partials"]), o["bad_rows"], stream))
    if want:
        assert L.snac_last_kernel() == b"k_c51_loss"
    arena.check()
    for k in out:
        if k not in want and not (k == "partials" and "stats" in want):
            guard.view_untouched(out[k], k + " (NULL in the call)")
    for k, (flat, _) in ins.items():
        assert torch.equal(flat.view(torch.uint8), before[k].view(torch.uint8)), k + " was written"
    got = {k: (t.cpu().numpy() if k in want else None) for k, t in out.items() if k != "partials"}
    got["partials"] = out["partials"].cpu().numpy() if "stats" in want else None
    return got


def _c51_equal(got, want, what):
    for k in C51_OUTPUTS + ("partials",):
        g = got[k]
        if g is None:
            continue
        if k == "bad_rows":
            assert int(g[0]) == want[k], (what, k, int(g[0]), want[k])
        else:
            _same(g.reshape(len(g), -1), np.ascontiguousarray(want[k]).reshape(len(g), -1), (what, k))


@pytest.mark.parametrize("A,K,B", C51_SHAPES)
def test_c51_loss_equals_the_rule_byte_for_byte_and_writes_nothing_else(A, K, B):
    shifts = range(len(C51_SORTS)) if B <= 2 else (B % len(C51_SORTS),)      # one or two samples take every sort in turn
    for shift in shifts:
        case = make_c51_case(np.random.default_rng(1000 * A + 10 * K + B + shift), B, A, K, shift)
        for weighted in (True, False) if B in (2, 65, 4097) else (True,):
            want = c51_rule_of(case, weighted, 1.0 / B)
            assert want["bad_rows"] == c51_bad_rows_of(B, shift, weighted)
            first = None
            for offset in (False, True):                             # both placements; and two runs give the same bytes
                got = _c51_call(case, weighted, offset=offset, scale=1.0 / B)
                _c51_equal(got, want, (A, K, B, shift, weighted, offset))
                if first is not None:
                    for k, g in got.items():
                        assert g.tobytes() == first[k].tobytes(), (A, K, B, shift, k)
                first = got


def test_c51_null_outputs_stay_untouched_and_the_sums_are_the_stated_tree():
    A, K, B = 5, 51, 129
    case = make_c51_case(np.random.default_rng(12), B, A, K, 5)
    want = c51_rule_of(case, True, 1.0 / B)
    for n, subset in enumerate([(), ("loss",), ("grad",), ("bad_rows",), ("stats",), ("stats", "mean_loss"), ("loss", "grad"), ("loss", "stats", "bad_rows"),
                                ("grad", "stats", "mean_loss", "bad_rows")]):
        expect = dict(want, bad_rows=want["bad_rows"] if subset else 0)
        _c51_equal(_c51_call(case, want=subset, offset=bool(n % 2), scale=1.0 / B), expect, subset)
    B = 4097                                                          # the stated order differs from the index-order sum (asserted on the host)
    for A in ACTIONS:
        case = make_c51_case(np.random.default_rng(100 * A + B), B, A, 51, B % len(C51_SORTS))
        want = c51_rule_of(case)
        plain = np.float64(0.0)
        for t in want["u"][:, 0]:
            plain = plain + t
        got = _c51_call(case, want=("stats",))
        assert got["stats"].tobytes() == want["stats"].tobytes() and got["stats"][0] != plain / np.float64(B)


@pytest.mark.parametrize("A", ACTIONS)
def test_categorical_support_loss_follows_the_rule_and_its_backward_gives_the_closed_form_gradient(A):
    import torch
    from snac_amd import CategoricalSupport, PriorityTree, _lib

    B, K = 4097, 51
    env, _ = short_env({3: 1, 5: 2, 8: 3}[A], 65, True, seed=3)      # the env's actions, device and stream are taken
    dev = env.device
    sup = CategoricalSupport(env, atoms=K, vmin=0.0, vmax=100.0)
    assert sup.num_actions == A and sup.env is env
    case = make_c51_case(np.random.default_rng(A), B, A, K)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in C51_INPUTS}
    want = c51_rule_of(case, True, 1.0 / B)
    logits = t["logits"].clone().requires_grad_()
    extra = {k: t[k].clone().requires_grad_() for k in ("m", "weight")}
    mean, ce = sup.loss(logits, t["action"], extra["m"], weight=extra["weight"], want_per_sample=True)
    assert _lib.lib().snac_last_kernel() == b"k_c51_loss" and mean.requires_grad and not ce.requires_grad and mean.shape == ()
    mean.backward()
    assert all(v.grad is None for v in extra.values())               # constants of the loss
    _c51_equal(dict(loss=ce.cpu().numpy(), grad=logits.grad.cpu().numpy(), stats=sup.stats.cpu().numpy(), mean_loss=mean.detach().cpu().numpy().reshape(1),
                    bad_rows=sup.bad_rows.cpu().numpy(), partials=None), want, (A, "surface"))
    st = sup.stats_dict()
    assert list(st) == ["loss", "cross_entropy", "entropy", "target_mass", "good", "weight"] and st["good"] == B - want["bad_rows"]
    assert [st[k] for k in st] == [want["stats"][i] for i in (0, 1, 2, 3, 6, 7)]
    n = 65                                                           # a smaller batch after a larger one, no weights, a gradient that is not 1
    l2 = t["logits"][:n].clone().requires_grad_()
    (3.0 * sup.loss(l2, t["action"][:n].contiguous(), t["m"][:n].contiguous())).backward()
    w2 = c51_rule_of({k: case[k][:n] for k in C51_INPUTS}, False, 1.0 / n)
    assert l2.grad.cpu().numpy().tobytes() == (np.float32(3.0) * w2["grad"]).tobytes()
    assert int(sup.bad_rows.cpu()[0]) == want["bad_rows"] + w2["bad_rows"]      # the same counter as project()'s: it adds up
    index = torch.arange(B, dtype=torch.int32, device=dev)           # the cross-entropies as priorities, from the device and from the host
    trees = [PriorityTree(B, device=dev), PriorityTree(B, device=dev)]
    trees[0].update(index, ce)
    trees[1].update(index, torch.from_numpy(want["loss"]).to(dev))
    assert trees[0].weights().view(torch.int32).cpu().numpy().tobytes() == trees[1].weights().view(torch.int32).cpu().numpy().tobytes()
    assert trees[0].total() > 0
    with pytest.raises(ValueError, match="m must have shape"):
        sup.loss(logits, t["action"], t["m"][:, :-1].contiguous())


def test_the_device_cross_entropy_is_no_farther_from_float64_than_the_float32_composition():
    """The criterion of the TD test above, against examples/dqn_batched.py's composition (log_softmax over [B, A, K], the gather, the
    product with m, the sum, the weighting, the mean) on the good rows."""
    import torch
    from snac_amd import CategoricalSupport

    dev = torch.device("cuda", torch.cuda.current_device())
    K = 51
    for A in ACTIONS:
        full = make_c51_case(np.random.default_rng(50 + A), 8192 + 4 * len(C51_SORTS), A, K)
        rows = ~c51_rule_of(full)["bad"] & np.isfinite(full["logits"]).all(axis=(1, 2))
        case = {k: np.ascontiguousarray(full[k][rows]) for k in C51_INPUTS}
        B = int(rows.sum())
        assert B > 4096

        def composition(dtype, where):
            t = {k: torch.from_numpy(case[k]).to(where) for k in C51_INPUTS}
            logp = t["logits"].to(dtype).log_softmax(-1)[torch.arange(B, device=where), t["action"]]
            return float((t["weight"].to(dtype) * -(t["m"].to(dtype) * logp).sum(1)).mean())
        ref, comp = composition(torch.float64, "cpu"), composition(torch.float32, dev)
        t = {k: torch.from_numpy(case[k]).to(dev) for k in C51_INPUTS}
        sup = CategoricalSupport(A, atoms=K, device=dev)
        mine = float(sup.loss(t["logits"], t["action"], t["m"], weight=t["weight"]))
        print("A %d, B %d: reference %.12g, device %+.3g, float32 composition %+.3g" % (A, B, ref, mine - ref, comp - ref))
        assert abs(mine - ref) <= abs(comp - ref) + 2.0 ** -24 * abs(ref), (A, mine, comp, ref)
        assert int(sup.bad_rows.cpu()[0]) == 0 and sup.stats_dict()["good"] == B


# ---- the examples ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", [dict(), dict(double=True, huber=1.0, prioritized=True, n_step=3), dict(distributional=True, prioritized=True)],
                         ids=["plain", "double_huber_prioritized_nstep", "distributional_prioritized"])
def test_the_dqn_example_trains_with_the_device_loss(how):
    import torch

    mod = _example("dqn_batched")
    info = {}
    losses, _ = mod.run(envs=256, ticks=4, batch=512, prefill=16, device_loss=True, info=info, log=lambda line: None, **how)
    assert len(losses) == 4 and np.isfinite(losses).all() and info["bad_rows"] == 0
    if how.get("prioritized"):
        leaves = info["priorities"].view(torch.int32).cpu().numpy()  # the prefill gave every entry one weight: the updates moved them
        assert len(np.unique(leaves[leaves > 0])) > 16
    with pytest.raises(ValueError, match="belong to device_loss"):
        mod.run(envs=256, ticks=1, huber=1.0, log=lambda line: None)


def test_the_sac_example_trains_with_the_device_loss():
    mod = _example("sac_batched")
    info = {}
    out = mod.run(envs=256, ticks=4, batch=512, prefill=16, device_loss=True, info=info, log=lambda line: None)
    assert np.isfinite(np.asarray(out[0], np.float64)).all() and info["bad_rows"] == 0 and info["td_bad_rows"] == 0
