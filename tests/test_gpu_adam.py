"""GPU: snac_mlp_adam_step, snac_mlp_lerp, DeviceAdam and the three examples with --device-optimizer.

The kernels through the C ABI on the generated inputs of tests/test_adam_host.py, byte for byte against adam_rule: the networks [1, 1]
(P = 2), [7, 4] (32, under one wave), [51, 64, 6] (3718: W = 59, the last wave partly filled), [51, 65, 1, 9] (segment boundaries inside
waves, a layer of one unit), [51, 64, 64, 6] (7878: W = 124 > 64, stage two's lanes add two partials) and [502, 256, 256, 6] (196 102:
every block of a large grid redoes stage two); t = 1 from zero moments and t = 7 from random ones; the clip off, clipping and loose; no
target, tau = 0.005 and tau = 1; every array both at its allocation's start and one element in.  Every written array -- each w[l] / b[l]
of the network and of the target, m, v, norm_out and bad_steps -- is carved from a guard arena; grad keeps its bytes; the slack past
partials[W) stays 0xFF; two runs give equal bytes.  Then the order case, the subnormal case and the bad step of the host test,
snac_mlp_lerp alone, DeviceAdam on a torch.nn.Sequential against mlp_backward_rule plus adam_rule over five steps, and the examples for a
few ticks."""
import copy
import ctypes as C

import numpy as np
import pytest

from devmem import _example, _place, _vp
import guard
from test_adam_host import (ADAM_NETS, CLIPS, TAUS, adam_rule, adam_seed, bad_case, biases_of, flatten, lerp_rule, make_adam_case, order_case, same_step,
                            split, step_of, subnormal_case)
from test_gpu_mlp_backward import loss_inputs
from test_mlp_backward_host import CHUNK, mlp_backward_rule, num_params

pytestmark = pytest.mark.gpu

SLACK = 64                                                           # doubles past partials[W), which must stay as they were


class _Nets:
    """A case's network (and target) as per-layer arrays carved from a guard arena, with the descriptors that point at them, and m, v,
    norm_out and bad_steps beside them.  offset: every array one element into its allocation."""

    def __init__(self, c, offset, with_target=None):
        import torch
        from snac_amd import _lib

        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.c, P = c, c["P"]
        with_target = c["tgt"] is not None if with_target is None else with_target
        views = 2 * (len(c["dims"]) - 1) * (2 if with_target else 1) + 4
        self.arena = guard.Arena((3 + (1 if with_target else 0)) * P * 4 + 64 + (views + 1) * (guard.BAND + 1024), self.dev)
        o4, o8 = (4, 8) if offset else (0, 0)

        def net_of(flat, name):
            net = _lib.Mlp()
            net.layers = len(c["dims"]) - 1
            for l, d in enumerate(c["dims"]):
                net.dim[l] = d
            arrays = []
            for l, (w, b) in enumerate(split(c["dims"], flat)):
                tw = self.arena.carve(w.shape, torch.float32, offset=o4, name="%s.w%d" % (name, l))
                tb = self.arena.carve(b.shape, torch.float32, offset=o4, name="%s.b%d" % (name, l))
                tw.copy_(torch.from_numpy(w))
                tb.copy_(torch.from_numpy(b))
                net.w[l], net.b[l] = tw.data_ptr(), tb.data_ptr()
                arrays.append((tw, tb))
            return net, arrays

        self.net, self.net_arrays = net_of(c["theta"], "net")
        self.tgt, self.tgt_arrays = net_of(c["tgt"], "tgt") if with_target else (None, None)
        self.m = self.arena.carve((P,), torch.float32, offset=o4, name="m")
        self.v = self.arena.carve((P,), torch.float32, offset=o4, name="v")
        self.m.copy_(torch.from_numpy(c["m"]))
        self.v.copy_(torch.from_numpy(c["v"]))
        self.norm_out = self.arena.carve((2,), torch.float64, offset=o8, name="norm_out")
        self.bad = self.arena.carve((1,), torch.int32, offset=o4, name="bad_steps")
        self.bad.zero_()
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    @staticmethod
    def flat(arrays):
        return flatten([(w.cpu().numpy(), b.cpu().numpy()) for w, b in arrays])


def _step(c, offset):
    """One snac_mlp_adam_step call -> (dict of numpy outputs as adam_rule's, bad_steps)."""
    import torch
    from snac_amd import _lib

    n = _Nets(c, offset)
    W = -(-c["P"] // 64)
    g_flat, g = _place(c["g"], offset, n.dev)
    g_before = g_flat.clone()
    at = 1 if offset else 0                                          # 8-byte aligned, no more
    scratch = torch.full(((at + W + SLACK) * 8,), 0xFF, dtype=torch.uint8, device=n.dev)
    partials = scratch.view(torch.float64)[at:at + W]
    L = _lib.lib()
    _lib.check(L.snac_mlp_adam_step(C.byref(n.net), _vp(g), _vp(n.m), _vp(n.v), c["lr"], c["beta1"], c["beta2"], c["eps"], c["bias1"], c["bias2"],
                                    c["max_norm"], C.byref(n.tgt) if n.tgt is not None else None, c["tau"], _vp(n.norm_out), _vp(partials), _vp(n.bad),
                                    n.stream))
    assert L.snac_last_kernel() == b"k_adam_update"
    n.arena.check()
    assert torch.equal(g_flat.view(torch.uint8), g_before.view(torch.uint8)), "grad was written"
    raw = scratch.view(torch.float64)
    assert bool((raw[:at].view(torch.uint8) == 0xFF).all()) and bool((raw[at + W:].view(torch.uint8) == 0xFF).all()), "partials: written outside [0, W)"
    got = dict(theta=n.flat(n.net_arrays), m=n.m.cpu().numpy(), v=n.v.cpu().numpy(), tgt=None if n.tgt is None else n.flat(n.tgt_arrays),
               norm_out=n.norm_out.cpu().numpy(), partials=partials.cpu().numpy())
    return got, int(n.bad.cpu()[0])


def _check(c, what, offsets=(False, True)):
    want = step_of(c)
    for offset in offsets:
        got, bad = _step(c, offset)
        same_step(got, want, (what, offset))
        assert bad == int(want["bad"]), (what, offset, bad)
    again, _ = _step(c, False)                                       # two runs: equal bytes
    for k, a in again.items():
        assert a is None or a.tobytes() == got[k].tobytes(), (what, k)
    return want


# ---- the kernels against the rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", ADAM_NETS, ids=lambda d: "x".join(map(str, d)))
def test_the_kernels_equal_the_rule_byte_for_byte_and_write_nothing_else(dims):
    seen = set()
    for t in (1, 7):
        for clip in CLIPS:
            for tau in TAUS:
                c = make_adam_case(np.random.default_rng(adam_seed(dims, t, clip, tau)), dims, t=t, clip=clip, tau=tau)
                want = _check(c, (dims, t, clip, tau))
                seen.add((clip, bool(want["norm_out"][1] < 1.0)))
                assert (want["theta"] != c["theta"]).any() and not want["bad"]
    assert seen == {("off", False), ("clipped", True), ("loose", False)}


@pytest.mark.parametrize("clip", CLIPS)
def test_the_stated_order_of_the_sum_of_squares(clip):
    """One value 2^30 among 831 ones (the host test asserts that the stated order gives a sum, and a norm, that a sequential sum and
    another pairwise tree do not): partials and norm_out byte for byte."""
    want = _check(order_case(clip), ("order", clip))
    assert want["norm_out"][0] == 2.0 ** 30 + 2.0 ** -22 and (want["norm_out"][1] < 1.0) == (clip == "clipped")


def test_float32_subnormals_are_kept_not_flushed():
    c = subnormal_case()
    want = _check(c, "subnormal")
    assert ((want["v"] > 0) & (want["v"] < np.finfo(np.float32).tiny)).all()
    # and read back as they are: a second step from the stored subnormal moments
    b1, b2 = biases_of(2, c["beta1"], c["beta2"])
    _check(dict(c, theta=want["theta"], m=want["m"], v=want["v"], tgt=want["tgt"], t=2, bias1=b1, bias2=b2), "subnormal, second step")


def test_a_bad_step_writes_no_byte_and_counts():
    """A NaN at the last flat index and an infinity at index 0: no byte of any parameter, of m, v or the target changes (the arena's views
    hold what was copied in), bad_steps == 1, norm_out[1] == 0.0."""
    c = bad_case()
    want = step_of(c)
    assert want["bad"]
    for offset in (False, True):
        got, bad = _step(c, offset)
        assert bad == 1 and got["norm_out"][1] == 0.0 and not np.isfinite(got["norm_out"][0])
        for k in ("theta", "m", "v", "tgt"):
            assert got[k].tobytes() == c[k].tobytes(), (k, offset)
        same_step(got, want, ("bad", offset))
    only_nan = dict(c, g=np.where(np.isinf(c["g"]), np.float32(1.0), c["g"]))      # the NaN of the last wave's last lane alone
    got, bad = _step(only_nan, False)
    assert bad == 1 and got["theta"].tobytes() == c["theta"].tobytes() and np.isnan(got["norm_out"][0])


@pytest.mark.parametrize("dims", (ADAM_NETS[1], ADAM_NETS[3], ADAM_NETS[5]), ids=lambda d: "x".join(map(str, d)))
def test_lerp_alone_moves_the_target_by_the_rule(dims):
    import torch
    from snac_amd import _lib

    for tau in (0.005, 0.5, 1.0):
        for offset in (False, True):
            c = make_adam_case(np.random.default_rng(adam_seed(dims, 7, "off", 0.005) + 5), dims, t=7, tau=0.005)
            c["theta"][0], c["tgt"][-1] = np.nan, -0.0
            n = _Nets(c, offset)
            before = {k: t.clone() for k, t in (("m", n.m), ("v", n.v))}
            L = _lib.lib()
            _lib.check(L.snac_mlp_lerp(C.byref(n.tgt), C.byref(n.net), tau, n.stream))
            assert L.snac_last_kernel() == b"k_mlp_lerp"
            n.arena.check()
            want = lerp_rule(c["tgt"], c["theta"], tau)
            got = n.flat(n.tgt_arrays)
            assert np.array_equal(np.isnan(got), np.isnan(want)) and got[~np.isnan(got)].tobytes() == want[~np.isnan(want)].tobytes(), (dims, tau, offset)
            if tau == 1.0:
                assert got.tobytes() == c["theta"].tobytes()         # the bits copied, the NaN's too
            assert n.flat(n.net_arrays).tobytes() == c["theta"].tobytes(), "the network was written"
            assert torch.equal(n.m, before["m"]) and torch.equal(n.v, before["v"])


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
def _flat_of(net):
    import torch

    return flatten([(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in net if isinstance(m, torch.nn.Linear)])


def _sequential(dims, dev, seed):
    import torch

    torch.manual_seed(seed)
    mods = []
    for l in range(len(dims) - 1):
        mods += [torch.nn.Linear(dims[l], dims[l + 1])] + ([torch.nn.ReLU()] if l < len(dims) - 2 else [])
    return torch.nn.Sequential(*mods).to(dev)


@pytest.mark.parametrize("which", ("search", "td"))
def test_device_adam_on_a_sequential_equals_the_rules_over_five_steps(which):
    import torch
    from snac_amd import DeviceAdam, DeviceMLP

    dev = torch.device("cuda", torch.cuda.current_device())
    A, rows = 5, CHUNK + 1
    dims = (51, 64, A) if which == "td" else (51, 64, A + 1)
    P = num_params(dims)
    net, tnet = _sequential(dims, dev, 3), _sequential(dims, dev, 4)
    mlp, tmlp = DeviceMLP(net), DeviceMLP(tnet)
    hyper = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8)
    opt = DeviceAdam(mlp, max_norm=0.5, target=tmlp, tau=0.005, **hyper)
    assert opt.sync_every_step and not DeviceAdam(mlp, target=tmlp).sync_every_step
    loss_of = loss_inputs(which, rows, A, dev)
    x = torch.randn(rows, dims[0], generator=torch.Generator().manual_seed(5)).to(dev)
    theta, tgt, m, v = _flat_of(net), _flat_of(tnet), np.zeros(P, np.float32), np.zeros(P, np.float32)
    twin = state = None
    for step in range(1, 6):
        if step == 3:
            opt.lr = 3e-3                                            # a plain attribute, changed between steps
            state = opt.state_dict()                                 # and the state as it is after two steps
            twin_net = copy.deepcopy(net)
            twin = DeviceAdam(DeviceMLP(twin_net), max_norm=0.5, **dict(hyper, lr=3e-3))
            twin.load_state_dict(state)
            assert twin.t == 2 and state["m"].data_ptr() != opt._m.data_ptr()
        y = mlp.forward(x).requires_grad_()
        loss_of(y).backward()
        assert y.grad is not None and y.grad_fn is None
        layers = split(dims, theta)
        flat_want = mlp_backward_rule([w for w, _ in layers], [b for _, b in layers], x.cpu().numpy(), y.grad.cpu().numpy(), CHUNK)["flat"]
        b1, b2 = biases_of(step, *hyper["betas"])
        want = adam_rule(theta, flat_want, m, v, opt.lr, hyper["betas"][0], hyper["betas"][1], hyper["eps"], b1, b2, 0.5, tgt, 0.005)
        flat = opt.backward_step(x, y.grad)
        assert flat.cpu().numpy().tobytes() == flat_want.tobytes(), step
        got = dict(theta=_flat_of(net), m=opt._m.cpu().numpy(), v=opt._v.cpu().numpy(), tgt=_flat_of(tnet), norm_out=opt.grad_norm.cpu().numpy(),
                   partials=opt._partials.cpu().numpy())
        same_step(got, want, (which, step))
        assert opt.t == step and not want["bad"] and (want["theta"] != theta).any()
        theta, tgt, m, v = want["theta"], want["tgt"], want["m"], want["v"]
        if twin is not None:                                         # the state carried over: the same steps from it
            y2 = twin.mlp.forward(x).requires_grad_()
            loss_of(y2).backward()
            twin.backward_step(x, y2.grad)
            assert _flat_of(twin_net).tobytes() == theta.tobytes() and twin.t == step
    assert int(opt.bad_steps.cpu()[0]) == 0 and opt.grad_norm.dtype == torch.float64 and tuple(opt.grad_norm.shape) == (2,)
    assert float(opt.grad_norm.cpu()[1]) <= 1.0
    # sync_target: the constructor's tau, another tau, and the hard copy
    for tau in (None, 0.5, 1.0):
        opt.sync_target(tau)
        tgt = lerp_rule(tgt, theta, 0.005 if tau is None else tau)
        assert _flat_of(tnet).tobytes() == tgt.tobytes(), tau
    assert tgt.tobytes() == theta.tobytes()
    # a bad step: nothing moves, t still advances
    bad = torch.zeros(P, device=dev)
    bad[-1] = float("nan")
    opt.step(bad)
    assert opt.t == 6 and int(opt.bad_steps.cpu()[0]) == 1 and _flat_of(net).tobytes() == theta.tobytes() and opt._m.cpu().numpy().tobytes() == m.tobytes()
    assert float(opt.grad_norm.cpu()[1]) == 0.0


def test_a_train_forward_graph_made_before_a_step_is_refused_at_backward():
    """The step writes the parameters outside autograd and bumps their versions: a graph that saved them before is refused, as after a
    torch optimiser's step; so is one through the target's parameters after the target was moved."""
    import torch
    from snac_amd import DeviceAdam, DeviceMLP

    dev = torch.device("cuda", torch.cuda.current_device())
    dims = (7, 5, 4)
    net, tnet = _sequential(dims, dev, 7), _sequential(dims, dev, 8)
    mlp, tmlp = DeviceMLP(net), DeviceMLP(tnet)
    opt = DeviceAdam(mlp, target=tmlp, tau=0.005)
    x = torch.randn(17, 7, generator=torch.Generator().manual_seed(9)).to(dev)
    flat = torch.ones(num_params(dims), device=dev)
    y, ty = mlp.train_forward(x), tmlp.train_forward(x)
    opt.step(flat)
    for out in (y, ty):
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            out.sum().backward()
    ty = tmlp.train_forward(x)
    y = mlp.train_forward(x)
    opt.sync_target(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        ty.sum().backward()
    y.sum().backward()                                               # sync_target wrote the target alone
    assert all(p.grad is not None for p in net.parameters())
    mlp.train_forward(x).sum().backward()                            # and a pass made after the step works


# ---- the examples ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_loss", (False, True))
def test_the_dqn_example_with_the_device_optimizer_finishes_with_finite_losses(device_loss):
    mod = _example("dqn_batched")
    info = {}
    losses, _ = mod.run(envs=256, ticks=4, batch=256, prefill=8, replace=2, device_backward=True, device_optimizer=True, device_loss=device_loss,
                        info=info, log=lambda line: None)
    assert len(losses) == 4 and np.isfinite(losses).all() and info["bad_steps"] == 0
    with pytest.raises(ValueError, match="device_optimizer needs device_backward"):
        mod.run(envs=256, ticks=1, batch=256, prefill=8, device_optimizer=True, log=lambda line: None)


def test_the_ppo_example_with_the_device_optimizer_finishes_with_finite_losses():
    mod = _example("ppo_batched")
    info = {}
    losses, _ = mod.run(envs=256, iterations=2, horizon=8, epochs=1, batch=1024, device_rollout=True, device_backward=True, device_optimizer=True,
                        device_loss=True, info=info, log=lambda line: None)
    assert len(losses) >= 2 and np.isfinite(losses).all() and info["bad_steps"] == 0
    with pytest.raises(ValueError, match="device_optimizer needs device_backward"):
        mod.run(envs=256, iterations=1, horizon=8, epochs=1, batch=1024, device_rollout=True, device_optimizer=True, log=lambda line: None)


def test_the_selfplay_example_with_the_device_optimizer_finishes_with_finite_losses():
    mod = _example("alphazero_selfplay")
    for device_loss in (False, True):
        info = {}
        losses, _ = mod.train(kind=2, envs=32, steps=3, moves=3, iterations=4, paths=2, nodes=64, batch=64, capacity=8, device_backward=True,
                              device_optimizer=True, device_loss=device_loss, device_evaluator=device_loss, info=info)
        assert len(losses) == 3 and np.isfinite(losses).all() and info["bad_steps"] == 0
    with pytest.raises(ValueError, match="device_optimizer needs device_backward"):
        mod.train(kind=2, envs=32, steps=1, device_optimizer=True)
