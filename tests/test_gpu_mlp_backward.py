"""GPU: snac_mlp_backward, DeviceMLP.backward / train_forward and the three examples with --device-backward.

The kernels through the C ABI on the generated inputs of tests/test_mlp_backward_host.py (make_backward_case: normal rows, large
magnitudes, the row that cuts a hidden unit to exactly 0 and leaves one at -0.0, and the cancel pairs over the batch and over k that tell
the stated orders from every other association; that they do is asserted there, on the host), byte for byte against mlp_backward_rule:
the networks [7, 4], [51, 64, 6], [51, 65, 1, 9], [502, 256, 256, 6], [512, 256, 255, 64] and [1, 1] at 1, 15, 16, 17, C - 1, C, C + 1 and
2 C + 1 rows (the two widest up to C + 1) -- the smallest sizes that cross the 16-row tile, the chunk, the reduce over two and three
chunks and the 64-wide tiles of outputs and inputs (65, 255, 502) -- with float32 and float64 rows, written and accumulated, every array
also one element into its allocation.  grad is carved from a guard arena; work is filled with NaN bytes and allocated larger than asked
for, and the bytes past work_bytes stay; x, grad_y and the weights keep their bytes; two runs give equal bytes.  Then DeviceMLP on a
torch.nn.Sequential with TDLoss, PPOLoss and SearchLoss, accumulation by autograd, an Adam step between two calls, the refusal of a parameter
written between forward and backward and of a double backward, the module in float64 torch within the host test's derived bound, and the
examples for a few ticks."""
import copy
import ctypes as C

import numpy as np
import pytest

from devmem import _example, _place, _vp
import guard
from specmath import _same
from test_gpu_mlp import PlacedNet, module_of
from test_mlp_backward_host import (CHUNK, DIMS, accumulate_case, autograd_reference, backward_bound, backward_of, backward_seed, bound_case, layer_views,
                                    make_backward_case, mlp_backward_rule, num_params, work_bytes_formula)
from test_mlp_host import WIDE

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
SLACK = 4096                                                         # bytes of work past work_bytes, which must stay as they were
PLACEMENTS = ((0, False, 0), (0, True, 1), (1, False, 1), (1, True, 0))      # (float64 rows, one element into the allocation, accumulate)


def _backward(case, f64, offset, accumulate, g_old):
    """One snac_mlp_backward call -> the flat gradient as numpy."""
    import torch
    from snac_amd import _lib

    p = PlacedNet(case, f64, offset)
    dims = case["dims"]
    P = num_params(dims)
    gy_flat, gy = _place(case["grad_y"], offset, p.dev)
    gy_before = gy_flat.clone()
    arena = guard.Arena(P * 4 + 16 + 3 * (guard.BAND + 1024), p.dev)
    grad = arena.carve((P,), torch.float32, offset=4 if offset else 0, name="grad")
    if accumulate:
        grad.copy_(torch.from_numpy(g_old))
    L = _lib.lib()
    need = L.snac_mlp_backward_work_bytes(C.byref(p.net), p.rows)
    assert need == work_bytes_formula(dims, p.rows)
    at = 8 if offset else 0                                          # 8-byte aligned, no more
    work = torch.full((at + need + SLACK,), 0xFF, dtype=torch.uint8, device=p.dev)       # NaN bytes
    _lib.check(L.snac_mlp_backward(C.byref(p.net), _vp(p.x), p.f64, p.rows, _vp(gy), _vp(grad), accumulate, C.c_void_p(work.data_ptr() + at), need,
                                   p.stream))
    assert L.snac_last_kernel() == b"k_mlp_grad_reduce"
    arena.check()
    p.unchanged()
    assert torch.equal(gy_flat.view(torch.uint8), gy_before.view(torch.uint8)), "grad_y was written"
    assert bool((work[at + need:] == 0xFF).all()) and bool((work[:at] == 0xFF).all()), "work was written outside its work_bytes"
    return grad.cpu().numpy()


def _check_case(case, g_old, what):
    want = backward_of(case)["flat"], backward_of(case, g_old=g_old)["flat"]
    first = {}
    for f64, offset, accumulate in PLACEMENTS:
        got = _backward(case, f64, offset, accumulate, g_old)
        _same(got, want[accumulate], (what, f64, offset, accumulate))
        if accumulate in first:                                      # another placement, another input type: the same bytes
            assert got.tobytes() == first[accumulate].tobytes(), (what, accumulate)
        first[accumulate] = got


# ---- the kernels against the rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,rows", [(d, r) for d in DIMS for r in ROWS if r <= CHUNK + 1 or d not in WIDE],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_the_kernels_equal_the_rule_byte_for_byte_and_write_nothing_else(dims, rows):
    rng = np.random.default_rng(backward_seed(dims, rows))
    case = make_backward_case(rng, dims, rows)
    _check_case(case, rng.normal(size=num_params(dims)).astype(np.float32), (dims, rows))


def test_accumulate_adds_in_float64_and_rounds_once():
    case, g_old = accumulate_case()
    _check_case(case, g_old, "accumulate")
    assert _backward(case, 0, False, 1, g_old)[1] == 2.0 ** 24 + 2.0


def test_a_nan_row_and_non_finite_gradients_propagate_as_the_rule_says():
    dims, rows = (51, 64, 6), 17
    rng = np.random.default_rng(backward_seed(dims, rows) + 3)
    case = make_backward_case(rng, dims, rows)
    case["x"][4, 7] = np.nan
    case["grad_y"][9, 2] = np.inf                                    # 0 * inf = NaN below every cut unit of that row
    want = backward_of(case)["flat"]
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    _check_case(case, rng.normal(size=num_params(dims)).astype(np.float32), "non-finite")


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
def _grads(net):
    import torch

    return np.concatenate([np.concatenate([m.weight.grad.cpu().numpy().ravel(), m.bias.grad.cpu().numpy()]) for m in net if isinstance(m, torch.nn.Linear)])


def _rule_of_module(net, x, grad_y, **kw):
    import torch

    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    return mlp_backward_rule([m.weight.detach().cpu().numpy() for m in lin], [m.bias.detach().cpu().numpy() for m in lin], x.cpu().numpy(),
                             grad_y.cpu().numpy(), CHUNK, **kw)["flat"]


def loss_inputs(which, rows, A, dev):
    """A loss of the outputs y [rows, A (+ 1)] as a function y -> 0-dim tensor, from fixed random minibatch tensors."""
    import torch
    from snac_amd import PPOLoss, SearchLoss, TDLoss

    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)             # noqa: E731
    action = torch.randint(0, A, (rows,), generator=g).to(dev)
    if which == "td":
        rule = TDLoss(A, device=dev)
        q_next, ret, disc = r(rows, A), r(rows), torch.rand(rows, generator=g).to(dev)
        return lambda y: rule.loss(y, action, q_next=q_next, ret=ret, discount=disc)
    if which == "ppo":
        rule = PPOLoss(A, device=dev)
        mb = (action, -torch.rand(rows, generator=g).to(dev) - 1.0, r(rows), r(rows), r(rows))
        return lambda y: rule.loss(y[:, :A].contiguous(), y[:, A].contiguous(), mb)
    rule = SearchLoss(A, device=dev)
    mb = (torch.softmax(r(rows, A), 1).contiguous(), r(rows))
    return lambda y: rule.loss(y[:, :A].contiguous(), y[:, A].contiguous(), mb)


@pytest.mark.parametrize("which", ("td", "ppo", "search"))
def test_train_forward_with_the_device_losses_gives_the_rules_gradients(which):
    import torch
    from snac_amd import DeviceMLP

    dev = torch.device("cuda", torch.cuda.current_device())
    A, rows = 5, CHUNK + 1
    dims = (51, 64, A) if which == "td" else (51, 64, A + 1)
    case = make_backward_case(np.random.default_rng(backward_seed(dims, rows) + 5), dims, rows, cancel=False)
    net = module_of(case, dev)
    mlp = DeviceMLP(net)
    assert mlp.num_params == num_params(dims)
    loss_of = loss_inputs(which, rows, A, dev)
    for dtype in (torch.float32, torch.float64):
        x = torch.from_numpy(case["x"]).to(dev).to(dtype)
        plain = mlp.forward(x)
        leaf = plain.clone().requires_grad_()                        # the loss's own gradient to the outputs
        loss_of(leaf).backward()
        grad_y = leaf.grad
        assert bool(torch.isfinite(grad_y).all()) and bool((grad_y != 0).any())
        net.zero_grad(set_to_none=True)
        y = mlp.train_forward(x)
        assert y.requires_grad and y.dtype == torch.float32 and y.detach().cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
        loss_of(y).backward()                                        # (autograd runs it on a thread of its own: snac_last_kernel() is per thread)
        want = _rule_of_module(net, x, grad_y)
        _same(_grads(net), want, (which, dtype))
        flat, views = mlp.backward(x, grad_y)                        # the method itself: the same bytes, views of the parameters' shapes
        _same(flat.cpu().numpy(), want, (which, dtype, "backward"))
        for (gw, gb), (ww, wb), m in zip(views, layer_views(dims, want), [m for m in net if isinstance(m, torch.nn.Linear)]):
            assert gw.shape == m.weight.shape and gb.shape == m.bias.shape and gw.data_ptr() >= flat.data_ptr()
            assert gw.cpu().numpy().tobytes() == ww.tobytes() and gb.cpu().numpy().tobytes() == wb.tobytes()
        # a second backward without zero_grad: autograd accumulates, in float32
        loss_of(mlp.train_forward(x)).backward()
        _same(_grads(net), want + want, (which, dtype, "accumulated"))
        # accumulate=True into a flat buffer: in float64, rounded once
        out = flat.clone()
        assert mlp.backward(x, grad_y, accumulate=True, out=out)[0] is out
        _same(out.cpu().numpy(), _rule_of_module(net, x, grad_y, g_old=want), (which, dtype, "accumulate=True"))


def test_an_adam_step_between_two_calls_is_seen_by_the_next_and_any_torch_loss_works():
    import torch
    from snac_amd import DeviceMLP

    dev = torch.device("cuda", torch.cuda.current_device())
    dims, rows = (51, 65, 1, 9), 33
    case = make_backward_case(np.random.default_rng(backward_seed(dims, rows) + 7), dims, rows, cancel=False)
    net = module_of(case, dev)
    mlp = DeviceMLP(net)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    x = torch.from_numpy(case["x"]).to(dev)
    target = torch.randn(rows, dims[-1], generator=torch.Generator().manual_seed(3)).to(dev)
    seen = []
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        y = mlp.train_forward(x)
        caught = []
        y.register_hook(caught.append)                               # mse_loss's gradient to y, as autograd hands it over
        torch.nn.functional.mse_loss(y, target).backward()
        grad_y = caught[0].contiguous()
        want = _rule_of_module(net, x, grad_y)                       # the parameters as they are now: after the step, the stepped ones
        _same(_grads(net), want, ("adam", step))
        _same(mlp.backward(x, grad_y)[0].cpu().numpy(), want, ("adam", step, "backward"))
        seen.append(want)
        opt.step()
    assert (seen[0] != seen[1]).any()


def test_a_parameter_written_between_forward_and_backward_and_a_double_backward_raise():
    """The backward pass recomputes the activations from the parameters as they are, so a parameter written in place since
    train_forward() would give gradients that do not belong to the y the loss saw: autograd's version check refuses it, as for a torch
    module.  The backward runs outside autograd: differentiating through it a second time raises instead of giving nothing."""
    import torch
    from snac_amd import DeviceMLP

    dev = torch.device("cuda", torch.cuda.current_device())
    dims, rows = (7, 5, 4), 17
    case = make_backward_case(np.random.default_rng(backward_seed(dims, rows) + 9), dims, rows, cancel=False)
    net = module_of(case, dev)
    mlp = DeviceMLP(net)
    x = torch.from_numpy(case["x"]).to(dev)
    for p in net.parameters():
        y = mlp.train_forward(x)
        with torch.no_grad():
            p.mul_(0.5)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            y.sum().backward()
    y = mlp.train_forward(x)
    (g,) = torch.autograd.grad((y * y).sum(), net[0].weight, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    net.zero_grad(set_to_none=True)
    mlp.train_forward(x).sum().backward()                            # and an untouched pass still works afterwards
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


def test_the_module_in_float64_torch_stays_within_the_derived_bound():
    """copy.deepcopy(net).double() on the device with loss = sum(y * grad_y), on the host test's batch (bound_case: the rows that may take
    the other branch of the mask left out on both sides), against DeviceMLP.backward within backward_bound() of the host test, whose
    docstring derives it.  No slack is added."""
    import torch
    from snac_amd import DeviceMLP

    dev = torch.device("cuda", torch.cuda.current_device())
    dims = (51, 64, 6)
    case, generated = bound_case(dims)
    assert len(case["x"]) >= 128 and generated - len(case["x"]) <= 0.02 * generated
    net = module_of(case, dev)
    x = torch.from_numpy(case["x"]).to(dev).to(torch.float32)
    grad_y = torch.from_numpy(case["grad_y"]).to(dev)
    flat, _ = DeviceMLP(net).backward(x, grad_y)
    ref_net = copy.deepcopy(net).double()
    (ref_net(x.double()) * grad_y.double()).sum().backward()
    ref = _grads(ref_net)
    keep, err = backward_bound(case, backward_of(case))
    assert keep.all()
    ratio = np.abs(flat.cpu().numpy().astype(np.float64) - ref) / (err + 1e-300)
    host = np.abs(autograd_reference(case) - ref).max()
    print("largest error / bound against float64 torch on the device: %.3g over %d rows (its distance from the host's float64: %.3g)" % (
        ratio.max(), len(case["x"]), host))
    assert ratio.max() <= 1.0


# ---- the examples ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_loss", (False, True))
def test_the_dqn_example_with_the_device_backward_finishes_with_finite_losses(device_loss):
    mod = _example("dqn_batched")
    losses, _ = mod.run(envs=256, ticks=3, batch=256, prefill=8, device_backward=True, device_loss=device_loss, log=lambda line: None)
    assert len(losses) == 3 and np.isfinite(losses).all()
    with pytest.raises(ValueError, match="device_backward is not for distributional"):
        mod.run(envs=256, ticks=1, batch=256, prefill=8, device_backward=True, distributional=True, log=lambda line: None)


def test_the_ppo_example_with_the_device_backward_finishes_with_finite_losses():
    mod = _example("ppo_batched")
    losses, _ = mod.run(envs=256, iterations=2, horizon=8, epochs=1, batch=1024, device_rollout=True, device_backward=True, device_loss=True,
                        log=lambda line: None)
    assert len(losses) >= 2 and np.isfinite(losses).all()
    with pytest.raises(ValueError, match="device_backward needs device_rollout"):
        mod.run(envs=256, iterations=1, horizon=8, epochs=1, batch=1024, device_backward=True, log=lambda line: None)


def test_the_selfplay_example_with_the_device_backward_finishes_with_finite_losses():
    mod = _example("alphazero_selfplay")
    for device_loss in (False, True):
        losses, _ = mod.train(kind=2, envs=32, steps=3, moves=3, iterations=4, paths=2, nodes=64, batch=64, capacity=8, device_backward=True,
                              device_loss=device_loss, device_evaluator=device_loss)
        assert len(losses) == 3 and np.isfinite(losses).all()
