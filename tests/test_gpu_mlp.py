"""GPU: snac_mlp_forward, snac_mlp_policy_value and DeviceMLP.

The kernels through the C ABI on the generated inputs of tests/test_mlp_host.py (make_mlp_case: normal rows, large magnitudes, a row that
drives a hidden unit to exactly 0 and one to -0.0, a float32 overflow of a hidden unit, a NaN input, a value output that is not finite,
masked and all-masked heads from -inf biases, and the cancel rows that tell the stated order of a sum from every other; that each sort
lands in its branch, that the bad rows follow from the generator and that the other orders change the cancel rows is asserted there, on
the host), byte for byte against mlp_rule: the networks [7, 4], [51, 64, 6], [51, 65, 1, 9], [502, 256, 256, 6], [512, 256, 255, 64]
and [1, 1] at 1, 63, 64, 65, 257 and 4097 rows (the two widest up to 257: those rows already cross every edge of the kernel's tiles of 16
rows, 64 outputs and 16 inputs), float32 and float64 inputs, every array also taken one element into its allocation, which also makes
four runs whose bytes are equal.  Every output is carved from a guard arena: nothing lands outside the outputs, the inputs and the
weights keep their bytes, a NULL output is not written.  Then DeviceMLP on a torch.nn.Sequential: the same bytes, the parameters read in
place after an update, and the module in float64 torch within the host test's derived bound."""
import copy
import ctypes as C

import numpy as np
import pytest

from devmem import _place, _vp
import guard
from specmath import _same
from test_mlp_host import HEADS, NETS, bad_rows_of, case_seed, derived_bound, make_mlp_case, rows_of, rule_of, shifts_of

pytestmark = pytest.mark.gpu

OUTPUTS = ("priors", "value", "logits", "bad_rows")


class PlacedNet:
    """A case's network and rows on the device, and the descriptor that points at them."""

    def __init__(self, case, f64, offset):
        import torch
        from snac_amd import _lib

        self.dev = torch.device("cuda", torch.cuda.current_device())
        x = np.ascontiguousarray(case["x"] if f64 else case["x"].astype(np.float32))
        self.ins = dict(x=_place(x, offset, self.dev))
        for l, (w, b) in enumerate(zip(case["weights"], case["biases"])):
            self.ins["w%d" % l], self.ins["b%d" % l] = _place(w, offset, self.dev), _place(b, offset, self.dev)
        self.before = {k: flat.clone() for k, (flat, _) in self.ins.items()}
        self.net = _lib.Mlp()
        self.net.layers = len(case["weights"])
        for l, d in enumerate(case["dims"]):
            self.net.dim[l] = d
        for l in range(self.net.layers):
            self.net.w[l], self.net.b[l] = self.ins["w%d" % l][1].data_ptr(), self.ins["b%d" % l][1].data_ptr()
        self.x, self.f64, self.rows = self.ins["x"][1], int(f64), len(x)
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def unchanged(self):
        import torch

        for k, (flat, _) in self.ins.items():
            assert torch.equal(flat.view(torch.uint8), self.before[k].view(torch.uint8)), k + " was written"      # bytes: the rows hold NaNs


def _forward(case, f64, offset):
    import torch
    from snac_amd import _lib

    p = PlacedNet(case, f64, offset)
    N = case["dims"][-1]
    arena = guard.Arena(p.rows * N * 4 + 16 + 3 * (guard.BAND + 1024), p.dev)
    y = arena.carve((p.rows, N), torch.float32, offset=4 if offset else 0, name="y")
    _lib.check(_lib.lib().snac_mlp_forward(C.byref(p.net), _vp(p.x), p.f64, p.rows, _vp(y), p.stream))
    assert _lib.lib().snac_last_kernel() == b"k_mlp_forward"
    arena.check()
    p.unchanged()
    return y.cpu().numpy()


def _policy_value(case, f64, offset, want=OUTPUTS):
    """One snac_mlp_policy_value call with its outputs in a guard arena -> dict of numpy arrays (None where not asked for)."""
    import torch
    from snac_amd import _lib

    p = PlacedNet(case, f64, offset)
    A, rows = case["A"], p.rows
    arena = guard.Arena(rows * (8 * A + 16) + 64 + 6 * (guard.BAND + 1024), p.dev)
    off4, off8 = (4, 8) if offset else (0, 0)
    out = dict(priors=arena.carve((rows, A), torch.float32, offset=off4, name="priors"),
               value=arena.carve((rows,), torch.float64, offset=off8, name="value"),
               logits=arena.carve((rows, A + 1), torch.float32, offset=off4, name="logits"),
               bad_rows=arena.carve((1,), torch.int32, offset=off4, name="bad_rows"))
    if "bad_rows" in want:
        out["bad_rows"].zero_()
    o = {k: _vp(out[k]) if k in want else None for k in OUTPUTS}
    L = _lib.lib()
    _lib.check(L.snac_mlp_policy_value(C.byref(p.net), A, _vp(p.x), p.f64, rows, o["priors"], o["value"], o["logits"], o["bad_rows"], p.stream))
    if want:
        assert L.snac_last_kernel() == b"k_mlp_policy_value"
    arena.check()
    for k in OUTPUTS:
        if k not in want:
            guard.view_untouched(out[k], k + " (NULL in the call)")
    p.unchanged()
    return {k: (out[k].cpu().numpy() if k in want else None) for k in OUTPUTS}


def _equal(got, want, what):
    if got["priors"] is not None:
        _same(got["priors"], want["priors"], (what, "priors"))
    if got["value"] is not None:
        assert got["value"].tobytes() == want["value"].tobytes(), (what, "value")
    if got["logits"] is not None:
        _same(got["logits"], want["y"], (what, "logits"))
    if got["bad_rows"] is not None:
        assert int(got["bad_rows"][0]) == want["bad_rows"], (what, int(got["bad_rows"][0]), want["bad_rows"])


PLACEMENTS = ((0, False), (0, True), (1, False), (1, True))          # (float64 input, one element into the allocation)


# ---- the kernels against the rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,A,rows", [(d, A, r) for d, A in NETS for r in rows_of(d)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_the_kernels_equal_the_rule_byte_for_byte_and_write_nothing_else(dims, A, rows):
    for shift in shifts_of(rows):
        case = make_mlp_case(np.random.default_rng(case_seed(dims, rows, shift)), dims, rows, A, shift)
        want = rule_of(case)
        first = None
        for f64, offset in (PLACEMENTS if shift == shifts_of(rows)[0] else PLACEMENTS[1:3]):
            y = _forward(case, f64, offset)
            _same(y, want["y"], (dims, rows, shift, f64, offset, "y"))
            got = dict(y=y)
            if A is not None:
                assert want["bad_rows"] == bad_rows_of(rows, shift)
                got.update(_policy_value(case, f64, offset))
                _equal(got, want, (dims, rows, shift, f64, offset))
            if first is not None:                                    # another placement, another input type: the same bytes
                for k, g in got.items():
                    assert g.tobytes() == first[k].tobytes(), (dims, rows, shift, k)
            first = got


@pytest.mark.parametrize("head", HEADS[1:])
@pytest.mark.parametrize("dims,A", [n for n in NETS if n[1] is not None], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_masked_and_all_masked_heads(dims, A, head):
    for rows in (1, 65):
        for shift in shifts_of(rows):
            case = make_mlp_case(np.random.default_rng(case_seed(dims, rows, shift, head)), dims, rows, A, shift, head)
            want = rule_of(case)
            assert want["bad_rows"] == bad_rows_of(rows, shift, head)
            for f64, offset in PLACEMENTS[1:3]:
                _equal(_policy_value(case, f64, offset), want, (dims, rows, shift, head, f64))


def test_null_outputs_stay_untouched_and_the_others_unchanged():
    dims, A, rows = (51, 64, 6), 5, 257
    case = make_mlp_case(np.random.default_rng(case_seed(dims, rows, 3)), dims, rows, A, 3)
    want = rule_of(case)
    subsets = [(), ("priors",), ("value",), ("logits",), ("bad_rows",), ("priors", "value"), ("value", "bad_rows"), ("priors", "logits")]
    subsets += [tuple(k for k in OUTPUTS if k != o) for o in OUTPUTS]
    for n, subset in enumerate(subsets):
        _equal(_policy_value(case, n % 2, bool(n % 3), want=subset), want, subset)


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
def module_of(case, dev):
    import torch

    mods = []
    for l, (w, b) in enumerate(zip(case["weights"], case["biases"])):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
        mods += [lin] + ([torch.nn.ReLU()] if l < len(case["weights"]) - 1 else [])
    return torch.nn.Sequential(*mods).to(dev)


@pytest.mark.parametrize("dims,A", [NETS[0], NETS[1], NETS[2]], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_device_mlp_follows_the_rule_and_the_parameters_in_place(dims, A):
    import torch
    from snac_amd import DeviceMLP, _lib

    dev = torch.device("cuda", torch.cuda.current_device())
    rows = 257
    case = make_mlp_case(np.random.default_rng(case_seed(dims, rows, 2)), dims, rows, A, 2)
    want = rule_of(case)
    net = module_of(case, dev)
    mlp = DeviceMLP(net, A)
    assert mlp.device == dev and mlp.dims == tuple(dims) and mlp.num_actions == A
    for dtype in (torch.float32, torch.float64):
        x = torch.from_numpy(case["x"]).to(dev).to(dtype)
        y = mlp.forward(x)
        assert _lib.lib().snac_last_kernel() == b"k_mlp_forward" and y.dtype == torch.float32
        _same(y.cpu().numpy(), want["y"], (dims, dtype, "forward"))
        into = torch.empty_like(y)
        assert mlp.forward(x, out=into) is into
        assert into.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        priors, value, logits = mlp.policy_value(x, want_logits=True)
        assert priors.dtype == torch.float32 and value.dtype == torch.float64 and tuple(priors.shape) == (rows, A) and tuple(value.shape) == (rows,)
        _equal(dict(priors=priors.cpu().numpy(), value=value.cpu().numpy(), logits=logits.cpu().numpy(), bad_rows=None), want, (dims, dtype))
        p2, v2 = mlp(x)                                              # the evaluator's call
        assert p2.cpu().numpy().tobytes() == priors.cpu().numpy().tobytes() and v2.cpu().numpy().tobytes() == value.cpu().numpy().tobytes()
    assert int(mlp.bad_rows.cpu()[0]) == 4 * want["bad_rows"] > 0    # a counter: it adds up over the calls with a head
    # an optimiser-style step in place: the next launch reads the new parameters, nothing was copied
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(0.75).add_(0.015625)
    new = dict(case, weights=[m.weight.detach().cpu().numpy() for m in net if isinstance(m, torch.nn.Linear)],
               biases=[m.bias.detach().cpu().numpy() for m in net if isinstance(m, torch.nn.Linear)])
    moved = rule_of(new)
    x = torch.from_numpy(case["x"]).to(dev)
    y = mlp.forward(x).cpu().numpy()
    _same(y, moved["y"], (dims, "after the update"))
    finite = np.isfinite(want["y"]).all(axis=1) & np.isfinite(moved["y"]).all(axis=1)
    assert (y[finite] != want["y"][finite]).any()
    with pytest.raises(ValueError, match=r"must have shape \(rows, %d\)" % dims[0]):
        mlp.forward(torch.zeros(4, dims[0] + 1, device=dev))
    with pytest.raises(ValueError, match="contiguous torch.float32 or torch.float64"):
        mlp.forward(torch.zeros(4, dims[0], device=dev, dtype=torch.float16))
    with pytest.raises(ValueError, match="must be on"):
        mlp.forward(torch.zeros(4, dims[0]))
    with pytest.raises(ValueError, match="policy_value belongs to a network with a head"):
        DeviceMLP(net).policy_value(x)


def test_the_module_in_float64_torch_stays_within_the_derived_bound():
    """copy.deepcopy(net).double() on the same (float32-rounded) rows against DeviceMLP.forward, within derived_bound() of the host test
    (its docstring derives it; torch's own float64 sums are the `@` of that derivation).  No slack is added."""
    import torch
    from snac_amd import DeviceMLP

    dev = torch.device("cuda", torch.cuda.current_device())
    dims, A, rows = (51, 64, 6), 5, 257
    case = make_mlp_case(np.random.default_rng(case_seed(dims, rows, 1)), dims, rows, A, 1)
    out = rule_of(case)
    good = ~out["bad"] & np.isfinite(out["y"]).all(axis=1)
    net = module_of(case, dev)
    x = torch.from_numpy(case["x"]).to(dev).to(torch.float32)
    y = DeviceMLP(net, A).forward(x).cpu().numpy()[good].astype(np.float64)
    with torch.no_grad():
        ref = copy.deepcopy(net).double()(x.double()).cpu().numpy()[good]
    _, err = derived_bound(case, out, good)
    ratio = np.abs(y - ref) / (err + 1e-300)
    print("largest error / bound against float64 torch: %.3g over %d rows" % (ratio.max(), int(good.sum())))
    assert good.sum() > 128 and ratio.max() <= 1.0
