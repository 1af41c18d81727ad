"""Host: the rule of include/snac_hip.h, "Backward pass of the device network", restated in numpy (mlp_backward_rule), independently of the
kernels (tests/test_gpu_mlp_backward.py compares them byte for byte): the activations are mlp_rule's of tests/test_mlp_host.py, every
delta is one float64 chain over k in order, every gradient a float64 chain over the rows of a chunk and then over the chunks, vectorised
here over rows, units and parameters with a loop per chain step and one ufunc per float64 operation.  Then the inputs the GPU tests run
on (make_backward_case: rows of make_mlp_case's sorts normal, large and zero, a gradient to the outputs, and cancel pairs; that the mask
cuts what it must, that a NaN row reaches the weights it should and no others, and that the stated orders over the batch and over k can
be told from every other association is asserted here), the rule against float64 autograd within a derived bound, the two entry points'
argument checks -- each failing call fails its checks first, so the placeholder pointers are never dereferenced -- and DeviceMLP's
refusals before it touches a device.  Last, the code the kernels run (snac_amd/csrc/mlp_grad_rule.h) is compiled for the host with the
system compiler and compared with mlp_backward_rule byte for byte, and the same source runs once as a program under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os

import numpy as np
import pytest

from cabi_checks import PH, _err_code as _err, _net
import helpers
from hostcode import _vp, load_shared, run_sanitized
from snac_amd import _lib
from specmath import _same
from test_mlp_host import NETS, U24, U53, WIDE, layer_chain, make_mlp_net, mlp_rule

CHUNK = _lib.MLP_GRAD_CHUNK                                          # the header's SNAC_MLP_GRAD_CHUNK: nothing below hard-codes it
BIG = 2.0 ** 40
DIMS = tuple(d for d, _ in NETS)
ROW_SORTS = ("normal", "large", "zero")


# ---- the rule, in numpy: every ufunc call below is one float64 operation, rounded on its own ----------------------------------------------
def _delta_chain(W, up, korder="sequential"):
    """acc float64 [rows, N], the chains of the deltas below a layer: W float32 [K, N], up float32 [rows, K] (the deltas above).  korder:
    the stated order over k, or another association of the same sum."""
    W64, u64 = W.astype(np.float64), up.astype(np.float64)
    K = W.shape[0]
    zero = np.zeros((up.shape[0], W.shape[1]))

    def run(acc, ks):
        for k in ks:
            acc = acc + W64[k][None, :] * u64[:, k][:, None]         # the product is exact: 24 + 24 bits of significand
        return acc

    with np.errstate(all="ignore"):
        if korder == "sequential":
            return run(zero, range(K))
        if korder == "reversed":
            return run(zero, range(K - 1, -1, -1))
        assert korder == "split2"
        acc = zero
        for m in range(min(2, K)):
            acc = acc + run(zero, range(m, K, 2))
        return acc


def _batch_sums(d, h, chunk, order="sequential"):
    """(float64 [N, K], float64 [N]): the totals of a layer's weights and biases from d float32 [rows, N] (the deltas above) and h float32
    [rows, K] (the activations below).  order: the stated one (chunks of `chunk` rows, rows ascending, chunks ascending), the same on the
    rows reversed, or a pairwise tree over all rows."""
    d64, h64 = d.astype(np.float64), h.astype(np.float64)
    rows, N, K = len(d), d.shape[1], h.shape[1]
    idx = list(range(rows))
    if order == "reversed":
        idx.reverse()

    def tw(b):
        return d64[b][:, None] * h64[b][None, :]                     # exact

    def tb(b):
        return d64[b]

    with np.errstate(all="ignore"):
        if order == "pairwise":
            def tree(term, lo, hi):
                if hi - lo == 1:
                    return term(lo)
                mid = (lo + hi) // 2
                return tree(term, lo, mid) + tree(term, mid, hi)
            return np.zeros((N, K)) + tree(tw, 0, rows), np.zeros(N) + tree(tb, 0, rows)
        tot_w, tot_b = np.zeros((N, K)), np.zeros(N)
        for c0 in range(0, rows, chunk):
            part_w, part_b = np.zeros((N, K)), np.zeros(N)
            for b in idx[c0:c0 + chunk]:
                part_w = part_w + tw(b)
                part_b = part_b + tb(b)
            tot_w = tot_w + part_w
            tot_b = tot_b + part_b
    return tot_w, tot_b


def mlp_backward_rule(weights, biases, x, grad_y, chunk, g_old=None, order="sequential", korder="sequential"):
    """-> dict(flat float32 [P]: the gradients in the header's layout; total float64 [P]: before the last rounding; h: [h_0 .. h_L], the
    forward rule's float32 activations; delta: {l: float32 [rows, d_l]} for l = 1 .. L; acc: {l: the float64 chains under delta[l]})."""
    L = len(weights)
    with np.errstate(all="ignore"):
        h = [np.asarray(x).astype(np.float32)] + mlp_rule(weights, biases, x)["acts"]
        delta, accs = {L: np.asarray(grad_y, np.float32)}, {}
        for l in range(L - 1, 0, -1):
            accs[l] = _delta_chain(weights[l], delta[l + 1], korder)
            delta[l] = np.where(h[l] <= np.float32(0.0), np.float32(0.0), accs[l].astype(np.float32))     # a NaN is not <= 0: it passes acc
        totals = []
        for l in range(L):
            tw, tb = _batch_sums(delta[l + 1], h[l], chunk, order)
            totals += [tw.ravel(), tb]
        total = np.concatenate(totals)
        flat = total.astype(np.float32) if g_old is None else (np.asarray(g_old, np.float32).astype(np.float64) + total).astype(np.float32)
    return dict(flat=flat, total=total, h=h, delta=delta, acc=accs)


def num_params(dims):
    return sum(dims[l + 1] * (dims[l] + 1) for l in range(len(dims) - 1))


def layer_views(dims, flat):
    """[(gw [d_{l+1}, d_l], gb [d_{l+1}])] of a flat gradient."""
    out, at = [], 0
    for l in range(len(dims) - 1):
        K, N = dims[l], dims[l + 1]
        out.append((flat[at:at + N * K].reshape(N, K), flat[at + N * K:at + N * K + N]))
        at += N * (K + 1)
    return out


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------------
def cancel_pairs(rows, chunk):
    """The (b1, b2) of the cancel pairs that fit into `rows`: adjacent, the first and the last row of a chunk, the last row of a chunk and
    the first of the next, the first and the last row of the batch."""
    cand = [(2, 3), (0, min(chunk, rows) - 1), (chunk - 1, chunk), (0, rows - 1)]
    return list(dict.fromkeys((a, b) for a, b in cand if 0 <= a < b < rows))


def make_backward_case(rng, dims, rows, chunk=None, cancel=True, sorts=ROW_SORTS):
    """dict(weights, biases, x float64 [rows, dims[0]], grad_y float32 [rows, dims[-1]], sort, dims, pairs, krow).  The rows take the sorts
    of make_mlp_case in turn: normal, large (x 1000) and zero (hidden unit 0 cut to +0.0, unit 1 left at -0.0).  cancel: the rows of
    cancel_pairs() are copies of one input row, and pair p has +2^40 and -2^40 in output column p % d_L of grad_y (a pair whose row holds
    such a value in that column already is left out); and, for a network of two or more layers and four or more outputs, rows 1 and
    d_L - 1 of the last layer's weights are equal and row `krow` of grad_y holds +2^40 and -2^40 there: the order over k of a delta's chain
    then shows as the order over the batch does."""
    dims = tuple(dims)
    chunk = CHUNK if chunk is None else chunk
    weights, biases = make_mlp_net(rng, dims)
    K, L, dL = dims[0], len(dims) - 1, dims[-1]
    x = rng.normal(size=(rows, K))
    sort = [sorts[i % len(sorts)] for i in range(rows)]
    for i, s in enumerate(sort):
        if s == "large":
            x[i] *= 1.0e3
        elif s == "zero" and L >= 2 and dims[1] >= 2:
            x[i] = np.where(np.signbit(weights[0][1]), 0.0, -0.0)
    grad_y = (rng.normal(size=(rows, dL)) / rows).astype(np.float32)
    pairs, krow = [], None
    if cancel:
        used = {}
        for p, (a, b) in enumerate(cancel_pairs(rows, chunk)):
            col = p % dL
            if (a, col) in used or (b, col) in used:
                continue
            used[(a, col)] = used[(b, col)] = True
            pairs.append((a, b, col))
        if pairs:
            base = x[pairs[0][0]].copy() if sort[pairs[0][0]] == "normal" else rng.normal(size=K)
            for a, b, col in pairs:
                x[a], x[b] = base, base
                grad_y[a, col], grad_y[b, col] = BIG, -BIG
                sort[a] = sort[b] = "cancel"
        if L >= 2 and dL >= 4:
            weights[L - 1][dL - 1] = weights[L - 1][1]
            free = [b for b in range(rows) if sort[b] == "normal"]
            if free:
                krow = free[len(free) // 2]
                grad_y[krow, 1], grad_y[krow, dL - 1] = BIG, -BIG
                sort[krow] = "kcancel"
    return dict(weights=weights, biases=biases, x=x, grad_y=grad_y, sort=np.array(sort), dims=dims, pairs=pairs, krow=krow)


def backward_of(c, chunk=None, f64=True, **kw):
    return mlp_backward_rule(c["weights"], c["biases"], c["x"] if f64 else c["x"].astype(np.float32), c["grad_y"], CHUNK if chunk is None else chunk, **kw)


def backward_seed(dims, rows):
    return 77 + 1000 * sum(dims) + 7 * rows


def _differs(a, b):
    return ((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).any()


def test_the_mask_cuts_what_it_must_and_a_nan_row_reaches_the_weights_it_should():
    seen_zero = 0
    for dims in DIMS:
        L = len(dims) - 1
        for rows in (17, CHUNK + 1):
            if dims in WIDE and rows > 17:
                continue
            c = make_backward_case(np.random.default_rng(backward_seed(dims, rows)), dims, rows)
            out = backward_of(c)
            assert out["flat"].tobytes() == backward_of(c, f64=False)["flat"].tobytes()     # the float64 rows round to the float32 rows
            assert out["flat"].shape == (num_params(dims),) and np.isfinite(out["flat"]).all(), dims     # finite rows alone: finite gradients
            for l in range(1, L):
                cut = out["h"][l] <= 0
                assert not out["delta"][l][cut].view(np.uint32).any()                       # exactly +0.0f
                if dims[l] >= 8:
                    assert cut.any() and (out["delta"][l][~cut] != 0).any()
            zero = c["sort"] == "zero"
            if L >= 2 and dims[1] >= 8 and zero.any():
                h1, d1 = out["h"][1][zero], out["delta"][1][zero]
                assert not h1[:, 0].view(np.uint32).any() and (h1[:, 1].view(np.uint32) == 0x80000000).all()
                assert not d1[:, :2].view(np.uint32).any()           # the unit cut to +0.0 and the unit left at -0.0 pass nothing
                if all(d >= 8 for d in dims[1:-1]):                  # (a hidden layer of one unit may cut a whole row off)
                    assert ((d1 != 0) & (h1 > 0)).any(axis=1).all()  # other units of the same rows do
                seen_zero += 1
            # one NaN input: the weights it reaches, and no others
            b = int(np.nonzero(c["sort"] == "normal")[0][0])
            i = dims[0] // 2
            bad = dict(c, x=c["x"].copy())
            bad["x"][b, i] = np.nan
            views = layer_views(dims, backward_of(bad)["flat"])
            gw0, gb0 = views[0]
            assert np.isnan(gw0[:, i]).all() and np.isfinite(np.delete(gw0, i, axis=1)).all() and np.isfinite(gb0).all()
            for gw, gb in views[1:]:                                 # every activation of the row is a NaN, every delta is finite
                assert np.isnan(gw).all() and np.isfinite(gb).all()
    assert seen_zero >= 3


def test_the_stated_order_over_the_batch_shows_in_the_cancel_pairs():
    """Every other association of the sums over the batch -- one chain over all rows, the rows reversed, a pairwise tree, chunks of C / 2
    and of 2 C rows -- changes at least one float32 gradient of a batch with the cancel pairs, so kernels that re-associated could not pass
    the byte comparison."""
    for dims in ((7, 4), (51, 64, 6), (51, 65, 1, 9)):
        rows = 2 * CHUNK + 1
        c = make_backward_case(np.random.default_rng(backward_seed(dims, rows)), dims, rows)
        placed = {(a, b) for a, b, _ in c["pairs"]}
        assert placed == {(2, 3), (0, CHUNK - 1), (CHUNK - 1, CHUNK), (0, rows - 1)}, placed
        for a, b, col in c["pairs"]:
            assert np.array_equal(c["x"][a], c["x"][b]) and c["grad_y"][a, col] == BIG and c["grad_y"][b, col] == -BIG
        want = backward_of(c)["flat"]
        assert np.isfinite(want).all()
        for what, kw in (("one chain", dict(chunk=rows)), ("reversed", dict(order="reversed")), ("pairwise", dict(order="pairwise")),
                         ("C / 2", dict(chunk=CHUNK // 2)), ("2 C", dict(chunk=2 * CHUNK))):
            assert _differs(backward_of(c, **kw)["flat"], want), (dims, what)


def test_the_stated_order_of_a_delta_chain_shows_in_the_generated_inputs():
    told = 0
    for dims in ((51, 64, 6), (502, 256, 256, 6), (512, 256, 255, 64)):
        rows = 17
        c = make_backward_case(np.random.default_rng(backward_seed(dims, rows)), dims, rows)
        L, dL, k = len(dims) - 1, dims[-1], c["krow"]
        assert k is not None and np.array_equal(c["weights"][L - 1][1], c["weights"][L - 1][dL - 1])
        assert c["grad_y"][k, 1] == BIG and c["grad_y"][k, dL - 1] == -BIG
        want = backward_of(c)
        for korder in ("reversed", "split2"):
            got = backward_of(c, korder=korder)
            assert _differs(got["delta"][L - 1][k], want["delta"][L - 1][k]), (dims, korder, "delta")
            assert _differs(got["flat"], want["flat"]), (dims, korder)
            told += 1
    assert told == 6


def accumulate_case():
    """(case, g_old): the network [1, 1] on two rows whose bias gets the total 1 + 2^-25, added to a g_old of 2^24.  In float64 the sum
    lies above the middle of 2^24 and 2^24 + 2 and rounds up; rounded to float32 first the total is 1, the sum in float32 a tie, and the
    result 2^24."""
    c = dict(weights=[np.array([[0.5]], np.float32)], biases=[np.array([0.25], np.float32)], x=np.array([[3.0], [5.0]]),
             grad_y=np.array([[1.0], [2.0 ** -25]], np.float32), dims=(1, 1), sort=np.array(["normal"] * 2), pairs=[], krow=None)
    return c, np.array([0.0, 2.0 ** 24], np.float32)


def test_accumulate_adds_in_float64_and_rounds_once():
    c, g_old = accumulate_case()
    plain, acc = backward_of(c), backward_of(c, g_old=g_old)
    assert plain["total"][1] == 1.0 + 2.0 ** -25 and plain["flat"][1] == 1.0
    assert acc["flat"][1] == 2.0 ** 24 + 2.0 and (g_old + plain["flat"])[1] == 2.0 ** 24       # rounding first and adding in float32 is another result
    dims, rows = (51, 64, 6), 17
    rng = np.random.default_rng(5)
    c = make_backward_case(rng, dims, rows, cancel=False)
    g_old = (2.0 ** 20 * (1.0 + rng.random(num_params(dims)))).astype(np.float32) * np.where(rng.random(num_params(dims)) < 0.5, -1, 1).astype(np.float32)
    plain = backward_of(c)
    assert np.array_equal(backward_of(c, g_old=g_old)["flat"], (g_old.astype(np.float64) + plain["total"]).astype(np.float32))
    assert np.array_equal(backward_of(c, g_old=np.zeros_like(g_old))["flat"], plain["flat"])


# ---- against float64 autograd ------------------------------------------------------------------------------------------------------------
def backward_bound(c, out):
    """(keep bool [rows], err float64 [P]): the rows whose reference pre-activations all lie further from zero than the forward bound, and
    -- computed on the batch of those rows alone, which `out` must be the rule of -- the bound on every gradient's distance from the
    float64 reference (the docstring of the test below derives it).  Called twice: once on the whole batch for `keep`, once on the kept
    rows for `err`."""
    weights, biases = c["weights"], c["biases"]
    L = len(weights)
    rows = len(c["x"])
    with np.errstate(all="ignore"):
        # forward: derived_bound's recurrence of tests/test_mlp_host.py, layer by layer, with the reference's pre-activations
        h = out["h"]
        ref = h[0].astype(np.float64)
        err_h = [np.zeros_like(ref)]
        keep = np.ones(rows, bool)
        for l, (W, b) in enumerate(zip(weights, biases)):
            W64, b64 = W.astype(np.float64), b.astype(np.float64)
            K = W.shape[1]
            x64 = h[l].astype(np.float64)
            size = np.abs(b64)[None, :] + np.abs(x64) @ np.abs(W64).T
            acc = layer_chain(W, b, h[l])
            err = (K + 2) * U53 * size + U24 * np.abs(acc) + err_h[l] @ np.abs(W64).T
            pre = ref @ W64.T + b64[None, :]
            if l < L - 1:
                keep &= (np.abs(pre) > err).all(axis=1)
                ref = np.maximum(pre, 0.0)
            err_h.append(err)
        # backward: the deltas downward, then every sum over the batch
        chunks = -(-rows // CHUNK)
        err_d = {L: np.zeros((rows, weights[-1].shape[0]))}
        for l in range(L - 1, 0, -1):
            W64 = np.abs(weights[l].astype(np.float64))
            K = weights[l].shape[0]
            d64 = np.abs(out["delta"][l + 1].astype(np.float64))
            err_d[l] = (K + 2) * U53 * (d64 @ W64) + U24 * np.abs(out["acc"][l]) + err_d[l + 1] @ W64
        errs, at = [], 0
        for l in range(L):
            d64, h64 = np.abs(out["delta"][l + 1].astype(np.float64)), np.abs(h[l].astype(np.float64))
            N, K = d64.shape[1], h64.shape[1]
            tot_w = np.abs(out["total"][at:at + N * K]).reshape(N, K)
            tot_b = np.abs(out["total"][at + N * K:at + N * K + N])
            at += N * (K + 1)
            ed, eh = err_d[l + 1], err_h[l] if l > 0 else np.zeros_like(h64)
            ew = (rows + chunks + 2) * U53 * (d64.T @ h64) + U24 * tot_w + ed.T @ h64 + d64.T @ eh + ed.T @ eh
            eb = (rows + chunks + 2) * U53 * d64.sum(axis=0) + U24 * tot_b + ed.sum(axis=0)
            errs += [ew.ravel(), eb]
    return keep, np.concatenate(errs)


def autograd_reference(c):
    """The flat gradient of sum(y * grad_y) of the module in float64 torch on the CPU, on the float32-rounded rows."""
    import torch

    ws = [torch.tensor(w.astype(np.float64), requires_grad=True) for w in c["weights"]]
    bs = [torch.tensor(b.astype(np.float64), requires_grad=True) for b in c["biases"]]
    h = torch.tensor(c["x"].astype(np.float32).astype(np.float64))
    for l, (w, b) in enumerate(zip(ws, bs)):
        h = torch.nn.functional.linear(h, w, b)
        if l < len(ws) - 1:
            h = torch.relu(h)
    (h * torch.tensor(c["grad_y"].astype(np.float64))).sum().backward()
    return np.concatenate([np.concatenate([w.grad.numpy().ravel(), b.grad.numpy()]) for w, b in zip(ws, bs)])


def bound_case(dims, rows=257):
    """The batch of the comparison with float64 autograd: normal and large rows, no cancel pairs; the rows that may take the other branch
    of the mask left out of the batch handed to both sides.  -> (case, rows generated)."""
    c = make_backward_case(np.random.default_rng(backward_seed(dims, rows) + 1), dims, rows, cancel=False, sorts=ROW_SORTS[:2])
    keep, _ = backward_bound(c, backward_of(c))
    kept = dict(c, x=c["x"][keep], grad_y=c["grad_y"][keep], sort=c["sort"][keep])
    return kept, rows


def test_the_rule_stays_within_the_derived_bound_of_float64_autograd():
    """The reference is the module in float64 torch on the CPU, loss = sum(y * grad_y), on the rule's float32-rounded rows.  The bound is
    derived, not fitted to what is seen (which is printed).  Forward, err_h of layer l + 1 is derived_bound's of tests/test_mlp_host.py:
    (K + 2) 2^-53 (|b| + |W||h|) + 2^-24 |acc| + |W| err_h, and 0 for the input.  A row whose reference pre-activation lies within that bound of zero at some hidden unit may take
    the other branch of the mask in the rule than in the reference; such a row is left out of the batch handed to BOTH sides, at most 2 %
    of the rows may be, and at least 128 rows are compared per network.  For the rows left in, mask and reference agree, and downward
        err_delta_L = 0        (grad_y is the same on both sides)
        err_delta_l = (K + 2) 2^-53 |W_l|^T |delta_{l+1}| + 2^-24 |acc| + |W_l|^T err_delta_{l+1}
    -- K exact products and K additions, each within 2^-53 of a partial sum that is at most |W|^T |delta|, the same for the reference's own
    sum; the rounding of acc to float32; the error of the deltas above through the layer (a masked unit is 0 on both sides).  For a weight,
    with `rows` additions within the chunks and `chunks` over them,
        (rows + chunks + 2) 2^-53 sum_b |delta||h| + 2^-24 |total| + sum_b (err_delta |h| + |delta| err_h + err_delta err_h)
    and for a bias the same with h = 1 and err_h = 0."""
    worst, compared = 0.0, 0
    for dims in DIMS:
        c, generated = bound_case(dims)
        kept = len(c["x"])
        assert generated - kept <= 0.02 * generated and kept >= 128, (dims, generated, kept)
        out = backward_of(c)
        keep, err = backward_bound(c, out)
        assert keep.all()
        ref = autograd_reference(c)
        ratio = np.abs(out["flat"].astype(np.float64) - ref) / (err + 1e-300)
        assert ratio.max() <= 1.0, (dims, ratio.max(), int(ratio.argmax()))
        worst, compared = max(worst, ratio.max()), compared + kept
        print("%s: %d of %d rows compared, largest error / bound %.3g" % (list(dims), kept, generated, ratio.max()))
    print("largest error / bound: %.3g over %d rows" % (worst, compared))
    assert compared >= 128 * len(DIMS)


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------
def work_bytes_formula(dims, rows):
    """What the header states: 8 * chunks * P + 4 * rows * 2 * (d_1 + .. + d_{L-1})."""
    return 8 * (-(-rows // CHUNK)) * num_params(dims) + 4 * rows * 2 * sum(dims[1:-1])


def _wb(L, net, rows):
    return L.snac_mlp_backward_work_bytes(C.byref(net) if net is not None else None, rows)


def _bwd(L, net=None, x=PH, f64=0, rows=4, grad_y=PH, grad=PH, accumulate=0, work=PH, work_bytes=1 << 40):
    return L.snac_mlp_backward(C.byref(net) if net is not None else None, x, f64, rows, grad_y, grad, accumulate, work, work_bytes, None)


def test_the_library_exports_the_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    vp, net = C.c_void_p, C.POINTER(_lib.Mlp)
    P = _lib.PROTOTYPES
    assert P["snac_mlp_backward_work_bytes"] == (C.c_int64, [net, C.c_int32])
    assert P["snac_mlp_backward"] == (C.c_int, [net, vp, C.c_int, C.c_int32, vp, vp, C.c_int32, vp, C.c_int64, vp])
    assert all(n in _lib.EXPORTS for n in ("snac_mlp_backward_work_bytes", "snac_mlp_backward"))
    assert CHUNK in (64, 128, 256, 512) and _lib.CONSTANTS["SNAC_MLP_GRAD_CHUNK"] == CHUNK


def test_work_bytes_is_the_formula_of_the_header_and_refuses_bad_networks():
    L = _lib.lib()
    for dims in DIMS + ((512, 256, 256, 256, 64),):
        last, chunks = 0, 0
        for rows in (1, 16, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 65536, (1 << 31) - 1):
            got = _wb(L, _net(dims), rows)
            assert got == work_bytes_formula(dims, rows), (dims, rows, got)
            grows = len(dims) > 2 or -(-rows // CHUNK) > chunks       # with every row where rows are parked, else with every chunk
            assert got > last if grows else got == last, (dims, rows, got, last)
            last, chunks = got, -(-rows // CHUNK)
    assert _wb(L, _net((51, 64, 6), w=[0, 0], b=[0, 0]), 4) == work_bytes_formula((51, 64, 6), 4)  # host only: the pointers are not looked at
    _err(L, _wb(L, None, 4), -1, b"null net")
    for layers in (0, -1, 5):
        _err(L, _wb(L, _net(layers=layers), 4), -1, b"layers must be 1 .. 4")
    for d0 in (0, -1, 513):
        _err(L, _wb(L, _net((d0, 64, 6)), 4), -1, b"dim[0]")
    for hidden in (0, 257, -4):
        _err(L, _wb(L, _net((51, hidden, 6)), 4), -1, b"a hidden width must be 1 .. 256")
    for last in (0, 65, -1):
        _err(L, _wb(L, _net((51, 64, last)), 4), -1, b"dim[layers]")
    for rows in (0, -1, -(1 << 31)):
        _err(L, _wb(L, _net(), rows), -1, b"rows must be >= 1")


def test_backward_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    odd4, odd8 = C.c_void_p((1 << 20) + 2), C.c_void_p((1 << 20) + 4)
    ok = _net()
    _err(L, _bwd(L, None), -1, b"null net")
    for layers in (0, -1, 5):
        _err(L, _bwd(L, _net(layers=layers)), -1, b"layers must be 1 .. 4")
    for d0 in (0, -1, 513):
        _err(L, _bwd(L, _net((d0, 64, 6))), -1, b"dim[0]")
    for hidden in (0, 257, -4):
        _err(L, _bwd(L, _net((51, hidden, 6))), -1, b"a hidden width must be 1 .. 256")
        _err(L, _bwd(L, _net((51, 64, hidden, 6))), -1, b"a hidden width must be 1 .. 256")
    for last in (0, 65, -1):
        _err(L, _bwd(L, _net((51, 64, last))), -1, b"dim[layers]")
    _err(L, _bwd(L, _net(w=[1 << 20, 0])), -1, b"null weights / bias")
    _err(L, _bwd(L, _net(b=[0, 1 << 20])), -1, b"null weights / bias")
    _err(L, _bwd(L, _net(w=[(1 << 20) + 2, 1 << 20])), -1, b"4-byte aligned")
    _err(L, _bwd(L, _net(b=[1 << 20, (1 << 20) + 1])), -1, b"4-byte aligned")
    _err(L, _bwd(L, ok, x=None), -1, b"null x")
    _err(L, _bwd(L, ok, x=odd4), -1, b"x must be aligned")
    _err(L, _bwd(L, ok, f64=1, x=odd8), -1, b"x must be aligned")
    _err(L, _bwd(L, ok, f64=2), -1, b"x_is_f64 must be 0 or 1")
    for rows in (0, -1, -(1 << 31)):
        _err(L, _bwd(L, ok, rows=rows), -1, b"rows must be >= 1")
    _err(L, _bwd(L, ok, grad_y=None), -1, b"null grad_y / grad")
    _err(L, _bwd(L, ok, grad=None), -1, b"null grad_y / grad")
    _err(L, _bwd(L, ok, grad_y=odd4), -1, b"grad_y and grad must be 4-byte aligned")
    _err(L, _bwd(L, ok, grad=odd4), -1, b"grad_y and grad must be 4-byte aligned")
    for accumulate in (2, -1):
        _err(L, _bwd(L, ok, accumulate=accumulate), -1, b"accumulate must be 0 or 1")
    _err(L, _bwd(L, ok, work=None), -1, b"null work")
    _err(L, _bwd(L, ok, work=odd8), -1, b"work must be 8-byte aligned")
    need = work_bytes_formula((51, 64, 6), 4)
    for short in (need - 1, 0, -1):
        _err(L, _bwd(L, ok, work_bytes=short), -1, b"work_bytes")
    _err(L, _bwd(L, _net((512, 256, 256, 256, 64)), rows=65536, work_bytes=work_bytes_formula((512, 256, 256, 256, 64), 65536) - 1), -1, b"work_bytes")


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------------
def hostless_mlp(dims):
    """A DeviceMLP bound to cuda:0 whose parameters lie on the host (its constructor refuses them: the fields are set here): every
    refusal of backward() and train_forward() comes before the device or the library is touched, so it needs neither."""
    import torch
    from snac_amd import DeviceMLP

    mlp = DeviceMLP.__new__(DeviceMLP)
    mlp.dims, mlp.device, mlp.num_actions = tuple(dims), torch.device("cuda", 0), None
    mlp._params = [(torch.zeros(dims[l + 1], dims[l], requires_grad=True), torch.zeros(dims[l + 1], requires_grad=True)) for l in range(len(dims) - 1)]
    mlp._lib = mlp._net = mlp._bad = mlp._work = None
    return mlp


def test_device_mlp_backward_refuses_before_it_touches_a_device():
    import torch

    dims = (51, 64, 6)
    mlp = hostless_mlp(dims)
    P = num_params(dims)
    assert mlp.num_params == P
    x, gy = torch.zeros(4, 51), torch.zeros(4, 6)
    for bad, words in ((torch.zeros(4, 50), r"x must have shape \(rows, 51\)"), (torch.zeros(0, 51), r"x must have shape"),
                       (torch.zeros(4, 51, dtype=torch.float16), "contiguous torch.float32 or torch.float64"),
                       (torch.zeros(51, 4).t(), "contiguous torch.float32 or torch.float64"), (np.zeros((4, 51), np.float32), "contiguous torch.float32")):
        with pytest.raises(ValueError, match=words):
            mlp.backward(bad, gy)
        with pytest.raises(ValueError, match=words):
            mlp.train_forward(bad)
    for bad in (torch.zeros(4, 5), torch.zeros(5, 6), torch.zeros(4, 6, dtype=torch.float64), torch.zeros(6, 4).t(), torch.zeros(24), None):
        with pytest.raises(ValueError, match=r"grad_y must be a contiguous torch.float32 tensor of shape \(4, 6\)"):
            mlp.backward(x, bad)
    with pytest.raises(ValueError, match="accumulate=True needs out"):
        mlp.backward(x, gy, accumulate=True)
    with pytest.raises(ValueError, match="accumulate must be True or False"):
        mlp.backward(x, gy, accumulate=1, out=torch.zeros(P))
    for bad in (torch.zeros(P + 1), torch.zeros(P, dtype=torch.float64), torch.zeros(2 * P)[::2], torch.zeros(1, P), [0.0] * P):
        with pytest.raises(ValueError, match=r"out must be a contiguous torch.float32 tensor of shape \(%d,\)" % P):
            mlp.backward(x, gy, out=bad)
    with pytest.raises(ValueError, match="x must be on cuda:0"):
        mlp.backward(x, gy)                                          # everything else is in order: the rows are on the host
    with pytest.raises(ValueError, match="x must be on cuda:0"):
        mlp.backward(x, gy, accumulate=True, out=torch.zeros(P))
    with pytest.raises(ValueError, match="x must be on cuda:0"):
        mlp.train_forward(x)
    views = mlp._views(torch.arange(P, dtype=torch.float32))
    assert [tuple(gw.shape) + tuple(gb.shape) for gw, gb in views] == [(64, 51, 64), (6, 64, 6)]
    assert float(views[0][1][0]) == 64 * 51 and float(views[1][0][0, 0]) == 64 * 52 and float(views[1][1][-1]) == P - 1


# ---- the kernels' code on the host -------------------------------------------------------------------------------------------------------
HOST_SRC = os.path.join(helpers.TESTS, "native", "mlp_grad_host.cpp")
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", _lib.CSRC, HOST_SRC]
HOST_NETS = ((7, 4), (51, 64, 6), (51, 65, 1, 9), (502, 256, 256, 6))


def test_the_kernels_code_compiled_for_the_host_equals_the_rule_byte_for_byte(tmp_path):
    fn = load_shared(tmp_path, "mlp_grad_host", ["-O2", "-fPIC", "-shared"] + HOST_FLAGS, timeout=600).mlp_grad_host
    vp = C.c_void_p
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, vp, vp, vp, vp, C.c_int, C.c_int32, vp, C.c_int32, C.c_int32, vp]
    for dims in HOST_NETS:
        P = num_params(dims)
        for rows in (1, 17, CHUNK + 1):
            rng = np.random.default_rng(backward_seed(dims, rows))
            c = make_backward_case(rng, dims, rows)
            g_old = rng.normal(size=P).astype(np.float32)
            want = backward_of(c)["flat"], backward_of(c, g_old=g_old)["flat"]
            L = len(dims) - 1
            dim = np.array(list(dims) + [0] * (5 - len(dims)), np.int32)
            wp, bp = (vp * 4)(*[_vp(w) for w in c["weights"]]), (vp * 4)(*[_vp(x) for x in c["biases"]])
            for f64 in (0, 1):
                x = np.ascontiguousarray(c["x"] if f64 else c["x"].astype(np.float32))
                for accumulate in (0, 1):
                    grad = g_old.copy() if accumulate else np.full(P, 7, np.float32)
                    assert fn(L, _vp(dim), wp, bp, _vp(x), f64, rows, _vp(c["grad_y"]), CHUNK, accumulate, _vp(grad)) == P
                    _same(grad, want[accumulate], (dims, rows, f64, accumulate))
    assert fn(1, _vp(np.array([513, 4, 0, 0, 0], np.int32)), None, None, None, 0, 1, None, CHUNK, 0, None) == -1


def test_the_kernels_code_runs_clean_under_the_host_sanitizers(tmp_path):
    """A stand-alone program (mlp_grad_host.cpp with its main), not code loaded into python."""
    r = run_sanitized(tmp_path, "mlp_grad_host_main", ["-DMLP_GRAD_HOST_MAIN"] + HOST_FLAGS, probe_timeout=300, build_timeout=600, run_timeout=300)
    assert r.stdout.count(", off 0") == 7 * 4 * 2 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
