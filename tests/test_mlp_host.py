"""Host: the rule of include/snac_hip.h, "Policy / value network on the device", restated in numpy (mlp_rule), independently of the kernel
(tests/test_gpu_mlp.py and tests/test_gpu_uct_mlp.py compare them byte for byte): every output of a layer is one float64 chain in index
order, vectorised here over rows and outputs with a loop over i and one ufunc per operation; the head is the softmax of "Acting from a
policy" (spec_exp of tests/test_policy_act_host.py).  Then the inputs the GPU tests run on (make_mlp_case: that every sort of row lands
in the branch it is meant for, that the number of bad rows follows from the generator alone, and that the stated order of a sum can be
told from the reversed, the pairwise and the 2-, 4- and 64-way split sums, is asserted here), the rule against plain float64 `@` within
a derived bound, the three entry points' argument checks -- each failing call fails its checks first, so the placeholder pointers are
never dereferenced -- and DeviceMLP's refusals before it touches a device.  Last, the code the kernel runs (snac_amd/csrc/mlp_rule.h) is
compiled for the host with the system compiler and compared with mlp_rule byte for byte, and the same source runs once as a program
under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os

import numpy as np
import pytest

from cabi_checks import PH, _err_code as _err, _net
import helpers
from hostcode import _vp, load_shared, run_sanitized
from snac_amd import _lib
from specmath import _same, spec_exp

BIG = 2.0 ** 60
HUGE = 3.0e38                                                        # a float32 whose sums with its like overflow float32, not float64
# the networks of the GPU tests: (dims, num_actions or None)
NETS = (((7, 4), 3), ((51, 64, 6), 5), ((51, 65, 1, 9), 8), ((502, 256, 256, 6), 5), ((512, 256, 255, 64), None), ((1, 1), None))
WIDE = (NETS[3][0], NETS[4][0])                                      # run at rows <= 257 only: the numpy loop stays within seconds
ROWS = (1, 63, 64, 65, 257, 4097)
SORTS = ("normal", "cancel", "large", "zero", "overflow", "nan", "value_bad", "cancel")
BAD = ("overflow", "nan", "value_bad")
HEADS = ("plain", "masked", "all_masked")


# ---- the rule, in numpy: every ufunc call below is one float64 operation, rounded on its own ----------------------------------------------
def layer_chain(W, b, x, order="sequential"):
    """acc [rows, N] float64 of one layer: W float32 [N, K], b float32 [N], x float32 [rows, K].  order: the stated one, or another
    association of the same sum (for the assertion that the generated inputs tell them apart)."""
    W64, x64 = W.astype(np.float64), x.astype(np.float64)
    K = W.shape[1]
    start = np.broadcast_to(b.astype(np.float64)[None, :], (x.shape[0], W.shape[0]))

    def term(i):
        return W64[None, :, i] * x64[:, i, None]                     # exact: 24 + 24 bits of significand

    def run(acc, idx):
        for i in idx:
            acc = acc + term(i)
        return acc

    with np.errstate(all="ignore"):
        if order == "sequential":
            return run(start, range(K))
        if order == "reversed":
            return run(start, range(K - 1, -1, -1))
        if order == "pairwise":
            def tree(lo, hi):
                if hi - lo == 1:
                    return term(lo)
                mid = (lo + hi) // 2
                return tree(lo, mid) + tree(mid, hi)
            return start + tree(0, K)
        ways = int(order[len("split"):])                             # `ways` partial sums over i = m, m + ways, ..., added to b in turn
        acc = start
        for m in range(min(ways, K)):
            acc = acc + run(np.zeros_like(start), range(m, K, ways))
        return acc


def mlp_rule(weights, biases, x, num_actions=None, order="sequential"):
    """-> dict(y float32 [rows, dims[-1]], acts: the float32 activations of every layer; with num_actions: priors float32 [rows, A],
    value float64 [rows], bad bool [rows], bad_rows int)."""
    with np.errstate(all="ignore"):
        h = np.asarray(x).astype(np.float32)                         # float64 rows are rounded to float32 first
        acts = []
        for l, (W, b) in enumerate(zip(weights, biases)):
            acc = layer_chain(W, b, h, order)
            if l == len(weights) - 1:
                h = acc.astype(np.float32)
            else:
                h = np.where(acc < 0.0, np.float32(0.0), acc.astype(np.float32))     # a NaN is not < 0: it stays; so does -0.0
            acts.append(h)
        out = dict(y=h, acts=acts)
        if num_actions is None:
            return out
        A = num_actions
        assert h.shape[1] == A + 1
        l = h[:, :A]
        m = l[:, 0].copy()
        for a in range(1, A):
            m = np.where(l[:, a] > m, l[:, a], m)
        bad = np.isnan(l).any(axis=1) | (l == np.inf).any(axis=1) | (m == -np.inf) | ~np.isfinite(h[:, A])
        ls, ms = np.where(bad[:, None], np.float32(0.0), l), np.where(bad, np.float32(0.0), m)
        xs = ls.astype(np.float64) - ms.astype(np.float64)[:, None]
        e = spec_exp(xs)
        S = np.zeros(len(h))
        for a in range(A):
            S = S + e[:, a]
        priors = np.where(bad[:, None], np.float32(0.0), (e / S[:, None]).astype(np.float32))
        value = np.where(bad, 0.0, h[:, A].astype(np.float64))
    out.update(priors=priors, value=value, bad=bad, bad_rows=int(bad.sum()))
    return out


def leaves_rule(out, first_has, first_idx, done, stats, terminal_word, leaf, est):
    """The fused step of the search on mlp_rule's `out` -> (value, est): indices clamped into range, one float64 addition."""
    S = len(leaf)
    f = np.clip(first_idx, 0, S - 1)
    n = np.clip(leaf, 0, len(stats) - 1)
    term = np.where(first_has != 0, done[f] != 0, stats[n, terminal_word] != 0)
    value = np.where(term, 0.0, out["value"])
    return value, est + value


# ---- the inputs of the GPU tests: the sorts of row take turns, row i of sort (i + shift) % len(SORTS) -------------------------------------
def cancel_places(K):
    """The input columns that share one column of layer 0's weights, and the (first, second) places of +2^60 and -2^60 of the cancel
    rows: adjacent, 32, 64 and 65 apart, first to last, the last two."""
    P = sorted({p for p in (0, 1, 32, 64, 65, K - 2, K - 1) if 0 <= p < K})
    pairs = [(a, b) for a, b in ((0, 1), (0, 32), (0, 64), (0, 65), (0, K - 1), (K - 2, K - 1), (1, 65)) if a in P and b in P and a < b]
    return P, list(dict.fromkeys(pairs))


def channel_of(dims, A):
    """Whether the network carries input 2 alone to the value output (value_bad rows): it needs a head, input 2 outside the shared
    columns and every hidden layer at least 4 wide."""
    return A is not None and dims[0] > 2 and 2 not in cancel_places(dims[0])[0] and all(d >= 4 for d in dims[1:-1])


def make_mlp_net(rng, dims, A=None, head="plain"):
    """(weights, biases) float32: N(0, 1 / K) weights, small biases, and what the sorts of make_mlp_case need: the columns of
    cancel_places() of layer 0 equal, so that +2^60 and -2^60 there cancel in every output of the layer at once; biases +0.0 and -0.0 of
    the first two hidden units; with channel_of(): input 2 feeds hidden unit 3 alone, which every hidden layer hands on unchanged to the
    value output, weight 4.  head "masked": the bias of one or two logits is -inf; "all_masked": of every logit."""
    L = len(dims) - 1
    weights = [(rng.normal(size=(dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32) for l in range(L)]
    biases = [(0.1 * rng.normal(size=dims[l + 1])).astype(np.float32) for l in range(L)]
    P, _ = cancel_places(dims[0])
    weights[0][:, P] = weights[0][:, [0]]
    if L >= 2 and dims[1] >= 2:
        biases[0][0], biases[0][1] = 0.0, -0.0
    if channel_of(dims, A):
        if L == 1:
            weights[0][:, 2] = 0.0
            weights[0][A, 2] = 4.0
        else:
            weights[0][:, 2] = 0.0
            weights[0][3, :] = 0.0
            weights[0][3, 2], biases[0][3] = 1.0, 0.0
            for l in range(1, L - 1):
                weights[l][3, :] = 0.0
                weights[l][3, 3], biases[l][3] = 1.0, 0.0
            weights[L - 1][A, 3] = 4.0
    if head != "plain":
        assert A is not None
        masked = range(A) if head == "all_masked" else sorted(rng.choice(A, size=1 + int(rng.integers(2)), replace=False))
        for a in masked:
            biases[L - 1][a] = -np.inf
    return weights, biases


def make_mlp_case(rng, dims, rows, A=None, shift=0, head="plain"):
    """dict(weights, biases, x float64 [rows, dims[0]] (a float32 input is x.astype(float32): the same rows after the rule's rounding),
    sort: the rows' sorts, dims, A, head)."""
    dims = tuple(dims)
    weights, biases = make_mlp_net(rng, dims, A, head)
    K, L = dims[0], len(dims) - 1
    W0 = weights[0]
    x = rng.normal(size=(rows, K))
    sorts = [SORTS[(i + shift) % len(SORTS)] for i in range(rows)]
    _, pairs = cancel_places(K)
    unit = (A if A is not None else dims[1] - 1) if L == 1 else min(2, dims[1] - 1)      # the output that the overflow rows drive to +inf
    cancels = 0
    for i, sort in enumerate(sorts):
        if sort == "large":
            x[i] *= 1.0e3
        elif sort == "zero" and L >= 2 and dims[1] >= 2:             # every product of hidden unit 1 is -0.0, its bias too
            x[i] = np.where(np.signbit(W0[1]), 0.0, -0.0)            # also where the weight is a zero: its sign counts
        elif sort == "overflow" or (sort == "value_bad" and not channel_of(dims, A)):
            x[i] = HUGE * np.where(W0[unit] < 0, -1.0, 1.0)
        elif sort == "nan":
            x[i, int(rng.integers(K))] = np.nan
        elif sort == "value_bad":
            x[i, 2] = 2.0e38
        elif sort == "cancel" and pairs:
            a, b = pairs[(cancels + shift) % len(pairs)]
            cancels += 1
            x[i, a], x[i, b] = BIG, -BIG
    return dict(weights=weights, biases=biases, x=x, sort=np.array(sorts), dims=dims, A=A, head=head)


def bad_rows_of(rows, shift=0, head="plain"):
    """From the generator alone: how many rows of make_mlp_case(rng, dims, rows, A, shift, head) the head refuses."""
    return rows if head == "all_masked" else sum(SORTS[(i + shift) % len(SORTS)] in BAD for i in range(rows))


def rule_of(c, order="sequential", f64=True):
    return mlp_rule(c["weights"], c["biases"], c["x"] if f64 else c["x"].astype(np.float32), c["A"], order)


def case_seed(dims, rows, shift=0, head="plain"):
    return 1000 * sum(dims) + 7 * rows + shift + 100000 * HEADS.index(head)


def rows_of(dims):
    return tuple(r for r in ROWS if r <= 257 or tuple(dims) not in WIDE)


def shifts_of(rows):
    return range(len(SORTS)) if rows == 1 else (rows % len(SORTS),)  # a single row takes every sort in turn


def gpu_cases(heads=("plain",)):
    """Every case of tests/test_gpu_mlp.py: (dims, A, rows, shift, head)."""
    for dims, A in NETS:
        for rows in rows_of(dims):
            for head in (heads if A is not None else ("plain",)):
                if head != "plain" and rows not in (1, 65):
                    continue
                for shift in shifts_of(rows):
                    yield dims, A, rows, shift, head


def test_the_generated_inputs_contain_every_sort_in_its_branch_and_bad_rows_follows_from_the_generator():
    seen = set()
    for dims, A, rows, shift, head in gpu_cases(HEADS):
        c = make_mlp_case(np.random.default_rng(case_seed(dims, rows, shift, head)), dims, rows, A, shift, head)
        out = rule_of(c)
        assert np.array_equal(out["y"], rule_of(c, f64=False)["y"], equal_nan=True)      # the float64 rows round to the float32 rows
        sort, L, x32 = c["sort"], len(dims) - 1, c["x"].astype(np.float32)
        first = out["acts"][0]
        normal = sort == "normal"
        finite = np.isfinite(out["y"]).all(axis=1) if head == "plain" else np.ones(rows, bool)      # a masked logit is -inf by design
        assert finite[normal].all()
        if L >= 2 and normal.any() and dims[1] >= 8:                 # ReLU cuts some hidden units of a row to exactly 0 and keeps others
            assert (first[normal] == 0).any() and (first[normal] > 0).any()
        at = sort == "large"
        assert (dims[0] == 1 or (np.abs(x32[at]).max(axis=1) > 100.0).all()) and finite[at].all()
        at = sort == "zero"
        if L >= 2 and dims[1] >= 2 and at.any():
            assert not first[at, 0].view(np.uint32).any() and (first[at, 1].view(np.uint32) == 0x80000000).all()
            assert finite[at].all()
        at = sort == "overflow"
        if at.any() and dims[0] > 1:
            assert (first[at] == np.inf).any(axis=1).all(), dims    # a float32 overflow of the chain's float64 sum
        at = sort == "nan"
        assert np.isnan(out["y"][at]).all()
        if A is not None:
            want = bad_rows_of(rows, shift, head)
            assert out["bad_rows"] == want, (dims, rows, shift, head, out["bad_rows"], want, sort[out["bad"]])
            if head != "all_masked":
                assert set(sort[out["bad"]]) <= set(BAD) and not out["bad"][~np.isin(sort, BAD)].any()
                at = sort == "value_bad"
                assert not np.isfinite(out["y"][at, A]).any()
                if channel_of(dims, A) and head == "plain":          # the value alone: the logits of these rows are finite
                    assert np.isfinite(out["y"][at, :A]).all()
                good = ~out["bad"]
                assert np.allclose(out["priors"][good].sum(axis=1), 1.0, atol=1e-6) and (out["value"][good] == out["y"][good, A]).all()
            if head == "masked":
                masked = np.isneginf(c["biases"][-1][:A])
                assert 1 <= masked.sum() <= 2 and not out["priors"][:, masked].view(np.uint32).any()
                assert out["bad"].all() or (out["priors"][~out["bad"]][:, ~masked] > 0).any()
            assert not out["priors"][out["bad"]].view(np.uint32).any() and not out["value"][out["bad"]].view(np.uint64).any()
            seen |= {head}
        seen |= set(sort)
    assert seen == set(SORTS) | set(HEADS)


def test_the_stated_order_of_a_sum_shows_in_the_generated_inputs():
    """Every other association of a layer's sums -- reversed, pairwise, split 2, 4 and 64 ways -- changes at least one float32 output of
    the cancel rows, so a kernel that re-associated could not pass the byte comparison; an ordinary row almost never tells them apart
    after the rounding to float32.  (A 64-way split of at most 64 terms is the stated order: it is asked of the two wide inputs.)"""
    told = {}
    for dims, A in NETS:
        rows = 65
        c = make_mlp_case(np.random.default_rng(case_seed(dims, rows, rows % len(SORTS))), dims, rows, A, rows % len(SORTS))
        want = rule_of(c)["y"]
        cancel = c["sort"] == "cancel"
        for order in ("reversed", "pairwise", "split2", "split4", "split64"):
            got = mlp_rule(c["weights"], c["biases"], c["x"], None, order)["y"]
            differs = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
            if dims[0] >= 4 and (order != "split64" or dims[0] > 65):
                assert differs[cancel].any(), (dims, order)
                told.setdefault(order, []).append(dims)
    assert all(len(told[o]) >= 2 for o in ("reversed", "pairwise", "split2", "split4", "split64")), told


# ---- against plain float64 ---------------------------------------------------------------------------------------------------------------
U53, U24 = 2.0 ** -53, 2.0 ** -24
EPS_EXP, ROUND, FLOOR = 2e-12, 2.0 ** -48, np.exp(-45.0)             # tests/test_search_loss_host.py's bounds on EXP


def derived_bound(c, out, good):
    """(ref, err) float64 [good rows, dims[-1]]: the last layer's outputs of the float64 reference and the bound on their distance from
    the rule's (the docstring of the test below derives it)."""
    with np.errstate(all="ignore"):
        x = c["x"].astype(np.float32)[good]
        ref = x.astype(np.float64)
        err = np.zeros_like(ref)
        h = x
        L = len(c["weights"])
        for l, (W, b) in enumerate(zip(c["weights"], c["biases"])):
            W64, b64 = W.astype(np.float64), b.astype(np.float64)
            K = W.shape[1]
            size = np.abs(b64)[None, :] + np.abs(h.astype(np.float64)) @ np.abs(W64).T
            acc = layer_chain(W, b, h)
            err = (K + 2) * U53 * size + U24 * np.abs(acc) + err @ np.abs(W64).T
            ref = ref @ W64.T + b64[None, :]
            if l < L - 1:
                ref = np.maximum(ref, 0.0)
            h = out["acts"][l][good]
    return ref, err


def test_the_rule_stays_within_the_derived_bound_of_plain_float64():
    """The reference is h = maximum(W @ h + b, 0) in float64 throughout, a float64 softmax of the first A outputs and the last output as
    the value.  The bound is derived, not fitted to what is seen (which is printed).  Per layer, with x the rule's own float32 input of
    the layer and err_in the bound on its distance from the reference's input:
        the chain: K products (exact) and K additions, each within 2^-53 of its partial sum, which is at most |b| + |W||x|; with the
                   reference's own sum over the same terms that is (K + 2) 2^-53 (|b| + |W||x|) to first order
        the rounding of acc to float32: 2^-24 |acc|
        the input's error through the layer: |W| err_in (ReLU and the rounding move no two values further apart than they were)
    so err_out = (K + 2) 2^-53 (|b| + |W||x|) + 2^-24 |acc| + |W| err_in, and err = 0 for the input.  For the head, with d the largest
    err_out over the row's logits: EXP is within eps = 2e-12 relative, p_a = e_a / S within 2 eps and a few roundings, a shift of the
    logits by at most d moves p_a by at most p_a (exp(2 d) - 1), EXP cuts below -45 where the true probability is up to e^-45, and the
    result is rounded to float32:
        |p_a - ref| <= p_a (2 eps + 2^-48 + 2^-24) + (p_a + 2^-24) (exp(2 d) - 1) + e^-45        (no more than 1)
        |value - ref| <= err_out of output A
    Every good row of every network is compared; none is left out."""
    worst = dict(y=0.0, priors=0.0, value=0.0)
    compared = 0
    for dims, A in NETS:
        rows = 257
        c = make_mlp_case(np.random.default_rng(case_seed(dims, rows, 1)), dims, rows, A, 1)
        out = rule_of(c)
        good = np.isfinite(out["y"]).all(axis=1) & np.isfinite(c["x"]).all(axis=1) if A is None else ~out["bad"] & np.isfinite(out["y"]).all(axis=1)
        ref, err = derived_bound(c, out, good)
        y = out["y"][good].astype(np.float64)
        ratio = np.abs(y - ref) / (err + 1e-300)
        assert ratio.max() <= 1.0, (dims, "y", ratio.max(), c["sort"][good][ratio.max(axis=1).argmax()])
        worst["y"] = max(worst["y"], ratio.max())
        compared += int(good.sum())
        if A is not None:
            z = ref[:, :A] - ref[:, :A].max(axis=1, keepdims=True)
            p_ref = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
            p = out["priors"][good].astype(np.float64)
            d = err[:, :A].max(axis=1, keepdims=True)
            with np.errstate(over="ignore"):
                b_p = np.minimum(1.0, p * (2 * EPS_EXP + ROUND + U24) + (p + U24) * np.expm1(2.0 * d) + FLOOR)
            r_p, r_v = np.abs(p - p_ref) / b_p, np.abs(out["value"][good] - ref[:, A]) / (err[:, A] + 1e-300)
            assert r_p.max() <= 1.0 and r_v.max() <= 1.0, (dims, r_p.max(), r_v.max())
            worst["priors"], worst["value"] = max(worst["priors"], r_p.max()), max(worst["value"], r_v.max())
    print("largest error / bound: outputs %.3g, priors %.3g, value %.3g over %d rows" % (worst["y"], worst["priors"], worst["value"], compared))
    assert compared > 6 * 128


def test_the_fused_step_of_the_search_in_numpy():
    rng = np.random.default_rng(3)
    c = make_mlp_case(rng, (51, 64, 6), 65, 5)
    out = rule_of(c)
    lv = make_leaves(rng, 65, 9)
    value, est = leaves_rule(out, **lv)
    term = value == 0
    assert term.any() and (~term).any() and np.array_equal(est, lv["est"] + value)
    assert (value[~term] == out["value"][~term]).all()


def make_leaves(rng, S, stats_rows, row_words=64, terminal_word=34):
    """The fused step's inputs: terminal and non-terminal slots of both kinds (a leaf made in this iteration, a stored node), indices
    below, inside and past their ranges."""
    first_has = (rng.random(S) < 0.5).astype(np.uint8)
    first_idx = rng.integers(-3, S + 3, size=S).astype(np.int32)
    done = (rng.random(S) < 0.4).astype(np.uint8) * np.uint8(1 + 254 * (rng.random() < 0.5))
    stats = rng.integers(1, 1 << 20, size=(stats_rows, row_words)).astype(np.int32)
    stats[:, terminal_word] = (rng.random(stats_rows) < 0.4) * rng.integers(1, 1 << 30, size=stats_rows)
    leaf = rng.integers(-2, stats_rows + 2, size=S).astype(np.int32)
    est = rng.normal(size=S)
    est[::7] = -0.0
    return dict(first_has=first_has, first_idx=first_idx, done=done, stats=stats, terminal_word=terminal_word, leaf=leaf, est=est)


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------
def _fwd(L, net=None, x=PH, f64=0, rows=4, y=PH):
    return L.snac_mlp_forward(C.byref(net) if net is not None else None, x, f64, rows, y, None)


def _pv(L, net=None, A=5, x=PH, f64=0, rows=4, priors=PH, value=PH, logits=PH, bad=PH):
    return L.snac_mlp_policy_value(C.byref(net) if net is not None else None, A, x, f64, rows, priors, value, logits, bad, None)


def _vl(L, net=None, A=5, obs=PH, f64=0, S=4, first_has=PH, first_idx=PH, done=PH, stats=PH, stats_rows=8, leaf=PH, priors=PH, value=PH, est=PH,
        bad=PH):
    return L.snac_mlp_uct_value_leaves(C.byref(net) if net is not None else None, A, obs, f64, S, first_has, first_idx, done, stats, stats_rows,
                                       leaf, priors, value, est, bad, None)


def test_the_library_exports_the_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    vp, net = C.c_void_p, C.POINTER(_lib.Mlp)
    P = _lib.PROTOTYPES
    assert P["snac_mlp_forward"] == (C.c_int, [net, vp, C.c_int, C.c_int32, vp, vp])
    assert P["snac_mlp_policy_value"] == (C.c_int, [net, C.c_int32, vp, C.c_int, C.c_int32, vp, vp, vp, vp, vp])
    assert P["snac_mlp_uct_value_leaves"] == (C.c_int, [net, C.c_int32, vp, C.c_int, C.c_int32, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp])
    assert all(n in _lib.EXPORTS for n in ("snac_mlp_forward", "snac_mlp_policy_value", "snac_mlp_uct_value_leaves"))
    assert C.sizeof(_lib.Mlp) == 88 and _lib.Mlp.w.offset == 24 and _lib.Mlp.b.offset == 56 and _lib.Mlp.dim.size == 20


def test_the_entry_points_validate_their_arguments_before_any_hip_call():
    L = _lib.lib()
    odd4, odd8 = C.c_void_p((1 << 20) + 2), C.c_void_p((1 << 20) + 4)
    for call in (_fwd, _pv, _vl):
        ok = _net()
        _err(L, call(L, None), -1, b"null net")
        for layers in (0, -1, 5):
            _err(L, call(L, _net(layers=layers)), -1, b"layers must be 1 .. 4")
        for d0 in (0, -1, 513):
            _err(L, call(L, _net((d0, 64, 6))), -1, b"dim[0]")
        for hidden in (0, 257, -4):
            _err(L, call(L, _net((51, hidden, 6))), -1, b"a hidden width must be 1 .. 256")
            _err(L, call(L, _net((51, 64, hidden, 6))), -1, b"a hidden width must be 1 .. 256")
        for last in (0, 65, -1):
            _err(L, call(L, _net((51, 64, last))), -1, b"dim[layers]")
        _err(L, call(L, _net(w=[1 << 20, 0])), -1, b"null weights / bias")
        _err(L, call(L, _net(b=[0, 1 << 20])), -1, b"null weights / bias")
        _err(L, call(L, _net(w=[(1 << 20) + 2, 1 << 20])), -1, b"4-byte aligned")
        _err(L, call(L, _net(b=[1 << 20, (1 << 20) + 1])), -1, b"4-byte aligned")
        _err(L, call(L, ok, **{"obs" if call is _vl else "x": None}), -1, b"null x")
        _err(L, call(L, ok, **{"obs" if call is _vl else "x": odd4}), -1, b"x must be aligned")
        _err(L, call(L, ok, f64=1, **{"obs" if call is _vl else "x": odd8}), -1, b"x must be aligned")
        _err(L, call(L, ok, f64=2), -1, b"x_is_f64 must be 0 or 1")
        for rows in (0, -1, -(1 << 31)):
            _err(L, call(L, ok, **{"S" if call is _vl else "rows": rows}), -1, b"rows must be >= 1")
    ok = _net()
    _err(L, _fwd(L, ok, y=odd4), -1, b"y must be 4-byte aligned")
    assert _fwd(L, ok, y=None) == 0 and _fwd(L, _net((512, 256, 256, 256, 64)), y=None) == 0 and _fwd(L, _net((1, 1)), y=None) == 0
    assert _fwd(L, ok, f64=1, y=None) == 0                          # no output: no launch, although no device exists to launch on
    for call in (_pv, _vl):
        for A in (0, 1, 2, 4, 6, 7, 9, -3):
            _err(L, call(L, ok, A=A), -3, b"num_actions must be 3, 5 or 8")
        _err(L, call(L, ok, A=3), -1, b"dim[layers] must be num_actions + 1")
        _err(L, call(L, _net((51, 64, 5))), -1, b"dim[layers] must be num_actions + 1")
        _err(L, call(L, ok, priors=odd4), -1, b"priors must be 4-byte aligned")
        _err(L, call(L, ok, value=odd8), -1, b"value must be 8-byte aligned")
        _err(L, call(L, ok, bad=odd4), -1, b"bad_rows must be 4-byte aligned")
    _err(L, _pv(L, ok, logits=odd4), -1, b"logits must be 4-byte aligned")
    none = dict(priors=None, value=None, bad=None)
    assert _pv(L, ok, logits=None, **none) == 0 and _pv(L, _net((7, 4)), A=3, logits=None, **none) == 0
    _err(L, _pv(L, ok, rows=0, logits=None, **none), -1, b"rows must be >= 1")
    for k in ("first_has", "first_idx", "done", "stats", "leaf"):
        _err(L, _vl(L, ok, **{k: None}), -1, b"null first_has / first_idx / done / stats / leaf")
    for k in ("first_idx", "stats", "leaf"):
        _err(L, _vl(L, ok, **{k: odd4}), -1, b"first_idx, stats and leaf must be 4-byte aligned")
    for n in (0, -1):
        _err(L, _vl(L, ok, stats_rows=n), -1, b"stats_rows must be >= 1")
    _err(L, _vl(L, ok, est=odd8), -1, b"est must be 8-byte aligned")
    assert _vl(L, ok, est=None, **none) == 0 and _vl(L, _net((51, 65, 1, 9)), A=8, est=None, **none) == 0
    _err(L, _vl(L, ok, leaf=None, est=None, **none), -1, b"null first_has")


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------------
def test_device_mlp_refuses_bad_modules_and_devices_before_it_touches_a_device():
    import torch
    from snac_amd import DeviceMLP

    nn = torch.nn
    net = nn.Sequential(nn.Linear(51, 64), nn.ReLU(), nn.Linear(64, 6))
    with pytest.raises(ValueError, match="cuda device"):
        DeviceMLP(net, 5)                                            # the parameters are on the cpu
    with pytest.raises(ValueError, match="must be a contiguous torch.float32 tensor on cuda:0"):
        DeviceMLP(net, 5, device="cuda:0")
    for bad, words in ((nn.Sequential(), "empty"), (nn.Sequential(nn.Linear(5, 6), nn.ReLU()), "ends in a ReLU"),
                       (nn.Sequential(nn.Linear(5, 8), nn.Tanh(), nn.Linear(8, 6)), "module 1 is Tanh: a ReLU belongs"),
                       (nn.Sequential(nn.Linear(5, 8), nn.Linear(8, 6)), "module 1 is Linear: a ReLU belongs"),
                       (nn.Sequential(nn.ReLU(), nn.Linear(5, 6)), "module 0 is ReLU: a Linear belongs"),
                       (nn.Sequential(nn.Linear(5, 8, bias=False), nn.ReLU(), nn.Linear(8, 6)), "without a bias"),
                       (nn.Linear(5, 6), "must be a torch.nn.Sequential"), (5, "Sequential of Linear and ReLU or a list"),
                       ([torch.zeros(6, 5)], "Sequential of Linear and ReLU or a list"), ([], "1 .. 4 Linear layers"),
                       ([(torch.zeros(6, 5), torch.zeros(6))] * 5, "1 .. 4 Linear layers"),
                       ([(torch.zeros(6, 5), torch.zeros(5))], r"layer 0 must be \(weight \[out, in\], bias \[out\]\)"),
                       ([(torch.zeros(6, 5), 3.0)], "layer 0 must be")):
        with pytest.raises(ValueError, match=words):
            DeviceMLP(bad, 5, device="cuda:0")
    for na in (4, True, "5", 5.0):
        with pytest.raises(ValueError, match="num_actions must be None, 3, 5 or 8"):
            DeviceMLP(net, na, device="cuda:0")
    # tensors of no device at all
    meta = [(torch.empty(64, 51, device="meta"), torch.empty(64, device="meta")), (torch.empty(6, 64, device="meta"), torch.empty(6, device="meta"))]
    with pytest.raises(ValueError, match="cuda device"):
        DeviceMLP(meta, 5)
    with pytest.raises(ValueError, match="on cuda:0"):
        DeviceMLP(meta, 5, device="cuda:0")


# ---- the kernel's code on the host -------------------------------------------------------------------------------------------------------
HOST_SRC = os.path.join(helpers.TESTS, "native", "mlp_host.cpp")
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", _lib.CSRC, HOST_SRC]


def test_the_kernels_code_compiled_for_the_host_equals_the_rule_byte_for_byte(tmp_path):
    fn = load_shared(tmp_path, "mlp_host", ["-O2", "-fPIC", "-shared"] + HOST_FLAGS, timeout=600).mlp_host
    vp = C.c_void_p
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, vp, vp, vp, vp, C.c_int, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp]
    for dims, A in NETS:
        for rows in (1, 65) if dims in WIDE else (1, 65, 257):
            for head in (HEADS if A is not None and rows == 65 else ("plain",)):
                for shift in shifts_of(rows):
                    rng = np.random.default_rng(case_seed(dims, rows, shift, head))
                    c = make_mlp_case(rng, dims, rows, A, shift, head)
                    want = rule_of(c)
                    L = len(dims) - 1
                    dim = np.array(list(dims) + [0] * (5 - len(dims)), np.int32)
                    wp, bp = (vp * 4)(*[_vp(w) for w in c["weights"]]), (vp * 4)(*[_vp(x) for x in c["biases"]])
                    for f64 in (0, 1):
                        x = np.ascontiguousarray(c["x"] if f64 else c["x"].astype(np.float32))
                        y = np.full((rows, dims[-1]), 7, np.float32)
                        if A is None:
                            assert fn(L, _vp(dim), wp, bp, _vp(x), f64, rows, 0, _vp(y), *[None] * 6, 1, 64, 34, None, None) == 0
                            _same(y, want["y"], (dims, rows, shift, f64))
                            continue
                        lv = make_leaves(rng, rows, 9)
                        priors, value, est = np.full((rows, A), 7, np.float32), np.full(rows, 7, np.float64), lv["est"].copy()
                        bad = fn(L, _vp(dim), wp, bp, _vp(x), f64, rows, A, _vp(y), _vp(priors), _vp(value), *[None] * 4, 1, 64, 34, None, None)
                        assert bad == want["bad_rows"] == bad_rows_of(rows, shift, head), (dims, rows, shift, head, bad)
                        _same(y, want["y"], (dims, rows, shift, head, f64, "y"))
                        _same(priors, want["priors"], (dims, rows, shift, head, f64, "priors"))
                        assert value.tobytes() == want["value"].tobytes()
                        bad = fn(L, _vp(dim), wp, bp, _vp(x), f64, rows, A, None, _vp(priors), _vp(value), _vp(lv["first_has"]), _vp(lv["first_idx"]),
                                 _vp(lv["done"]), _vp(lv["stats"]), len(lv["stats"]), 64, lv["terminal_word"], _vp(lv["leaf"]), _vp(est))
                        wv, we = leaves_rule(want, **lv)
                        assert bad == want["bad_rows"] and value.tobytes() == wv.tobytes() and est.tobytes() == we.tobytes()
    assert fn(1, _vp(np.array([513, 4, 0, 0, 0], np.int32)), None, None, None, 0, 1, 0, *[None] * 7, 1, 64, 34, None, None) == -1


def test_the_kernels_code_runs_clean_under_the_host_sanitizers(tmp_path):
    """A stand-alone program (mlp_host.cpp with its main), not code loaded into python."""
    r = run_sanitized(tmp_path, "mlp_host_main", ["-DMLP_HOST_MAIN"] + HOST_FLAGS, probe_timeout=300, build_timeout=600, run_timeout=300)
    assert r.stdout.count("bad ") == 7 * 3 * 2 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
