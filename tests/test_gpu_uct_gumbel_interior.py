"""GPU: the Gumbel interior search (UCTSearch(gumbel=m, gumbel_interior=True); snac_uct_select_gumbel_interior / snac_uct_set_priors_value /
snac_uct_improved_policy, k_uct.hip) against a restatement in python floats of the rules of include/snac_hip.h ("Gumbel interior").

The rules, restated on top of the Gumbel root restatement (tests/test_gpu_uct_gumbel.py).  Every node keeps net_value, the evaluator's
value of its state (0 at a terminal node), written with its priors.  A root with candidates takes its turn action as before; every other
non-terminal node n has an improved policy
    vmix = sumN == 0 ? v : (v + sumN * (sp > 0 ? spq / sp : sW / sumN)) * I[sumN]        (sums over the visited children, prior-weighted)
    qh_a = visited ? W_a / N_a : vmix, normalised by the tree's bounds;   sig_a = ((c_visit + maxN) * c_scale) * qh_a
    pi_a = p_a * uct_exp(sig_a - smax) / Z
and the path takes the largest pi_a - (N_a + P_a) * I[sumN + sumP] (ties lowest a), then expands / falls back to the tried children /
descends as PUCT does after its U.  uct_exp is tests/test_uct_gumbel_interior_host.py's, the device's operation for operation, so every
comparison is bit for bit: every statistics word (net_value included), tree size, record, select output, est, the bytes of q_bounds,
cand, the moves, and the bytes of improved_policy(), which the same device function computes with every P = 0."""
import ctypes as C

import numpy as np
import pytest

from devmem import _env
from test_gpu_uct_gumbel import C_SCALE, C_VISIT, PI_ATOL, VL, GumbelRestatement, _cand, _noisy_scores, _phases
from test_gpu_uct_norm import _empty, scaled_evaluator
from test_gpu_uct_paths import _outputs
from test_gpu_uct_puct import C as CPUCT
from test_gpu_uct_puct import GAMMA
from test_gpu_uct_puct import _same_outputs as _same_outputs_puct
from test_gpu_uct_selfplay import _near_the_end, pick, restart
from test_uct_gumbel_interior_host import uct_exp

pytestmark = pytest.mark.gpu

INF = float("inf")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def improved(child, cn, cf, W, prior, v, lo, hi, c_visit, c_scale, inv_of):
    """The improved policy of one node from its words, python floats in the header's order: (pi [A], N [A], P [A], sumN, sumP).
    inv_of(i) is 1 / (1 + i): the table's entry (selection) or the quotient (snac_uct_improved_policy)."""
    A = len(child)
    has = [int(child[a]) >= 0 for a in range(A)]
    N = [max(int(cn[a]), 0) if has[a] else 0 for a in range(A)]
    P = [int(cf[a]) if has[a] else 0 for a in range(A)]
    vis = [has[a] and N[a] > 0 for a in range(A)]
    sum_n, sum_p, max_n = sum(N), sum(P), max(N)
    p = [float(prior[a]) for a in range(A)]
    q = [0.0] * A
    sp = spq = sw = 0.0
    for a in range(A):
        if vis[a]:
            q[a] = float(W[a]) / float(N[a])
            sp = sp + p[a]
            spq = spq + p[a] * q[a]
            sw = sw + float(W[a])
    v = float(v)
    if sum_n == 0:
        vmix = v
    else:
        mean = spq / sp if sp > 0.0 else sw / float(sum_n)
        vmix = (v + float(sum_n) * mean) * inv_of(sum_n)
    s2 = (c_visit + float(max_n)) * c_scale
    sig, smax = [], -INF
    for a in range(A):
        qh = q[a] if vis[a] else vmix
        if hi > lo:
            qh = (qh - lo) / (hi - lo)
        s = s2 * qh
        sig.append(s)
        if s > smax:                                                 # a NaN never wins
            smax = s
    e, z = [], 0.0
    for a in range(A):
        e.append(p[a] * uct_exp(sig[a] - smax))
        z = z + e[a]
    pi = [e[a] / z if z > 0.0 else 0.0 for a in range(A)]
    return pi, N, P, sum_n, sum_p


def _quotient(i):
    return 1.0 / (1.0 + float(i))


def _best(score, child):
    """(best, tried): the largest score by strict >, ties to the lowest a, over all actions / over the tried ones."""
    best, bu, tried, tu = -1, 0.0, -1, 0.0
    for a, u in enumerate(score):
        if best < 0 or u > bu:
            best, bu = a, u
        if int(child[a]) >= 0 and (tried < 0 or u > tu):
            tried, tu = a, u
    return best, tried


class InteriorRestatement(GumbelRestatement):
    """The Gumbel root search with the improved policy's rule everywhere else, and the nodes' network values."""

    def _netv(self):
        if not hasattr(self, "netv"):
            self.netv = np.zeros(self.B * (self.cap + self.K), np.float64)
            self._kept = None
        return self.netv

    def prime_roots(self):
        netv = self._netv()
        if self._kept is not None:                                   # advance(): a kept node keeps its value, every other row loses it
            old_netv, moves = self._kept
            for b, old in moves.items():
                base = int(self.roots[b])
                netv[base:base + self.cap] = 0.0
                netv[base + np.arange(len(old))] = old_netv[old]
            self._kept = None
        p, v = self._eval(self.roots)
        todo = self.visits[self.roots] == 0                          # only_unvisited
        self.prior[self.roots[todo]] = p[todo]
        netv[self.roots[todo]] = np.where(self.terminal[self.roots], 0.0, v)[todo]

    def _clear(self, lo, hi):
        super()._clear(lo, hi)
        self._netv()[lo:hi] = 0.0

    def _policy(self, n, b, P, inv_of):
        ch = [int(c) for c in self.child[n]]
        cn = [int(self.visits[c]) if c >= 0 else 0 for c in ch]      # the mirrors in n's line 0
        cw = [float(self.W[c]) if c >= 0 else 0.0 for c in ch]
        cf = [P.get(c, 0) if c >= 0 else 0 for c in ch]
        return improved(ch, cn, cf, cw, self.prior[n], self.netv[n], float(self.bounds[b, 0]), float(self.bounds[b, 1]), self.c_visit,
                        self.c_scale, inv_of)

    def _select_tree(self, b):
        base, cap, K = b * self.cap, self.cap, self.K
        fresh = base + int(self.used[b])
        cs = [a for a in range(self.A) if int(self.cand[b]) >> a & 1]
        P, expander, out = {}, {}, []
        for k in range(K):
            s = b * K + k
            scratch = self.B * cap + s
            n, path, res = base, [], None
            leaf, r = base, np.float32(0)
            for depth in range(cap):
                path.append(n)
                if n >= fresh:
                    res = (base, scratch, 0, n, False, np.float32(0), expander[n])
                    break
                leaf, r = n, self.reward[n]
                if self.terminal[n]:
                    break
                if depth == 0 and cs:                                # the candidate whose turn it is
                    best, tried = cs[(self.offset + k) % len(cs)], -1
                else:                                                # no U anywhere else
                    pi, N, Pa, sum_n, sum_p = self._policy(n, b, P, lambda i: self._tab(self.itab, i))
                    inv = self._tab(self.itab, sum_n + sum_p)
                    best, tried = _best([pi[a] - float(N[a] + Pa[a]) * inv for a in range(self.A)], self.child[n])
                    self.interior_levels += 1
                if self.child[n, best] < 0:
                    if self.used[b] < cap:
                        new = base + int(self.used[b])
                        self.used[b] += 1
                        self.child[n, best] = new
                        expander[new] = s
                        path.append(new)
                        res = (n, new, best, new, True, np.float32(0), s)
                        break
                    if tried < 0:
                        self.root_stops += depth == 0 and bool(cs)
                        break
                    self.fallbacks += 1                              # the budget spent: the best of the tried children by score
                    best = tried
                n = int(self.child[n, best])
            if res is None:
                res = (leaf, scratch, 0, leaf, False, r, -1)
            for x in path:
                P[x] = P.get(x, 0) + 1
            out.append(res)
        return out

    interior_levels = fallbacks = 0

    def iteration(self):
        """NormPuctRestatement.iteration, keeping the leaves' values: an expanded row is written whole (net_value 0), and after the
        walks gets its priors and its value (0 where the leaf is terminal)."""
        import torch

        sel = [r for b in range(self.B) for r in self._select_tree(b)]
        src, dst, act, leaf, exp, rleaf, first = (np.array(x) for x in zip(*sel))
        self.last = dict(src=src, dst=dst, action=act, leaf=leaf, expanded=exp, r_leaf=rleaf.astype(np.float32), first_slot=first)
        self.fresh_hits.append((~exp) & (first >= 0))
        t = self.it * (self.H + 1)
        with self.slot_keys():
            _, rew, done = self.pool.transition(torch.as_tensor(act.astype(np.int8)), src=src, dst=dst, t=t, want_obs=False)
        rew, done = rew.cpu().numpy(), done.cpu().numpy()
        first_r = np.where(first >= 0, rew[np.maximum(first, 0)], rleaf.astype(np.float32)).astype(np.float64)
        leaf_term = np.where(first >= 0, done[np.maximum(first, 0)], self.terminal[leaf])
        priors, value = self._eval(leaf)
        kept = np.where(leaf_term, 0.0, value)
        est = first_r + kept
        self.last_est, self.last_term = est, leaf_term
        for s in np.nonzero(exp)[0]:
            x = int(leaf[s])
            self.parent[x], self.action[x], self.reward[x], self.terminal[x] = src[s], act[s], rew[s], done[s]
            self.prior[x] = 0
            self.netv[x] = 0.0
        self._walks(leaf, est)
        for s in np.nonzero(exp)[0]:
            self.prior[int(leaf[s])] = priors[s]
            self.netv[int(leaf[s])] = kept[s]
        self.it += 1

    def advance(self, actions):
        moves = {}
        for b in range(self.B):                                      # the rows each tree keeps, as PuctRestatement.advance finds them
            base = int(self.roots[b])
            if self.terminal[base]:
                continue
            c = int(self.child[base, actions[b]])
            old = []
            if c >= 0:
                old = [c]
                for i in range(c + 1, base + int(self.used[b])):
                    x = i
                    while x > c:
                        x = int(self.parent[x])
                    if x == c:
                        old.append(i)
            moves[b] = np.array(old, np.int64)
        self._kept = (self._netv().copy(), moves)                    # applied before the new roots are primed
        return super().advance(actions)

    def improved_policy(self):
        """[B, A] float32: snac_uct_improved_policy on the roots (every P = 0, the quotient for the table; a terminal root: zeros)."""
        out = np.zeros((self.B, self.A), np.float32)
        for b in range(self.B):
            root = int(self.roots[b])
            if not self.terminal[root]:
                out[b] = np.array(self._policy(root, b, {}, _quotient)[0], np.float64).astype(np.float32)
        return out


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _search(env, B, cap, K, m, budget, fn=None, interior=True, **kw):
    from snac_amd import UCTSearch

    fn = scaled_evaluator(env.num_actions) if fn is None else fn
    s = UCTSearch(env, cap, 0, GAMMA, c=CPUCT, max_iterations=budget, trees=B, paths=K, virtual_loss=VL, evaluator=fn, q_normalise=True,
                  gumbel=m, gumbel_interior=interior, **kw)
    s.reset()
    return s


def _pair(env, B, cap, K, m, budget, renv=None):
    fn = scaled_evaluator(env.num_actions)
    search = _search(env, B, cap, K, m, budget, fn)
    ref = InteriorRestatement(env if renv is None else renv, B, cap, K, VL, 0, GAMMA, CPUCT, fn, 0.0, budget, m=m)
    return search, ref


def _same(search, ref, live_only=False, outputs=True):
    """Every statistics word (net_value in words 56-57), tree size and record, the select outputs, est and the bounds' bytes;
    live_only: rows [base, base + used) only (after advance() the rest is unspecified)."""
    import torch

    torch.cuda.synchronize()
    A, B, cap = ref.A, ref.B, ref.cap
    used = search.tree_sizes().cpu().numpy()
    assert np.array_equal(used, ref.used)
    rows = np.concatenate([b * cap + np.arange(int(used[b])) for b in range(B)]) if live_only else np.arange(B * (cap + ref.K))
    stats = search.stats.cpu().numpy()[rows]
    assert np.array_equal(stats[:, :A], ref.child[rows]) and (stats[:, A:8] == -1).all()
    assert np.array_equal(stats[:, 32], ref.parent[rows]) and np.array_equal(stats[:, 33], ref.action[rows])
    assert np.array_equal(stats[:, 34] != 0, ref.terminal[rows]) and np.array_equal(stats[:, 35], ref.visits[rows])
    assert np.ascontiguousarray(stats[:, 36:38]).tobytes() == ref.W[rows].tobytes()
    assert np.ascontiguousarray(stats[:, 38]).view(np.float32).tobytes() == ref.reward[rows].tobytes()
    assert np.ascontiguousarray(stats[:, 48:48 + A]).tobytes() == ref.prior[rows].tobytes()
    assert np.ascontiguousarray(stats[:, 56:58]).tobytes() == ref.netv[rows].tobytes()              # net_value, raw float64 bytes
    assert search.net_values.cpu().numpy()[rows].tobytes() == ref.netv[rows].tobytes()
    assert not stats[:, 39:48].any() and not stats[:, 48 + A:56].any() and not stats[:, 58:].any()
    ch, has = ref.child[rows], ref.child[rows] >= 0
    mirror_w = np.ascontiguousarray(stats[:, 16:32]).view(np.float64)[:, :A]
    assert np.array_equal(stats[:, 8:8 + A][has], ref.visits[ch[has]]) and not stats[:, 8:8 + A][~has].any()
    assert mirror_w[has].tobytes() == ref.W[ch[has]].tobytes()
    ri = torch.as_tensor(rows, device=search.env.device)
    assert torch.equal(search.pool.records[ri], ref.pool.records[ri])
    if outputs and ref.last is not None:
        _same_outputs_puct(search, ref)
    assert search.q_bounds.cpu().numpy().tobytes() == ref.bounds.tobytes(), (search.q_bounds.cpu().numpy(), ref.bounds)


def _same_policy(search, ref):
    import torch

    got = search.improved_policy()
    assert got.dtype == torch.float32 and tuple(got.shape) == (ref.B, ref.A)
    got, want = got.cpu().numpy(), ref.improved_policy()
    assert got.tobytes() == want.tobytes(), np.abs(got - want).max()
    live = ~ref.terminal[ref.roots]
    assert not got[~live].any()
    assert np.abs(got[live].astype(np.float64).sum(1) - 1.0).max(initial=0.0) <= PI_ATOL
    return got


def _lockstep(search, ref, n):
    """gumbel_run(n) with the restatement following launch by launch (tests/test_gpu_uct_gumbel.py: _lockstep, with this file's _same)."""
    plan = _phases(n, min(ref.m, ref.A))
    state = dict(pos=0, halved=False, halvings=0)
    candidates, set_priors = search._candidates, search._set_priors

    def on_candidates(mode, action=None):
        candidates(mode, action)
        assert mode == 1 and plan[state["pos"]][0] and not state["halved"]
        ref.halve()
        state["halved"] = True
        state["halvings"] += 1
        assert np.array_equal(_cand(search), ref.cand), state

    def on_set_priors():
        set_priors()
        halve, i = plan[state["pos"]]
        assert halve == state["halved"], state
        ref.offset = i * ref.K
        ref.iteration()
        state["pos"] += 1
        state["halved"] = False
        _same(search, ref, live_only=ref.advanced)
        assert np.array_equal(_cand(search), ref.cand)

    search._candidates, search._set_priors = on_candidates, on_set_priors
    try:
        search.gumbel_run(n)
    finally:
        del search._candidates, search._set_priors
    assert state["pos"] == n
    return state["halvings"]


# ---- a. the restatement, launch by launch -------------------------------------------------------------------------------------------------
CASES = [(kind, dyn, m) for kind, dyn, A in ((1, False, 3), (2, True, 5), (3, True, 8)) for m in sorted({2, A})]


@pytest.mark.parametrize("cap", [24, 64])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("B", [5, 70])
@pytest.mark.parametrize("kind,dyn,m", CASES)
def test_gumbel_interior_search_equals_the_restatement_bit_for_bit(kind, dyn, m, B, K, cap):
    """Two moves of gumbel_begin -> gumbel_run(9) -> gumbel_actions -> advance, so net_value is carried across two re-rootings, and
    three run(1) launches without candidates after the first advance(), where the root too follows the interior rule; rows 0::3 are one step before the time limit, so root children of theirs are terminal and, in 1D and 2D, their
    second roots are terminal.  cap = 24 with K = 3: the simulations spend the node budget."""
    import torch

    n, extra = 9, 3
    env = _env(kind, dyn, B, 5 + kind + dyn)
    _near_the_end(kind, dyn)(env)
    A = env.num_actions
    search, ref = _pair(env, B, cap, K, m, 2 * n + extra)
    ref.advanced = False
    _same(search, ref)                                               # the primed roots: priors and values, empty bounds
    assert _empty(ref.bounds).all() and ref.netv[ref.roots].any()
    prior = ref.prior[ref.roots].astype(np.float64)
    p0 = _same_policy(search, ref)                                   # nothing visited: vmix = v for every action, pi' = the normalised priors
    assert np.abs(p0 - prior / prior.sum(1, keepdims=True)).max() <= PI_ATOL
    for move in range(2):
        assert not _cand(search).any()
        scores = _noisy_scores(search, 100 + move)
        search.gumbel_begin(scores)
        ref.begin(scores.cpu().numpy())
        assert np.array_equal(_cand(search), ref.cand)
        _lockstep(search, ref, n)
        got = search.gumbel_actions()
        assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), ref.pick_moves())
        assert np.array_equal(_cand(search), ref.cand)
        _same_policy(search, ref)
        live = ~ref.terminal[ref.roots]
        if move == 0:
            assert live.all()
        else:                                                        # before the second re-rooting shrinks the trees again
            assert ref.netv[: B * cap].any() and not ref.netv[B * cap:].any()
            spent = int((ref.used == cap).sum())
        r, d = search.advance(got)
        er, ed = ref.advance(got.cpu().numpy())
        ref.advanced = True
        assert r.cpu().numpy().tobytes() == er.tobytes() and np.array_equal(d.cpu().numpy(), ed)
        assert not _cand(search).any()
        _same(search, ref, live_only=True, outputs=False)            # a kept node keeps its net_value, a new root is primed with one
        _same_policy(search, ref)
        if move == 0:
            if kind != 3:
                assert ed[0::3].all() and not ed.all()
            ref.offset = 0
            for _ in range(extra):                                   # cand == 0: the interior rule at the root as well
                search.run(1)
                ref.iteration()
                _same(search, ref, live_only=True)
            _same_policy(search, ref)
        else:
            assert ed[~live].all()                                   # a terminal root stays, with the value it had (0)
    assert search.iterations == 2 * n + extra and ref.interior_levels > 0
    if cap == 24 and K == 3:
        print("trees with the budget spent: %d of %d; fallbacks to the tried children: %d" % (spent, B, ref.fallbacks))
        assert spent > 0 and ref.fallbacks > 0


# ---- b. written statistics ----------------------------------------------------------------------------------------------------------------
NAN = float("nan")
P0 = [0.1, 0.2, 0.3, 0.25, 0.15]
# per tree: (children present, child_visits, child_value, priors, net_value, bounds)
WRITTEN = [
    ([0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0.0] * 5, P0, 0.7, (INF, -INF)),                             # 0: nothing visited: vmix = v
    ([1, 1, 0, 0, 0], [3, 2, 0, 0, 0], [6.0, -2.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.5, 0.3, 0.2], 0.5, (-1.0, 2.0)),   # 1: sp == 0: the visit-weighted mean
    ([1, 1, 1, 0, 0], [4, 2, 2, 0, 0], [1.0, 2.0, 3.0, 0.0, 0.0], [0.0] * 5, 0.2, (0.0, 2.0)),       # 2: every prior zero: Z == 0, pi = 0
    ([1, 1, 0, 0, 0], [2, 2, 0, 0, 0], [8.0, 6.0, 0.0, 0.0, 0.0], P0, 1.0, (3.5, 3.5)),              # 3: hi == lo: q as it is
    ([1, 1, 1, 0, 0], [0, 7, 2, 0, 0], [5.0, 70.0, -6.0, 0.0, 0.0], P0, -0.3, (-3.0, 10.0)),         # 4: a child row with 0 visits: not visited
    ([1, 1, 0, 0, 0], [3, 1, 0, 0, 1000], [3.0, 2.0, 0.0, 0.0, 555.0], P0, 0.4, (0.0, 4.0)),         # 5: a count without a child: not counted
    ([1, 1, 0, 0, 0], [5, 5, 0, 0, 0], [5000.0, 0.0, 0.0, 0.0, 0.0], P0, 0.0, (INF, -INF)),          # 6: sig spread below -700: uct_exp gives 0
    ([1, 1, 1, 0, 0], [2, 3, 1, 0, 0], [NAN, 3.0, 1.0, 0.0, 0.0], P0, 0.1, (-1.0, 3.0)),             # 7: a NaN W: NaN q, NaN vmix
    ([1, 1, 1, 1, 1], [3, 1, 4, 1, 5], [30.0, -20.0, 10.0, 90.0, -50.0], P0, 12.5, (-20.0, 90.0)),   # 8: a terminal root (set below)
    ([1, 1, 1, 1, 1], [3, 1, 4, 1, 5], [30.0, -20.0, 10.0, 90.0, -50.0], P0, 12.5, (-20.0, 90.0)),   # 9: everything visited, bounds on
    ([1, 0, 1, 0, 1], [6, 0, 1, 0, 2], [-3.0, 0.0, 4.0, 0.0, 1.0], [0.3, 0.3, 0.2, 0.1, 0.1], -2.0, (-4.0, 4.0)),  # 10: visited and unvisited actions mixed
]
TERMINAL_TREE = 8


def _write(search):
    """Writes WRITTEN into the roots of `search` (B = len(WRITTEN) trees of A = 5 actions, cap 16): root b's child a is row base + 1 + a,
    a terminal node, so that a path that descends stops there; used = 1 + A."""
    import torch

    B, A, cap = len(WRITTEN), 5, search.nodes_per_tree
    assert search.trees == B and search.num_actions == A and search.paths == 1
    stats = search.stats.cpu().numpy()
    bounds = np.zeros((B, 2))
    for b, (has, visits, W, prior, netv, bd) in enumerate(WRITTEN):
        base = b * cap
        root = stats[base]
        root[:] = 0
        root[0:8], root[32:34] = -1, -1
        root[34] = b == TERMINAL_TREE
        root[8:8 + A] = visits
        root[16:16 + 2 * A] = np.array(W, np.float64).view(np.int32)
        root[35] = 1 + sum(v for v, h in zip(visits, has) if h)
        root[48:48 + A] = np.array(prior, np.float32).view(np.int32)
        root[56:58] = np.array([netv], np.float64).view(np.int32)
        for a in range(A):
            if has[a]:
                row = stats[base + 1 + a]
                row[:] = 0
                root[a] = base + 1 + a
                row[0:8], row[32], row[33], row[34], row[35] = -1, base, a, 1, visits[a]
                row[36:38] = np.array([W[a]], np.float64).view(np.int32)
        bounds[b] = bd
    search.stats.copy_(torch.as_tensor(stats))
    search.q_bounds.copy_(torch.as_tensor(bounds))
    search._used.fill_(1 + A)
    search.cand.zero_()
    torch.cuda.synchronize()


def _written_policy(b, inv_of):
    has, visits, W, prior, netv, bd = WRITTEN[b]
    child = [1 if h else -1 for h in has]
    prior = [float(x) for x in np.array(prior, np.float32)]
    return improved(child, visits, [0] * 5, W, prior, netv, bd[0], bd[1], C_VISIT, C_SCALE, inv_of) + (child,)


def test_selection_and_improved_policy_on_written_statistics():
    import torch

    B, A, cap = len(WRITTEN), 5, 16
    env = _env(2, True, B, 3)
    search = _search(env, B, cap, 1, 4, 64)                          # inv_table covers every sumN written below
    _write(search)
    before = search.stats.cpu().numpy().copy()
    # the policy: the roots through improved_policy(), then rows outside the trees, a terminal child row and a root again through the C ABI
    got = search.improved_policy().cpu().numpy()
    want = np.zeros((B, A), np.float32)
    for b in range(B):
        if b != TERMINAL_TREE:
            want[b] = np.array(_written_policy(b, _quotient)[0], np.float64).astype(np.float32)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert not got[TERMINAL_TREE].any() and not got[2].any()         # a terminal root; Z == 0
    assert got[6, 0] == 1.0 and not got[6, 1:].any()                 # exp(-55000) is 0
    assert got[7, 0] == 0.0 and not got[7, 3:].any() and got[7, 1] > 0 and got[7, 2] > 0 and abs(float(got[7].sum()) - 1.0) <= PI_ATOL
    p0 = np.array(P0, np.float32).astype(np.float64)
    assert np.abs(got[0] - p0 / p0.sum()).max() <= PI_ATOL           # vmix = v for every action: the normalised priors
    assert got[5, 4] < got[5, 3]                                     # the count of 1000 without a child pulled nothing towards action 4
    rows = torch.tensor([9 * cap, -1, B * cap, B * cap + 3, 0x7FFFFFFF, -0x80000000, 9 * cap + 1, 3 * cap], dtype=torch.int32, device=env.device)
    pi = torch.full((len(rows), A), 7.0, dtype=torch.float32, device=env.device)
    from snac_amd import _lib

    L = _lib.lib()
    _lib.check(L.snac_uct_improved_policy(A, C.c_void_p(search.stats.data_ptr()), search.rows, B, cap, len(rows), C.c_void_p(rows.data_ptr()),
                                          C_VISIT, C_SCALE, C.c_void_p(search.q_bounds.data_ptr()), C.c_void_p(pi.data_ptr()), env._stream()))
    torch.cuda.synchronize()
    pi = pi.cpu().numpy()
    assert pi[0].tobytes() == want[9].tobytes() and pi[7].tobytes() == want[3].tobytes()
    assert not pi[1:7].any()                                         # outside [0, B * cap) (a scratch row included); then a terminal child
    assert np.array_equal(search.stats.cpu().numpy(), before)        # read only
    # selection: one path per tree, no candidates: the interior rule at the root
    search._select()
    torch.cuda.synchronize()
    o = _outputs(search)
    picked = []
    for b in range(B):
        base = b * cap
        if b == TERMINAL_TREE:
            assert o["leaf"][b] == base and not o["expanded"][b] and o["first_slot"][b] == -1
            picked.append(None)
            continue
        pi_b, N, P, sum_n, sum_p, child = _written_policy(b, _quotient)          # the table's entries are these quotients
        best, _ = _best([pi_b[a] - float(N[a] + P[a]) * _quotient(sum_n + sum_p) for a in range(A)], child)
        picked.append(best)
        if child[best] < 0:                                          # expanded into the tree's next row
            assert o["expanded"][b] and o["action"][b] == best and o["leaf"][b] == base + 1 + A and o["src"][b] == base, (b, best, o)
        else:                                                        # descended to the (terminal) child
            assert not o["expanded"][b] and o["leaf"][b] == base + 1 + best, (b, best, o)
    # written out: 0: the largest prior.  2: pi = 0, the lowest count wins: the first untried action.  6: pi = (1, 0, ..): 1 - 5 / 11 beats
    # 0 - 0.  10: the best visited child's sigma dominates pi': a visited action is taken although two are untried
    assert picked[0] == 2 and picked[2] == 3 and picked[6] == 0 and WRITTEN[10][0][picked[10]] == 1
    assert len({p for p in picked if p is not None}) > 2


# ---- c. the switch ------------------------------------------------------------------------------------------------------------------------
def test_the_interior_rule_and_normalised_puct_pick_different_actions():
    """One root: child 0 tried twice with q = 0 and prior 0.9, four untried actions of prior 0.025, network value 1.  PUCT (c = 1.25,
    first_play_value 0): U_0 = 1.25 * 0.9 * sqrt(3) / 3 = 0.65 against 1.25 * 0.025 * sqrt(3) = 0.054: it descends to child 0.  The
    interior rule: vmix = (1 + 2 * 0) / 3, so every untried action's completed q is above child 0's, sigma = 52 * q separates them by
    e^-17, pi' is 0.25 on each untried action and about 0 on action 0, whose score is then -2 / 3: it expands action 1."""
    import torch

    B, A, cap = 1, 5, 8
    env = _env(2, True, B, 3)
    out = {}
    for interior in (False, True):
        search = _search(env, B, cap, 1, 4, 4, interior=interior)
        stats = search.stats.cpu().numpy()
        root, row = stats[0], stats[1]
        root[:], row[:] = 0, 0
        root[0:8], root[32:34], root[0] = -1, -1, 1
        root[8], root[35] = 2, 3
        root[48:48 + A] = np.array([0.9, 0.025, 0.025, 0.025, 0.025], np.float32).view(np.int32)
        root[56:58] = np.array([1.0], np.float64).view(np.int32)
        row[0:8], row[32], row[33], row[34], row[35] = -1, 0, 0, 1, 2
        search.stats.copy_(torch.as_tensor(stats))
        search._used.fill_(2)
        search._select()
        torch.cuda.synchronize()
        out[interior] = _outputs(search)
    assert not out[False]["expanded"][0] and out[False]["leaf"][0] == 1                   # PUCT: down to child 0
    assert out[True]["expanded"][0] and out[True]["action"][0] == 1 and out[True]["leaf"][0] == 2      # interior: action 1 expanded


def test_with_the_switch_off_the_search_is_the_gumbel_root_search():
    import torch

    from snac_amd import UCTSearch

    B, cap, K, m, n = 7, 24, 3, 4, 6
    env = _env(2, True, B, 29)
    fn = scaled_evaluator(env.num_actions)
    off = _search(env, B, cap, K, m, n, fn, interior=False)
    plain = UCTSearch(env, cap, 0, GAMMA, c=CPUCT, max_iterations=n, trees=B, paths=K, virtual_loss=VL, evaluator=fn, q_normalise=True, gumbel=m)
    plain.reset()
    assert off.gumbel_interior is False and plain.gumbel_interior is False
    for s in (off, plain):
        s.gumbel_begin(_noisy_scores(s, 5))
        s.gumbel_run(n)
    torch.cuda.synchronize()
    assert torch.equal(off.stats, plain.stats) and torch.equal(off.tree_sizes(), plain.tree_sizes()) and torch.equal(off.cand, plain.cand)
    assert torch.equal(off.pool.records, plain.pool.records)
    oa, ob = _outputs(off), _outputs(plain)
    for k in oa:
        assert oa[k].tobytes() == ob[k].tobytes(), k
    assert off._est.cpu().numpy().tobytes() == plain._est.cpu().numpy().tobytes()
    assert off.q_bounds.cpu().numpy().tobytes() == plain.q_bounds.cpu().numpy().tobytes()
    assert torch.equal(off.gumbel_actions(), plain.gumbel_actions())
    assert off.improved_policy().cpu().numpy().tobytes() == plain.improved_policy().cpu().numpy().tobytes()
    assert not off.net_values.any()                                  # the words stay zero


def test_improved_policy_agrees_with_the_root_search_formula_where_every_action_is_visited():
    """With no unvisited root action v_mix enters nothing, and the two policies differ in their exp / log implementations only."""
    import torch

    B, cap, K, m, n = 6, 64, 1, 3, 9
    env = _env(1, False, B, 43)
    fn = scaled_evaluator(env.num_actions)
    search = _search(env, B, cap, K, m, n, fn)
    search.gumbel_begin(_noisy_scores(search, 11))
    search.gumbel_run(n)
    assert (search.root_visits() > 0).all()                          # m = A = 3: the first phase visits every action
    plain = _search(env, B, cap, K, m, n, fn, interior=False)
    plain.stats.copy_(search.stats)
    plain.q_bounds.copy_(search.q_bounds)
    got, want = search.improved_policy().cpu().numpy(), plain.improved_policy().cpu().numpy()
    print("max |kernel - torch float64 formula| = %.3g" % np.abs(got - want).max())
    assert np.abs(got - want).max() <= PI_ATOL
    assert np.abs(got.astype(np.float64).sum(1) - 1.0).max() <= PI_ATOL
    prior = search.root_priors().cpu().numpy().astype(np.float64)
    assert np.abs(got - prior / prior.sum(1, keepdims=True)).max() > 1.0e-3      # the search moved the policy


# ---- d. snac_uct_set_priors_value ---------------------------------------------------------------------------------------------------------
def test_set_priors_value_writes_ten_words_of_the_rows_it_may():
    import torch

    from snac_amd import _lib

    B, cap, A = 3, 8, 5
    env = _env(2, True, B, 3)
    search = _search(env, B, cap, 1, 4, 4)
    L = _lib.lib()
    g = torch.Generator(device="cpu")
    g.manual_seed(1)
    pattern = torch.randint(-2 ** 31, 2 ** 31 - 1, tuple(search.stats.shape), generator=g, dtype=torch.int64).to(torch.int32)
    pattern[:, 35] = 0
    pattern[5, 35], pattern[9, 35] = 4, -1                           # visited rows
    rows = torch.tensor([2, -1, search.rows, 5, search.rows - 1, 0x7FFFFFFF, 9, 2 * cap + 1], dtype=torch.int32, device=env.device)
    m = len(rows)
    priors = (torch.arange(m * A, dtype=torch.float32, device=env.device).view(m, A) + 0.5) / 64.0
    value = torch.arange(m, dtype=torch.float64, device=env.device) * 1.25 - 3.0
    value[7] = float("-inf")

    def call(only_unvisited):
        search.stats.copy_(pattern)
        _lib.check(L.snac_uct_set_priors_value(A, C.c_void_p(search.stats.data_ptr()), search.rows, m, C.c_void_p(rows.data_ptr()),
                                               C.c_void_p(priors.data_ptr()), C.c_void_p(value.data_ptr()), only_unvisited, env._stream()))
        torch.cuda.synchronize()
        return search.stats.cpu().numpy()

    for only_unvisited, written in ((1, [0, 4, 7]), (0, [0, 3, 4, 6, 7])):           # entries of `rows`; the others are outside or visited
        got, want = call(only_unvisited), pattern.numpy().copy()
        for i in written:
            r = int(rows[i])
            want[r, 48:48 + A] = priors[i].cpu().numpy().view(np.int32)
            want[r, 48 + A:56] = 0
            want[r, 56:58] = value[i:i + 1].cpu().numpy().view(np.int32)
        assert np.array_equal(got, want), only_unvisited             # no other word of any row
    assert search.net_values.cpu().numpy()[[2, search.rows - 1, 2 * cap + 1]].tolist() == [-3.0, 2.0, float("-inf")]


def test_advance_carries_the_net_value_and_restart_zeroes_it_before_priming():
    import torch

    B, cap, K, m, n = 6, 32, 2, 4, 6
    env = _env(2, True, B, 17)
    search = _search(env, B, cap, K, m, 2 * n)
    search.gumbel_begin(_noisy_scores(search, 3))
    search.gumbel_run(n)
    a = search.gumbel_actions().long()
    roots = search._roots
    child = search.stats[roots, :][torch.arange(B, device=env.device), a].long()
    assert (child > 0).all()
    old, kept_priors = search.net_values[child].clone(), search.prior[child].clone()
    assert old.ne(0).any()
    search.advance(a)
    assert search.net_values[roots].cpu().numpy().tobytes() == old.cpu().numpy().tobytes()       # moved with the node, bit for bit
    assert torch.equal(search.prior[roots], kept_priors)
    mask = torch.tensor([1, 0, 1, 0, 0, 1], dtype=torch.uint8, device=env.device)
    keep = search.net_values[roots].clone()
    prime = search._prime_roots
    search._prime_roots = lambda: None
    try:
        search.restart(mask)
        torch.cuda.synchronize()
        seen = search.net_values[roots].clone()
    finally:
        del search._prime_roots
    assert not seen[mask.bool()].any() and torch.equal(seen[~mask.bool()], keep[~mask.bool()])   # zeroed where restarted, kept elsewhere
    assert not search.prior[roots][mask.bool()].any()
    prime()
    torch.cuda.synchronize()
    obs = search.pool.observe(roots.to(torch.int32))
    _, v = scaled_evaluator(env.num_actions)(obs)
    now = search.net_values[roots]
    assert torch.equal(now[mask.bool()], v.to(torch.float64)[mask.bool()]) and now[mask.bool()].ne(0).any()      # the priming call's value
    assert torch.equal(now[~mask.bool()], keep[~mask.bool()])        # a visited root keeps its own


# ---- e. self-play -------------------------------------------------------------------------------------------------------------------------
def test_gumbel_interior_self_play_equals_the_restatement_move_by_move():
    import torch

    from snac_amd import SelfPlay, _lib

    B, cap, K, m, its, moves = 5, 48, 3, 4, 8, 6
    ts = _lib.env_sizes(2, True).total_step
    env, renv = _env(2, True, B, 39), _env(2, True, B, 39)           # play() resets env rows: the restatement follows on a twin
    for e in (env, renv):
        _near_the_end(2, True)(e)
    search = _search(env, B, cap, K, m, (ts + 1) * its)
    captured, begin = [], search.gumbel_begin

    def on_begin(scores):
        captured.append(scores.clone())
        begin(scores)

    search.gumbel_begin = on_begin
    play = SelfPlay(search, moves, sample_moves=0, gumbel=True)
    play.play(2, its)
    play.play(moves - 2, its)
    torch.cuda.synchronize()
    assert len(captured) == moves
    fn = scaled_evaluator(env.num_actions)
    ref = InteriorRestatement(renv, B, cap, K, VL, 0, GAMMA, CPUCT, fn, 0.0, (ts + 1) * its, m=m)
    A = env.num_actions
    want_action, want_pi = np.zeros((moves, B), np.int8), np.zeros((moves, B, A), np.float32)
    want_done, want_value = np.zeros((moves, B), np.uint8), np.zeros((moves, B), np.float32)
    restarts = np.zeros(B, np.int64)
    for mv in range(moves):
        ref.begin(captured[mv].cpu().numpy())
        ref.run(its)
        a = ref.pick_moves()
        want_pi[mv] = ref.improved_policy()
        want_value[mv] = pick(ref, True, mv)[2]
        r, d = ref.advance(a)
        want_action[mv], want_done[mv] = a, d
        renv.reset(mask=torch.as_tensor(d, device=env.device), want_obs=False)
        restart(ref, d)
        ref.rebound(d)
        restarts += d
    assert (restarts > 0).any() and (restarts == 0).any()            # the inputs: trees that restarted and trees that did not
    assert play.action.cpu().numpy().tobytes() == want_action.tobytes()
    assert play.pi.cpu().numpy().tobytes() == want_pi.tobytes()      # the kernel's policy: bit for bit
    assert play.done.cpu().numpy().tobytes() == want_done.tobytes() and play.value.cpu().numpy().tobytes() == want_value.tobytes()
    live = play.pi.cpu().numpy().astype(np.float64).sum(2)
    assert np.abs(live - 1.0).max() <= PI_ATOL                       # every recorded move was made at a live root
    _same(search, ref, live_only=True, outputs=False)
    assert not _cand(search).any() and torch.equal(env._hdr, renv._hdr)


def test_a_gumbel_interior_move_does_not_synchronise_with_the_host():
    import torch

    B, its = 64, 3
    env = _env(2, True, B, 3)
    _near_the_end(2, True)(env)
    search = _search(env, B, 64, 4, 4, 4 * its)
    search.gumbel_begin(search.gumbel_scores())                      # warm-up: every kernel and torch op once
    search.gumbel_run(its)
    search.advance(search.gumbel_actions(), check=False)
    search.improved_policy()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            search.gumbel_begin(search.gumbel_scores())
            search.gumbel_run(its)
            a, pi = search.gumbel_actions(), search.improved_policy()
            r, d = search.advance(a, check=False)
            search.restart(d)
        search.run(1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert search.iterations == 3 * its + 1 and d.any() and not d.all()
    assert np.abs(pi.cpu().numpy().astype(np.float64).sum(1) - 1.0).max() <= PI_ATOL


# ---- f. sharding --------------------------------------------------------------------------------------------------------------------------
def test_a_sharded_gumbel_interior_search_is_the_whole_search():
    """In the manner of tests/test_gpu_uct_sharding.py: trees [off, off + n) of the whole batch and the shard with env_id_base + off."""
    import torch

    from snac_amd import UCTSearch

    import test_gpu_uct_sharding as sh

    K, m, n = 4, 4, 8
    whole_env, shards = sh._envs(2, True)
    sh._near_the_end(whole_env, 0)
    for off, e in shards:
        sh._near_the_end(e, off)
    A = whole_env.num_actions
    rng = np.random.default_rng(17)
    scores = [rng.gumbel(size=(sh.N, A)).astype(np.float32) for _ in range(2)]       # per global tree and move

    def make(env, off):
        s = UCTSearch(env, nodes_per_tree=sh.CAP, horizon=0, gamma=sh.GAMMA, c=CPUCT, max_iterations=2 * n, paths=K, virtual_loss=sh.VL,
                      evaluator=scaled_evaluator(A), q_normalise=True, gumbel=m, gumbel_interior=True)
        s.reset()
        out = []
        for mv in range(2):
            x = torch.as_tensor(scores[mv][off:off + s.trees], device=env.device)
            s.gumbel_begin(s.gumbel_scores(noise=False) + x)
            s.gumbel_run(n)
            a, pi = s.gumbel_actions(), s.improved_policy()
            out.append((s.cand.clone(), a, pi, s.q_bounds_of_trees()))
            if mv == 0:
                s.advance(a)
        torch.cuda.synchronize()
        return s, out

    def values(s, first, cnt):                                       # the live rows' net values, tree by tree
        used = s.tree_sizes().cpu().numpy()
        nv = s.net_values.cpu().numpy()
        return [nv[(first + b) * sh.CAP:(first + b) * sh.CAP + int(used[first + b])].tobytes() for b in range(cnt)]

    whole, wout = make(whole_env, 0)
    assert len(set(wout[0][1].cpu().numpy().tolist())) > 1
    for off, e in shards:
        s, out = make(e, off)
        cnt = s.trees
        for mv in range(2):
            for got, want in zip(out[mv], wout[mv]):
                assert got.cpu().numpy().tobytes() == want[off:off + cnt].cpu().numpy().tobytes(), (off, mv)
        sh._same_trees(s, whole, off, live_only=True)
        assert values(s, 0, cnt) == values(whole, off, cnt)
