"""GPU: the PUCT search (UCTSearch(evaluator=fn); snac_uct_select_puct / snac_uct_set_priors / snac_observe_nodes*, k_uct.hip and
k_nodes_obs.hip) against a restatement in python of the rules of include/snac_hip.h ("PUCT").

The rules, restated.  Slots, scratch rows, fresh rows, first_slot and the in-flight counts P are those of the multi-path search
(tests/test_gpu_uct_paths.py: Restatement, which this file extends).  At a stored, non-terminal node n every action a has
    tried:  Np = N_a + P_a,  q = (W_a - vl * P_a) / Np;     untried:  Np = 0,  q = first_play_value
    e = (prior_n[a] * S[N(n) + P(n)]) * I[Np];   U = q + c * e       S[i] = sqrt(max(i, 1)), I[i] = 1 / (1 + i)   (float64, ties lowest a)
and the best is expanded (untried, budget left), replaced by the best tried child (untried, budget spent; none: leaf = n) or descended.
The leaves are observed, the evaluator gives (priors, value), est = first reward + (leaf terminal ? 0 : value), the backup is the
multi-path one, and the expanded rows then get their priors; roots get theirs when they are made (reset, advance by an untried action).
The test evaluators are functions of the observation row alone built from integer arithmetic and one elementwise float32 division, so
the search and the restatement (other batch sizes, other positions) see the same bytes.  Every statistics word (W as raw float64 bytes,
priors as raw float32 bytes), every tree size, every node and scratch record and the last launch's select outputs must be equal."""
import math

import numpy as np
import pytest

from devmem import _env, _subtree
from test_gpu_uct import NON_DEFAULT, NON_DEFAULT_SEED
from test_gpu_uct_paths import H, KINDS, Restatement, _outputs

pytestmark = pytest.mark.gpu

VL, C, GAMMA = 0.5, 1.25, 0.97
HIGH, LOW = 1.0e4, -1.0e4                                            # above / below every reachable q (|reward| <= 10, gamma 0.97, |value| <= 1)


def make_evaluator(A, peaked):
    """obs -> (priors [S, A], value [S]): per row, integer hashes of the row's values, then one float32 division each."""
    import torch

    def fn(obs):
        x = torch.round(obs.to(torch.float64) * 64.0).to(torch.int64)
        j = torch.arange(x.shape[1], device=obs.device, dtype=torch.int64)
        h = torch.stack([(x * ((j * (2 * a + 3) + a + 1) % 11 + 1)).sum(1) for a in range(A)], 1)      # int64: exact in any order
        if peaked:
            num = torch.remainder(h, 5) + 1
            num[:, A - 1] += 40                                      # peaked on the highest action
        else:
            num = torch.remainder(h, 3) + 50                         # near-uniform
        priors = num.to(torch.float32) / num.sum(1, keepdim=True).to(torch.float32)
        value = (torch.remainder(h.sum(1), 201) - 100).to(torch.float32) / 100.0
        return priors, value

    return fn


class PuctRestatement(Restatement):
    """The PUCT search in python floats, tree by tree, on its own node pool."""

    def __init__(self, env, B, cap, K, vl, horizon, gamma, c, fn, fpv=0.0, max_iterations=64, rows=None):
        super().__init__(env, B, cap, K, vl, horizon, gamma, c, rows)
        self.fn, self.fpv = fn, float(fpv)
        n = max_iterations * K + 1
        self.stab = [math.sqrt(max(i, 1)) for i in range(n)]
        self.itab = [1.0 / (1 + i) for i in range(n)]
        self.prior = np.zeros((B * (cap + K), self.A), np.float32)
        self.roots = np.arange(B) * cap
        self.last_est = None
        self.prime_roots()

    def _eval(self, rows):
        import torch

        p, v = self.fn(self.pool.observe(np.asarray(rows, np.int32)))
        return p.to(torch.float32).cpu().numpy(), v.reshape(-1).to(torch.float64).cpu().numpy()

    def prime_roots(self):
        p, _ = self._eval(self.roots)
        todo = self.visits[self.roots] == 0                          # only_unvisited
        self.prior[self.roots[todo]] = p[todo]

    def _tab(self, t, i):
        return t[min(max(int(i), 0), len(t) - 1)]

    def _select_tree(self, b):
        base, cap, K = b * self.cap, self.cap, self.K
        fresh = base + int(self.used[b])
        P, expander, out = {}, {}, []
        for k in range(K):
            s = b * K + k
            scratch = self.B * cap + s
            n, path, res = base, [], None
            leaf, r = base, np.float32(0)
            for _ in range(cap):
                path.append(n)
                if n >= fresh:
                    res = (base, scratch, 0, n, False, np.float32(0), expander[n])
                    break
                leaf, r = n, self.reward[n]
                if self.terminal[n]:
                    break
                sq = self._tab(self.stab, int(self.visits[n]) + P.get(n, 0))
                best, bu, tried, tu = -1, 0.0, -1, 0.0
                for a in range(self.A):
                    ch = int(self.child[n, a])
                    if ch >= 0:
                        pc = P.get(ch, 0)
                        npc = int(self.visits[ch]) + pc
                        q = (float(self.W[ch]) - self.vl * float(pc)) / float(npc)
                    else:
                        npc, q = 0, self.fpv
                    e = (float(self.prior[n, a]) * sq) * self._tab(self.itab, npc)
                    u = q + self.c * e
                    if best < 0 or u > bu:
                        best, bu = a, u
                    if ch >= 0 and (tried < 0 or u > tu):
                        tried, tu = a, u
                if self.child[n, best] < 0:
                    if self.used[b] < cap:
                        new = base + int(self.used[b])
                        self.used[b] += 1
                        self.child[n, best] = new
                        expander[new] = s
                        path.append(new)
                        res = (n, new, best, new, True, np.float32(0), s)
                        break
                    if tried < 0:                                    # no children and the budget spent
                        break
                    best = tried
                n = int(self.child[n, best])
            if res is None:
                res = (leaf, scratch, 0, leaf, False, r, -1)
            for x in path:
                P[x] = P.get(x, 0) + 1
            out.append(res)
        return out

    def iteration(self):
        import torch

        sel = [r for b in range(self.B) for r in self._select_tree(b)]
        src, dst, act, leaf, exp, rleaf, first = (np.array(x) for x in zip(*sel))
        self.last = dict(src=src, dst=dst, action=act, leaf=leaf, expanded=exp, r_leaf=rleaf.astype(np.float32), first_slot=first)
        self.fresh_hits.append((~exp) & (first >= 0))
        assert not np.isin(src, dst).any()
        t = self.it * (self.H + 1)
        with self.slot_keys():
            _, rew, done = self.pool.transition(torch.as_tensor(act.astype(np.int8)), src=src, dst=dst, t=t, want_obs=False)
        rew, done = rew.cpu().numpy(), done.cpu().numpy()
        first_r = np.where(first >= 0, rew[np.maximum(first, 0)], rleaf.astype(np.float32)).astype(np.float64)
        leaf_term = np.where(first >= 0, done[np.maximum(first, 0)], self.terminal[leaf])
        priors, value = self._eval(leaf)
        est = first_r + np.where(leaf_term, 0.0, value)
        self.last_est, self.last_term = est, leaf_term
        for s in np.nonzero(exp)[0]:                                 # first every expanded row, whole (priors zero)
            x = int(leaf[s])
            self.parent[x], self.action[x], self.reward[x], self.terminal[x] = src[s], act[s], rew[s], done[s]
            self.prior[x] = 0
        for s in range(self.B * self.K):                             # then the walks in slot order
            x = int(leaf[s])
            self.leaf_count[x] += 1
            g = float(est[s])
            for _ in range(self.cap):
                self.visits[x] += 1
                self.W[x] = float(self.W[x]) + g
                p = int(self.parent[x])
                if p < 0:
                    break
                g = float(self.reward[p]) + self.gamma * g
                x = p
        for s in np.nonzero(exp)[0]:                                 # then the expanded rows' priors
            self.prior[int(leaf[s])] = priors[s]
        self.it += 1

    def advance(self, actions):
        old_prior, moves = self.prior.copy(), {}
        for b in range(self.B):
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
        out = super().advance(actions)
        for b, old in moves.items():
            base = int(self.roots[b])
            self.prior[base:base + self.cap] = 0
            self.prior[base + np.arange(len(old))] = old_prior[old]  # a kept node keeps its priors
        self.prime_roots()                                           # a root made from an untried action is unvisited
        return out


def _same_outputs(search, ref):
    got = _outputs(search)
    for k, want in ref.last.items():
        if k == "r_leaf":
            assert got[k].tobytes() == want.tobytes(), k
        else:
            assert np.array_equal(got[k], want), k
    assert search._est.cpu().numpy().tobytes() == ref.last_est.tobytes()
    assert np.array_equal(search._term.cpu().numpy(), ref.last_term)


def _same(search, ref, live_only=False):
    """Every statistics word, tree size and record; live_only: rows [base, base + used) only (after advance() the rest is unspecified)."""
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
    assert np.ascontiguousarray(stats[:, 48:48 + A]).tobytes() == ref.prior[rows].tobytes()         # priors, raw float32 bytes
    assert not stats[:, 39:48].any() and not stats[:, 48 + A:].any()
    assert np.array_equal(search.prior.cpu().numpy()[rows].view(np.int32), np.ascontiguousarray(stats[:, 48:48 + A]))
    ch, has = ref.child[rows], ref.child[rows] >= 0
    mirror_w = np.ascontiguousarray(stats[:, 16:32]).view(np.float64)[:, :A]
    assert np.array_equal(stats[:, 8:8 + A][has], ref.visits[ch[has]]) and not stats[:, 8:8 + A][~has].any()
    assert mirror_w[has].tobytes() == ref.W[ch[has]].tobytes()
    ri = torch.as_tensor(rows, device=search.env.device)
    assert torch.equal(search.pool.records[ri], ref.pool.records[ri])


def _pair(env, B, cap, K, vl, fn, iterations, fpv=None, rows=None, horizon=0, chunks=(None,), budget=None):
    from snac_amd import UCTSearch

    budget = iterations if budget is None else budget
    search = UCTSearch(env, cap, horizon, GAMMA, c=C, max_iterations=budget, trees=B, paths=K, virtual_loss=vl, evaluator=fn,
                       first_play_value=fpv)
    search.reset(rows=rows)
    ref = PuctRestatement(env, B, cap, K, vl, horizon, GAMMA, C, fn, 0.0 if fpv is None else fpv, budget, rows)
    _same(search, ref)                                               # the primed roots
    done = 0
    for k in chunks:
        k = iterations - done if k is None else k
        search.run(k)
        for _ in range(k):
            ref.iteration()
        done += k
        _same(search, ref)
        _same_outputs(search, ref)
        assert (search.visits[search._roots] == done * K).all()
    return search, ref


@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("vl", [0.0, VL])
@pytest.mark.parametrize("K,its", [(1, 30), (2, 20), (5, 10), (16, 5)])
@pytest.mark.parametrize("kind,dyn", KINDS)
def test_puct_search_equals_the_restatement_bit_for_bit(kind, dyn, K, its, vl, peaked):
    import torch

    B, cap = 12, 40
    env = _env(kind, dyn, B, 5 + kind + dyn)
    A = env.num_actions
    rows = torch.arange(B, device=env.device) // 2
    from snac_amd import UCTSearch

    fn = make_evaluator(A, peaked)
    if peaked:                                                       # the first expansion of every root is the prior's argmax
        probe = UCTSearch(env, cap, 0, GAMMA, c=C, max_iterations=1, trees=B, paths=K, virtual_loss=vl, evaluator=fn)
        probe.reset(rows=rows)
        rp = probe.root_priors().cpu().numpy()
        assert rp.dtype == np.float32 and (rp.argmax(1) == A - 1).all()
        probe.run(1)
        torch.cuda.synchronize()
        assert (probe.action.cpu().numpy()[np.arange(B) * cap + 1] == rp.argmax(1)).all()      # not UCB1's lowest untried action
    search, ref = _pair(env, B, cap, K, vl, fn, its, rows=rows, horizon=3 * (K % 2), chunks=(its // 3, None))
    assert (search.tree_sizes().cpu().numpy() > 1).all()
    assert np.array_equal(search.best_actions().cpu().numpy(), np.argmax(search.root_visits().cpu().numpy(), axis=1))


@pytest.mark.parametrize("fpv", [0.0, HIGH, LOW])
@pytest.mark.parametrize("kind,dyn,K", [(2, True, 1), (3, False, 4), (1, True, 2)])
def test_first_play_value_orders_expansion(kind, dyn, K, fpv):
    B, cap, its = 12, 40, 12
    env = _env(kind, dyn, B, 13 + kind)
    A = env.num_actions
    assert cap > A
    search, ref = _pair(env, B, cap, K, VL, make_evaluator(A, False), its, fpv=fpv, chunks=(1, None))
    kids = (ref.child[ref.roots] >= 0).sum(1)
    if fpv == LOW:                                                   # a tried child always beats an untried action: one root child, then below it
        assert (kids == 1).all() and (ref.used > 2).all()
        first = ref.child[ref.roots].max(1)
        assert ((ref.child[first] >= 0).sum(1) >= 1).all()          # grandchildren exist while root actions are unexpanded
    if fpv == HIGH:                                                  # every untried action beats a tried child: breadth first
        assert (kids == A).all()


@pytest.mark.parametrize("kind,dyn,K", [(1, False, 7), (2, True, 16), (3, True, 12)])
def test_paths_stop_on_fresh_rows_with_the_expanders_done(kind, dyn, K):
    """K > A and cap > A: in iteration 0 every non-root row is fresh, so at least K - A slots of every tree stop on fresh rows."""
    import torch

    from snac_amd import _lib

    B, cap = 12, 40
    env = _env(kind, dyn, B, 17 + kind)
    A = env.num_actions
    assert K > A and cap > A
    ts = _lib.env_sizes(kind, dyn).total_step
    env._hdr.view(torch.int16).view(B, 8)[0::3, 3] = ts - 1          # children come back done: terminal fresh rows
    search, ref = _pair(env, B, cap, K, VL, make_evaluator(A, False), 4, chunks=(1,))
    o = _outputs(search)
    on_fresh = (~o["expanded"]) & (o["first_slot"] >= 0)
    assert (on_fresh.reshape(B, K).sum(1) >= K - A).all()
    assert (o["src"][on_fresh] == np.repeat(np.arange(B) * cap, K)[on_fresh]).all()
    done = search._done.cpu().numpy() != 0
    term = search._term.cpu().numpy()
    assert np.array_equal(term[on_fresh], done[o["first_slot"][on_fresh]]) and term[on_fresh].any() and not term[on_fresh].all()
    search.run(3)
    for _ in range(3):
        ref.iteration()
    _same(search, ref)
    _same_outputs(search, ref)


@pytest.mark.parametrize("kind,dyn,cap", [(2, True, 1), (2, True, 2), (1, False, 4), (3, True, 9)])
@pytest.mark.parametrize("K", [1, 5])
def test_budget_exhaustion(kind, dyn, cap, K):
    """cap in {1, 2, A + 1}: best untried with the budget spent falls back to the tried children; no children: leaf = n."""
    B = 12
    env = _env(kind, dyn, B, 21 + cap)
    assert cap in (1, 2, env.num_actions + 1)
    search, ref = _pair(env, B, cap, K, VL, make_evaluator(env.num_actions, True), 12, chunks=(1, 4, None))
    assert (search.tree_sizes().cpu().numpy() == cap).all()
    assert ref.leaf_count[:B * cap].max() > 1


@pytest.mark.parametrize("kind,dyn", KINDS)
def test_terminal_roots_and_terminal_fresh_nodes(kind, dyn):
    import torch

    from snac_amd import _lib

    B, cap, K, its = 24, 32, 10, 6
    env = _env(kind, dyn, B, 31 + kind)
    ts = _lib.env_sizes(kind, dyn).total_step
    cs = env._hdr.view(torch.int16).view(B, 8)[:, 3]
    cs[0::3] = ts - 1
    cs[1::3] = ts - 2
    env._hdr.view(torch.int8).view(B, 16)[2::9, 2] |= _lib.FLAG_NEED_RESET   # terminal roots
    search, ref = _pair(env, B, cap, K, VL, make_evaluator(env.num_actions, False), its, chunks=(1, 3, None))
    term, ch = search.terminal.cpu().numpy(), search.children.cpu().numpy()
    vis, W, r = search.visits.cpu().numpy(), search.value_sum.cpu().numpy(), search.reward.cpu().numpy()
    roots = np.arange(B) * cap
    nonroot = np.arange(len(term)) % cap != 0
    nonroot[B * cap:] = False
    assert term[roots[2::9]].all() and term[nonroot].any()
    assert (ch[term] == -1).all()
    for x in np.nonzero(term)[0]:                                    # the value is never added at a terminal leaf
        w = 0.0
        for _ in range(int(vis[x])):
            w += float(r[x])
        assert W[x].tobytes() == np.float64(w).tobytes()
    assert (search.tree_sizes().cpu().numpy()[2::9] == 1).all() and (vis[roots[2::9]] == its * K).all()


@pytest.mark.parametrize("kind,dyn,K", [(2, True, 5), (3, False, 1), (1, True, 4)])
def test_advance_after_a_puct_run(kind, dyn, K):
    """Tried and untried actions mixed in one batch: kept nodes keep their priors bit for bit, roots made from untried actions get the
    evaluator's priors of their observation, further iterations still match."""
    import torch

    from snac_amd import UCTSearch

    B, cap, n = 12, 64, 10
    env = _env(kind, dyn, B, 71 + kind)
    A = env.num_actions
    fn = make_evaluator(A, False)
    search = UCTSearch(env, cap, 0, GAMMA, c=C, max_iterations=3 * n, trees=B, paths=K, virtual_loss=VL, evaluator=fn, first_play_value=LOW)
    search.reset()
    ref = PuctRestatement(env, B, cap, K, VL, 0, GAMMA, C, fn, LOW, 3 * n)
    search.run(n)
    for _ in range(n):
        ref.iteration()
    _same(search, ref)
    best = search.best_actions().cpu().numpy()
    rc = ref.child[ref.roots]
    a = np.where(np.arange(B) % 2 == 0, best, np.argmax(rc < 0, axis=1))          # even trees: the tried action; odd: an untried one
    tried = rc[np.arange(B), a] >= 0
    assert tried[0::2].all() and not tried[1::2].any()
    before = search.stats.clone().cpu().numpy()
    r, d = search.advance(torch.as_tensor(a, device=env.device))
    er, ed = ref.advance(a)
    _same(search, ref, live_only=True)
    assert r.cpu().numpy().tobytes() == er.tobytes() and np.array_equal(d.cpu().numpy(), ed)
    after = search.stats.cpu().numpy()
    sizes = search.tree_sizes().cpu().numpy()
    want = fn(search.pool.observe(search._roots))[0].cpu().numpy()
    for b in range(B):
        base = b * cap
        if tried[b]:
            old = _subtree(before[:, :A], int(before[base, a[b]]), [])
            new = _subtree(after[:, :A], base, [])
            assert len(old) == len(new) == sizes[b]
            assert np.array_equal(before[old][:, 48:56], after[new][:, 48:56]) and before[old][:, 48:48 + A].any()
        else:
            assert sizes[b] == 1 and after[base, 35] == 0
            assert np.ascontiguousarray(after[base, 48:48 + A]).tobytes() == want[b].tobytes()
    for chunk in (3, n - 3):
        search.run(chunk)
        for _ in range(chunk):
            ref.iteration()
        _same(search, ref, live_only=True)
        _same_outputs(search, ref)
    assert search.iterations == 2 * n


@pytest.mark.parametrize("kind,dyn,K", [(2, True, 1), (3, False, 4)])
def test_no_evaluator_is_the_default_search(kind, dyn, K):
    import torch

    from snac_amd import UCTSearch

    B, cap, n = 32, 40, 20
    env = _env(kind, dyn, B, 11 + kind)
    a = UCTSearch(env, cap, H[kind] // 4, GAMMA, max_iterations=n, trees=B, paths=K, virtual_loss=VL)
    b = UCTSearch(env, cap, H[kind] // 4, GAMMA, max_iterations=n, trees=B, paths=K, virtual_loss=VL, evaluator=None, first_play_value=None)
    for s in (a, b):
        s.reset()
        s.run(n)
    torch.cuda.synchronize()
    assert torch.equal(a.stats, b.stats) and torch.equal(a.pool.records, b.pool.records) and torch.equal(a.tree_sizes(), b.tree_sizes())
    assert not b.stats[:, 39:].any() and not b.prior.any() and not b.root_priors().any()
    with pytest.raises(ValueError):
        b.set_root_priors(torch.zeros(B, env.num_actions))


def test_set_root_priors_then_run():
    import torch

    from snac_amd import UCTSearch

    B, cap, K, n = 12, 40, 3, 10
    env = _env(2, True, B, 7)
    A = env.num_actions
    fn = make_evaluator(A, False)
    search = UCTSearch(env, cap, 0, GAMMA, c=C, max_iterations=n, trees=B, paths=K, virtual_loss=VL, evaluator=fn)
    search.reset()
    ref = PuctRestatement(env, B, cap, K, VL, 0, GAMMA, C, fn, 0.0, n)
    g = torch.Generator().manual_seed(5)
    noise = torch.rand((B, A), generator=g, dtype=torch.float64)
    p = (0.75 * search.root_priors().cpu().to(torch.float64) + 0.25 * noise / noise.sum(1, keepdim=True)).to(torch.float32)
    search.set_root_priors(p)
    ref.prior[ref.roots] = p.numpy()
    assert search.root_priors().cpu().numpy().tobytes() == p.numpy().tobytes()
    search.run(n)
    for _ in range(n):
        ref.iteration()
    _same(search, ref)
    _same_outputs(search, ref)
    with pytest.raises(ValueError):
        search.set_root_priors(p[:, :A - 1])


def test_puct_run_does_not_synchronise_with_the_host():
    import torch

    from snac_amd import UCTSearch

    env = _env(2, True, 64, 3)
    K = 8
    search = UCTSearch(env, 64, 0, GAMMA, max_iterations=32, paths=K, virtual_loss=VL, evaluator=make_evaluator(env.num_actions, False))
    search.reset()
    search.run(2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        search.run(10)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert (search.visits[search._roots] == 12 * K).all()
    with pytest.raises(ValueError):
        search.run(21)


@pytest.mark.parametrize("kind,dyn", [(2, True), (3, False)])
def test_a_captured_puct_run_replays_as_the_search(kind, dyn):
    """A graph of run(n) (one stream, no parallel branches) replayed after reset() leaves what run(n) leaves."""
    import torch

    from snac_amd import UCTSearch

    B, n, K = 32, 12, 6
    env = _env(kind, dyn, B, 41 + kind)
    search = UCTSearch(env, 48, 0, 0.95, max_iterations=n, paths=K, virtual_loss=VL, evaluator=make_evaluator(env.num_actions, True))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # warm-up outside capture (torch's capture protocol)
        search.reset()
        search.run(2)
    torch.cuda.current_stream().wait_stream(side)
    search.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        search.run(n)
    search.reset()
    g.replay()
    torch.cuda.synchronize()
    stats, records = search.stats.clone(), search.pool.records.clone()
    search.reset()
    search.run(n)
    torch.cuda.synchronize()
    assert torch.equal(search.stats, stats) and torch.equal(search.pool.records, records)
    assert (search.visits[search._roots] == n * K).all()


@pytest.mark.parametrize("kind,dyn,K", [(2, True, 4), (1, False, 1), (3, True, 8)])
def test_a_torch_network_guides_the_search(kind, dyn, K):
    """A small float32 MLP (softmax policy, tanh value): invariants only."""
    import torch

    from snac_amd import UCTSearch

    B, cap, n = 16, 64, 12
    env = _env(kind, dyn, B, 61 + kind)
    A = env.num_actions
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(env.obs_dim, 32), torch.nn.ReLU(), torch.nn.Linear(32, A + 1)).to(env.device)

    @torch.no_grad()
    def fn(obs):
        y = net(obs.to(torch.float32))
        return torch.softmax(y[:, :A], 1), torch.tanh(y[:, A])

    search = UCTSearch(env, cap, 0, GAMMA, c=C, max_iterations=n, trees=B, paths=K, virtual_loss=VL, evaluator=fn)
    search.reset()
    times_leaf = np.zeros(search.rows, np.int64)
    for _ in range(n):
        search.run(1)
        np.add.at(times_leaf, search._leaf.cpu().numpy(), 1)
    torch.cuda.synchronize()
    vis, ch = search.visits.cpu().numpy(), search.children.cpu().numpy()
    sizes = search.tree_sizes().cpu().numpy()
    live = np.concatenate([b * cap + np.arange(int(sizes[b])) for b in range(B)])
    assert (vis[np.arange(B) * cap] == n * K).all()
    kids = np.where(ch >= 0, vis[np.maximum(ch, 0)], 0).sum(1)
    assert np.array_equal(vis[live], (kids + times_leaf)[live])
    pr = search.prior.cpu().numpy()[live].astype(np.float64)
    assert (pr >= 0).all() and np.abs(pr.sum(1) - 1.0).max() <= 4 * A * 2.0 ** -24          # the float32 softmax's own rounding
    assert not search.stats[torch.as_tensor(live, device=env.device), 39:48].any()
    assert np.isfinite(search.value_sum.cpu().numpy()).all() and (sizes > 1).all()


@pytest.mark.parametrize("kind,dyn,K", [(2, True, 5)])
def test_puct_search_on_a_non_default_env_equals_the_restatement_bit_for_bit(kind, dyn, K):
    """env_id_base 1000, a 64-bit seed, brick_gt / time_gt, total_step 9 and an action distribution: the slots' keys start at 1000 * K."""
    B, cap, its = 12, 40, 10
    env = _env(kind, dyn, B, NON_DEFAULT_SEED, **NON_DEFAULT)
    assert env.env_id_base == 1000 and env.seed >> 32 == 9 and env.total_step == 9 and env.brick_gt and env.time_gt
    search, ref = _pair(env, B, cap, K, VL, make_evaluator(env.num_actions, False), its, horizon=3, chunks=(its // 3, None))
    assert (search.tree_sizes().cpu().numpy() > 1).all()
