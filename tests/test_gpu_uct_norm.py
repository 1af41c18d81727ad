"""GPU: the search with q normalised by per-tree min-max bounds (UCTSearch(q_normalise=True); snac_uct_select_paths_norm /
snac_uct_select_puct_norm / snac_uct_backup_paths_norm / snac_uct_bounds, k_uct.hip) against a restatement in python floats of the
rule of include/snac_hip.h ("Normalised q").

The rule, restated on top of the restatements of the multi-path search (tests/test_gpu_uct_paths.py) and of PUCT
(tests/test_gpu_uct_puct.py).  Tree b has a pair (lo, hi) of float64, empty = (+inf, -inf).  Selection reads the pair as the launch
finds it; the q of a TRIED child, (W_a - vl * P_a) / Np, becomes (q - lo) / (hi - lo) where hi > lo and stays as it is otherwise; an
untried action's first_play_value is used as given; nothing else changes.  Backup: right after a node below the root has its new
visits and value_sum, m = value_sum / visits enters the pair by  lo = m < lo ? m : lo;  hi = m > hi ? m : hi,  in slot order, then walk
order.  advance() recomputes every tree's pair, restart(mask) the masked trees', from the nodes the tree has then: min / max of
value_sum / visits over its rows below the root with visits > 0; no such row: empty.
Every comparison is bit for bit: every statistics word, tree size and record, the select outputs, est, and the raw bytes of q_bounds."""
import ctypes as C
import math

import numpy as np
import pytest

from devmem import _env
from test_gpu_uct_paths import H, VL, Restatement, _outputs
from test_gpu_uct_paths import _same as _same_rollout
from test_gpu_uct_paths import _same_outputs as _same_outputs_rollout
from test_gpu_uct_puct import C as CPUCT
from test_gpu_uct_puct import GAMMA, LOW, PuctRestatement, make_evaluator
from test_gpu_uct_puct import _same as _same_puct
from test_gpu_uct_puct import _same_outputs as _same_outputs_puct
from test_gpu_uct_selfplay import _near_the_end, pick, restart

pytestmark = pytest.mark.gpu

KINDS = [(1, False), (2, True), (3, True)]                           # A = 3, 5, 8
SCALE = 50.0                                                         # the evaluator's value times this: q far outside [-1, 1]


def scaled_evaluator(A, peaked=False):
    """make_evaluator with its value times SCALE (one elementwise float32 product: the same bytes at every batch size)."""
    base = make_evaluator(A, peaked)

    def fn(obs):
        p, v = base(obs)
        return p, v * SCALE

    return fn


# ---- the restatements ---------------------------------------------------------------------------------------------------------------------
class _Bounds:
    """The bounds and what reads and writes them, for both restatements."""

    def _init_bounds(self):
        self.bounds = np.tile(np.array([np.inf, -np.inf]), (self.B, 1))
        self.last_est = None

    def _q(self, b, q):
        lo, hi = float(self.bounds[b, 0]), float(self.bounds[b, 1])
        if hi > lo:
            q = (q - lo) / (hi - lo)
        return q

    def _fold(self, b, m):
        lo, hi = float(self.bounds[b, 0]), float(self.bounds[b, 1])
        self.bounds[b, 0] = m if m < lo else lo
        self.bounds[b, 1] = m if m > hi else hi

    def _walks(self, leaf, est):
        for s in range(self.B * self.K):                             # the walks in slot order
            b, x = s // self.K, int(leaf[s])
            self.leaf_count[x] += 1
            g = float(est[s])
            for _ in range(self.cap):
                self.visits[x] += 1
                self.W[x] = float(self.W[x]) + g
                p = int(self.parent[x])
                if p < 0:
                    break
                self._fold(b, float(self.W[x]) / float(self.visits[x]))      # x is below the root
                g = float(self.reward[p]) + self.gamma * g
                x = p

    def rebound(self, mask=None):
        """The bounds of the trees with mask[b] != 0 (None: all) from their nodes as they stand."""
        for b in range(self.B):
            if mask is not None and not mask[b]:
                continue
            self.bounds[b] = (np.inf, -np.inf)
            used = min(max(int(self.used[b]), 1), self.cap)
            for x in range(b * self.cap + 1, b * self.cap + used):
                if self.visits[x] > 0:
                    self._fold(b, float(self.W[x]) / float(self.visits[x]))

    def advance(self, actions):
        out = super().advance(actions)
        self.rebound()
        return out


class NormRestatement(_Bounds, Restatement):
    """The rollout search with normalised q."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self._init_bounds()

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
                untried = [a for a in range(self.A) if self.child[n, a] < 0]
                if untried and self.used[b] < cap:
                    new = base + int(self.used[b])
                    self.used[b] += 1
                    self.child[n, untried[0]] = new
                    expander[new] = s
                    path.append(new)
                    res = (n, new, untried[0], new, True, np.float32(0), s)
                    break
                if not (self.child[n] >= 0).any():                  # no children and the budget spent
                    break
                best, bu = -1, 0.0
                lg = math.sqrt(math.log(int(self.visits[n]) + P.get(n, 0)))
                for a in range(self.A):
                    ch = int(self.child[n, a])
                    if ch < 0:
                        continue
                    pc = P.get(ch, 0)
                    npc = int(self.visits[ch]) + pc
                    q = self._q(b, (float(self.W[ch]) - self.vl * float(pc)) / float(npc))
                    e = lg * (1.0 / math.sqrt(npc))
                    u = q + self.c * e
                    if best < 0 or u > bu:
                        best, bu = a, u
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
        t = self.it * (self.H + 1)
        with self.slot_keys():
            _, rew, done = self.pool.transition(torch.as_tensor(act.astype(np.int8)), src=src, dst=dst, t=t, want_obs=False)
            rew, done = rew.cpu().numpy(), done.cpu().numpy()
            first_r = np.where(first >= 0, rew[np.maximum(first, 0)], rleaf.astype(np.float32)).astype(np.float64)
            est, _ = self.pool.evaluate(torch.as_tensor(leaf), self.H, self.gamma, first_reward=torch.as_tensor(first_r), t0=t + 1)
        est = est.cpu().numpy()
        self.last_est = est
        for s in np.nonzero(exp)[0]:                                 # first every expanded row, whole
            x = int(leaf[s])
            self.parent[x], self.action[x], self.reward[x], self.terminal[x] = src[s], act[s], rew[s], done[s]
        self._walks(leaf, est)
        self.it += 1


class NormPuctRestatement(_Bounds, PuctRestatement):
    """The PUCT search with normalised q."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self._init_bounds()

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
                        q = self._q(b, (float(self.W[ch]) - self.vl * float(pc)) / float(npc))
                    else:
                        npc, q = 0, self.fpv                         # as given: in normalised units
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
        self._walks(leaf, est)
        for s in np.nonzero(exp)[0]:                                 # then the expanded rows' priors
            self.prior[int(leaf[s])] = priors[s]
        self.it += 1


# ---- comparing ----------------------------------------------------------------------------------------------------------------------------
def _same(search, ref, live_only=False, outputs=True):
    import torch

    puct = search.evaluator is not None
    (_same_puct if puct else _same_rollout)(search, ref, live_only=live_only)
    if outputs and ref.last is not None:
        if puct:
            _same_outputs_puct(search, ref)                          # est and the leaves' terminal flags included
        else:
            _same_outputs_rollout(search, ref)
            assert search._est.cpu().numpy().tobytes() == ref.last_est.tobytes()
    torch.cuda.synchronize()
    if getattr(search, "q_normalise", False):
        got = search.q_bounds_of_trees()
        assert tuple(got.shape) == (ref.B, 2) and got.dtype == torch.float64
        assert got.cpu().numpy().tobytes() == ref.bounds.tobytes(), (got.cpu().numpy(), ref.bounds)
        assert search.q_bounds.cpu().numpy().tobytes() == ref.bounds.tobytes()


def _puct_pair(env, B, cap, K, vl, fn, budget, fpv=None, normalise=True):
    from snac_amd import UCTSearch

    search = UCTSearch(env, cap, 0, GAMMA, c=CPUCT, max_iterations=budget, trees=B, paths=K, virtual_loss=vl, evaluator=fn, first_play_value=fpv,
                       q_normalise=normalise)
    search.reset()
    cls = NormPuctRestatement if normalise else PuctRestatement
    ref = cls(env, B, cap, K, vl, 0, GAMMA, CPUCT, fn, 0.0 if fpv is None else fpv, budget)
    return search, ref


def _rollout_pair(env, B, cap, K, vl, horizon, budget, normalise=True):
    from snac_amd import UCTSearch

    search = UCTSearch(env, cap, horizon, GAMMA, max_iterations=budget, trees=B, paths=K, virtual_loss=vl, q_normalise=normalise)
    search.reset()
    ref = (NormRestatement if normalise else Restatement)(env, B, cap, K, vl, horizon, GAMMA, math.sqrt(2))
    return search, ref


def _run_both(search, ref, n):
    search.run(n)
    for _ in range(n):
        ref.iteration()


def _empty(bounds):
    return np.isposinf(bounds[:, 0]) & np.isneginf(bounds[:, 1])


# ---- 1. PUCT ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vl", [0.0, 0.5])
@pytest.mark.parametrize("K,its", [(1, 30), (5, 10), (16, 5)])
@pytest.mark.parametrize("kind,dyn", KINDS)
def test_normalised_puct_search_equals_the_restatement_bit_for_bit(kind, dyn, K, its, vl):
    B, cap = 3, 40
    env = _env(kind, dyn, B, 5 + kind + dyn)
    search, ref = _puct_pair(env, B, cap, K, vl, scaled_evaluator(env.num_actions), its)
    _same(search, ref)                                               # the primed roots, empty bounds
    assert _empty(ref.bounds).all()
    done = 0
    for k in (1, 2, None):                                           # the first iterations select with empty bounds, then with hi == lo
        k = its - done if k is None else k
        _run_both(search, ref, k)
        done += k
        _same(search, ref)
        if done == 1 and K == 1:                                     # one mean so far
            assert (ref.bounds[:, 0] == ref.bounds[:, 1]).all()
    assert (ref.bounds[:, 1] > ref.bounds[:, 0]).all()
    assert (ref.bounds[:, 1] - ref.bounds[:, 0]).max() > 2.0         # q spans well beyond the unit interval: normalisation matters
    assert (search.visits[search._roots] == its * K).all()


# ---- 2. the rollout search ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("kind,dyn", KINDS)
def test_normalised_rollout_search_equals_the_restatement_bit_for_bit(kind, dyn, K):
    """K = 1 goes through the paths entry points (there is no one-path _norm form): first_slot arrays and all."""
    B, cap, its = 3, 40, 12
    env = _env(kind, dyn, B, 7 + kind + dyn)
    search, ref = _rollout_pair(env, B, cap, K, VL, H[kind], its)
    assert search._multi and search._first_slot is not None
    done = 0
    for k in (1, 2, None):
        k = its - done if k is None else k
        _run_both(search, ref, k)
        done += k
        _same(search, ref)
    assert (ref.bounds[:, 1] > ref.bounds[:, 0]).all()
    assert (search.visits[search._roots] == its * K).all()


# ---- 3. two blocks of the lane-per-tree kernels ---------------------------------------------------------------------------------------------
def test_trees_on_both_sides_of_a_block_boundary_and_a_spent_budget():
    """B = 70: trees 63 and 64 are the last lane of block 0 and the first of block 1; cap = 9 spends the node budget, so the best of
    the tried children is chosen by normalised q."""
    B, cap, K, its = 70, 9, 2, 6
    env = _env(2, True, B, 29)
    search, ref = _puct_pair(env, B, cap, K, 0.5, scaled_evaluator(env.num_actions), its)
    _run_both(search, ref, its)
    _same(search, ref)
    got = search.q_bounds_of_trees().cpu().numpy()
    stats = search.stats.cpu().numpy()
    for b in (63, 64):
        rows = slice(b * cap, (b + 1) * cap)
        assert got[b].tobytes() == ref.bounds[b].tobytes() and got[b, 1] > got[b, 0]
        assert np.array_equal(stats[rows, 35], ref.visits[rows]) and np.ascontiguousarray(stats[rows, 36:38]).tobytes() == ref.W[rows].tobytes()
    print("trees with the budget spent: %d of %d" % (int((ref.used == cap).sum()), B))
    assert (ref.used == cap).any()                                   # the input: a spent budget somewhere


# ---- 4. snac_uct_bounds on written statistics ---------------------------------------------------------------------------------------------
def _want_bounds(visits, W, used, cap):
    out = np.zeros((len(used), 2))
    for b, u in enumerate(used):
        rows = np.arange(b * cap + 1, b * cap + min(max(int(u), 1), cap))
        rows = rows[visits[rows] > 0]
        m = W[rows] / visits[rows].astype(np.float64)
        m = m[~np.isnan(m)]
        out[b] = (m.min(), m.max()) if len(m) else (np.inf, -np.inf)
    return out


def test_bounds_of_written_statistics():
    import torch

    from snac_amd import UCTSearch

    B, cap = 7, 200
    used = np.array([1, 2, 63, 64, 65, 130, 200], np.int32)
    env = _env(2, True, B, 3)
    search = UCTSearch(env, cap, 0, GAMMA, max_iterations=4, q_normalise=True)
    search.reset()
    rng = np.random.default_rng(11)
    R = search.rows
    visits = rng.integers(0, 6, size=R).astype(np.int32)             # about a sixth of the rows unvisited
    W = rng.normal(scale=300.0, size=R) + 0.125                      # no mean is a zero
    roots = np.arange(B) * cap
    visits[roots], W[roots] = 3, 1.0e40                              # a root's mean never enters
    visits[roots + 1] = np.maximum(visits[roots + 1], 1)
    for b in range(B):                                               # the rows past `used` hold huge values that must be ignored
        dead = np.arange(b * cap + used[b], (b + 1) * cap)
        visits[dead], W[dead] = 1, np.where(dead % 2 == 0, 1.0e30, -1.0e30)
    last = 5 * cap + used[5] - 1
    visits[last], W[last] = 2, 2.0e6                                 # the largest mean in the last used row of tree 5
    visits[3 * cap + 1], W[3 * cap + 1] = 4, -4.0e6                  # the smallest in row 1 of tree 3
    nan_row = 6 * cap + 77
    visits[nan_row], W[nan_row] = 2, np.nan                          # a NaN sum never enters
    unvisited = 4 * cap + 5
    visits[unvisited], W[unvisited] = 0, 9.0e9                       # visits == 0: skipped whatever its sum
    stats = search.stats.cpu().numpy()
    stats[:, 35] = visits
    stats[:, 36:38] = W.view(np.int32).reshape(R, 2)
    search.stats.copy_(torch.as_tensor(stats))
    search._used.copy_(torch.as_tensor(used))
    want = _want_bounds(visits, W, used, cap)
    assert _empty(want)[0] and want[1, 0] == want[1, 1] and want[5, 1] == 1.0e6 and want[3, 0] == -1.0e6 and np.isfinite(want[1:]).all()
    assert (visits[: B * cap] == 0).sum() > B and np.abs(want[1:]).max() < 1.0e7

    search._rebound(None)
    torch.cuda.synchronize()
    assert search.q_bounds.cpu().numpy().tobytes() == want.tobytes()

    sentinel = np.tile(np.array([123.5, -7.25]), (B, 1))             # not a pair the kernel could have made
    mask = np.ones(B, np.uint8)
    mask[[2, 5]] = 0
    search.q_bounds.copy_(torch.as_tensor(sentinel))
    search._rebound(torch.as_tensor(mask, device=env.device))
    torch.cuda.synchronize()
    masked = np.where(mask[:, None] != 0, want, sentinel)
    assert search.q_bounds.cpu().numpy().tobytes() == masked.tobytes()

    # the entry point itself, with a used[] outside [1, cap]: clamped
    wild = used.copy()
    wild[0], wild[6] = -5, cap + 1000
    search._used.copy_(torch.as_tensor(wild))
    L = search._lib
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.snac_uct_bounds(p(search.stats), search.rows, B, cap, p(search._used), None, p(search.q_bounds), env._stream()) == 0
    torch.cuda.synchronize()
    assert search.q_bounds.cpu().numpy().tobytes() == want.tobytes()


# ---- 5. advance() and restart() -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fpv", [LOW, 0.0])
def test_bounds_follow_advance_and_restart(fpv):
    """fpv far below every q keeps untried actions at every root (the untried case); fpv = 0 grows bushy trees (kept subtrees whose
    bounds are narrower than the tree's)."""
    import torch

    from snac_amd import _lib

    B, cap, K = 4, 64, 5
    env = _env(2, True, B, 71)
    env._hdr.view(torch.int8).view(B, 16)[2, 2] |= _lib.FLAG_NEED_RESET       # root 2 is terminal
    search, ref = _puct_pair(env, B, cap, K, 0.5, scaled_evaluator(env.num_actions), 20, fpv=fpv)
    _run_both(search, ref, 10)
    _same(search, ref)
    rc = ref.child[ref.roots]
    best = search.best_actions().cpu().numpy()
    a = best.copy()
    has_untried = (rc[1] < 0).any()
    if has_untried:
        a[1] = int(np.argmax(rc[1] < 0))                             # tree 1: an untried action
    assert rc[0, a[0]] >= 0 and rc[3, a[3]] >= 0 and ref.terminal[ref.roots[2]]
    if fpv == LOW:
        assert has_untried
    before = ref.bounds.copy()
    r, d = search.advance(torch.as_tensor(a, device=env.device))
    er, ed = ref.advance(a)
    assert r.cpu().numpy().tobytes() == er.tobytes() and np.array_equal(d.cpu().numpy(), ed)
    _same(search, ref, live_only=True, outputs=False)
    assert _empty(ref.bounds)[2] and (not has_untried or _empty(ref.bounds)[1])          # one-node trees
    for b in (0, 3):                                                 # a kept subtree: the bounds of its own nodes
        assert ref.used[b] > 2 and before[b, 0] <= ref.bounds[b, 0] and ref.bounds[b, 1] <= before[b, 1]
    _run_both(search, ref, 5)
    _same(search, ref, live_only=True)
    mask = np.array([1, 0, 1, 0], bool)
    kept = search.q_bounds_of_trees().cpu().numpy()
    search.restart(torch.as_tensor(mask, device=env.device))
    restart(ref, mask)
    ref.rebound(mask)
    _same(search, ref, live_only=True, outputs=False)
    now = search.q_bounds_of_trees().cpu().numpy()
    assert _empty(now)[mask].all() and now[~mask].tobytes() == kept[~mask].tobytes() and not _empty(now)[~mask].any()
    _run_both(search, ref, 5)
    _same(search, ref, live_only=True)
    assert search.iterations == 20


# ---- 6. SelfPlay ------------------------------------------------------------------------------------------------------------------------------
def test_self_play_on_a_normalised_puct_search_equals_the_restatement_move_by_move():
    import torch

    from snac_amd import SelfPlay, UCTSearch, _lib

    B, cap, K, its, moves, sample_moves = 4, 48, 3, 4, 6, 2
    ts = _lib.env_sizes(2, True).total_step
    prep = _near_the_end(2, True)
    env, renv = _env(2, True, B, 39), _env(2, True, B, 39)           # play() resets env rows: the restatement follows on a twin
    for e in (env, renv):
        prep(e)
    fn = scaled_evaluator(env.num_actions)
    budget = (ts + 1) * its
    search = UCTSearch(env, cap, 0, GAMMA, c=CPUCT, max_iterations=budget, paths=K, virtual_loss=0.5, evaluator=fn, q_normalise=True)
    search.reset()
    ref = NormPuctRestatement(renv, B, cap, K, 0.5, 0, GAMMA, CPUCT, fn, 0.0, budget)
    play = SelfPlay(search, moves, sample_moves=sample_moves)
    play.play(2, its)
    play.play(moves - 2, its)
    torch.cuda.synchronize()
    A = env.num_actions
    want = dict(pi=np.zeros((moves, B, A), np.float32), value=np.zeros((moves, B), np.float32), action=np.zeros((moves, B), np.int8),
                reward=np.zeros((moves, B), np.float32), done=np.zeros((moves, B), np.uint8), move=np.zeros((moves, B), np.int32))
    obs = []
    in_episode, restarts = np.zeros(B, np.int64), np.zeros(B, np.int64)
    roots = torch.arange(B, device=env.device) * cap
    for mv in range(moves):
        for _ in range(its):
            ref.iteration()
        obs.append(ref.pool.observe(roots))
        a, pi, v = pick(ref, in_episode >= sample_moves, mv)
        r, d = ref.advance(a)                                        # re-rooted: every tree's bounds from its kept nodes
        want["pi"][mv], want["value"][mv], want["action"][mv], want["reward"][mv], want["done"][mv], want["move"][mv] = pi, v, a, r, d, in_episode
        renv.reset(mask=torch.as_tensor(d, device=env.device), want_obs=False)
        restart(ref, d)
        ref.rebound(d)                                               # a restarted tree: empty
        restarts += d
        in_episode = np.where(d, 0, in_episode + 1)
    assert (restarts > 0).any() and (restarts == 0).any()            # the inputs: trees that restarted and trees that did not
    for s in range(moves):
        assert torch.equal(play.obs[s], obs[s]), s
    for k, w in want.items():
        assert getattr(play, k).cpu().numpy().tobytes() == w.tobytes(), k
    _same(search, ref, live_only=True, outputs=False)
    assert torch.equal(env._hdr, renv._hdr)


# ---- 7. off means off ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("puct", [False, True])
def test_q_normalise_false_is_the_search_without_the_argument(puct):
    import torch

    from snac_amd import UCTSearch

    B, cap, K, n = 12, 40, 4, 8
    env = _env(2, True, B, 19)
    kw = dict(c=CPUCT, evaluator=scaled_evaluator(env.num_actions)) if puct else {}
    a = UCTSearch(env, cap, 0 if puct else H[2] // 4, GAMMA, max_iterations=n, trees=B, paths=K, virtual_loss=VL, **kw)
    b = UCTSearch(env, cap, 0 if puct else H[2] // 4, GAMMA, max_iterations=n, trees=B, paths=K, virtual_loss=VL, q_normalise=False, **kw)
    for s in (a, b):
        s.reset()
        s.run(n)
    torch.cuda.synchronize()
    assert torch.equal(a.stats, b.stats) and torch.equal(a.tree_sizes(), b.tree_sizes()) and torch.equal(a.pool.records, b.pool.records)
    oa, ob = _outputs(a), _outputs(b)
    for k in oa:
        assert oa[k].tobytes() == ob[k].tobytes(), k
    assert a.q_bounds is None and b.q_bounds is None and a.q_normalise is False and b.q_normalise is False
    with pytest.raises(ValueError):
        b.q_bounds_of_trees()


# ---- 8. normalisation changes the search where it should ------------------------------------------------------------------------------------
def test_normalisation_changes_the_search():
    B, cap, its = 6, 40, 30
    env = _env(2, True, B, 23)
    fn = scaled_evaluator(env.num_actions)
    on, ref_on = _puct_pair(env, B, cap, 1, 0.0, fn, its, normalise=True)
    off, ref_off = _puct_pair(env, B, cap, 1, 0.0, fn, its, normalise=False)
    for _ in range(its):
        ref_on.iteration()
        ref_off.iteration()

    def root_visits(ref):
        ch = ref.child[ref.roots]
        return np.where(ch >= 0, ref.visits[np.maximum(ch, 0)], 0)

    assert not np.array_equal(root_visits(ref_on), root_visits(ref_off))     # else the case proves nothing
    on.run(its)
    off.run(its)
    _same(on, ref_on)
    _same(off, ref_off)
    assert np.array_equal(on.root_visits().cpu().numpy(), root_visits(ref_on))
    assert np.array_equal(off.root_visits().cpu().numpy(), root_visits(ref_off))


# ---- 9. no host synchronisation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("puct", [False, True])
def test_a_normalised_search_does_not_synchronise_with_the_host(puct):
    import torch

    from snac_amd import UCTSearch

    B, K = 64, 4
    env = _env(2, True, B, 3)
    kw = dict(evaluator=scaled_evaluator(env.num_actions)) if puct else {}
    search = UCTSearch(env, 64, 0 if puct else 50, GAMMA, max_iterations=32, paths=K, virtual_loss=VL, q_normalise=True, **kw)
    search.reset()
    mask = torch.arange(B, device=env.device) % 3 == 0
    search.run(2)                                                    # warm-up: every kernel and torch op of the guarded window
    search.advance(search.best_actions(), check=False)
    search.restart(mask)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        search.run(6)
        search.advance(search.best_actions(), check=False)
        search.run(2)
        search.restart(mask)
        search.run(2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert search.iterations == 12
    b = search.q_bounds_of_trees().cpu().numpy()
    assert (b[:, 1] >= b[:, 0]).all()                                # every tree ran two iterations since: no pair is empty


# ---- 10. sharding -------------------------------------------------------------------------------------------------------------------------
def test_a_sharded_normalised_search_is_the_whole_search():
    """In the manner of tests/test_gpu_uct_sharding.py: trees [off, off + n) of the whole batch and the shard with env_id_base + off."""
    import torch

    from snac_amd import UCTSearch

    import test_gpu_uct_sharding as sh

    K = 4
    whole_env, shards = sh._envs(2, True)
    sh._near_the_end(whole_env, 0)
    for off, e in shards:
        sh._near_the_end(e, off)

    def make(env):
        s = UCTSearch(env, nodes_per_tree=sh.CAP, horizon=0, gamma=sh.GAMMA, c=CPUCT, max_iterations=24, paths=K, virtual_loss=sh.VL,
                      evaluator=scaled_evaluator(env.num_actions), q_normalise=True)
        s.reset()
        s.run(14)
        return s

    whole = make(whole_env)
    picks = whole.best_actions()
    whole.advance(picks)
    whole.run(6)
    torch.cuda.synchronize()
    wb = whole.q_bounds_of_trees().cpu().numpy()
    assert (wb[:, 1] > wb[:, 0]).any() and len({wb[g].tobytes() for g in range(sh.N)}) > 1
    for off, e in shards:
        s = make(e)
        n = s.trees
        assert torch.equal(s.best_actions(), picks[off:off + n])
        s.advance(picks[off:off + n])
        s.run(6)
        sh._same_trees(s, whole, off, live_only=True)
        assert s.q_bounds_of_trees().cpu().numpy().tobytes() == wb[off:off + n].tobytes(), off
