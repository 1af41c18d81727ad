"""GPU: the Gumbel root search (UCTSearch(gumbel=m), SelfPlay(gumbel=True); snac_uct_select_gumbel, k_uct.hip; snac_uct_gumbel_candidates,
k_uct_play.hip) against a restatement in python floats of the rules of include/snac_hip.h ("Gumbel root").

The rules, restated on top of the normalised PUCT restatement (tests/test_gpu_uct_norm.py).  Tree b has a candidate mask cand[b] over its
root actions.  BEGIN: 0 at a terminal root, else the min(m, A) largest scores (float32, NaN as -inf), one at a time by strict >, scanning a
upward.  A launch with offset o: at the root of a tree with candidates c_0 < ... < c_{M-1}, path k takes a = c[(o + k) mod M]: tried --
descend; untried with budget -- expand; untried without -- stop at the root (a stored leaf).  Everywhere else, and in a tree without
candidates, the rule is the normalised PUCT one.  HALVE keeps the (M + 1) // 2 candidates of largest rank, PICK takes the largest, where
    rank = float(score) + ((c_visit + maxN) * c_scale) * q,   q = visited ? normalised W_a / N_a : first_play_value
(a tree without candidates: the most-visited action).  gumbel_run(n) follows gumbel_schedule(n, min(m, A)): phases of n // phases
iterations (the last takes the rest), a HALVE before every phase but the first, iteration i of a phase with offset i * K.
Every comparison is bit for bit -- every statistics word, tree size, record, select output, est, the bytes of q_bounds, cand, the moves --
except improved_policy(), a float64 torch computation compared with a float64 NumPy one within 1e-6."""
import numpy as np
import pytest

from devmem import _env
from test_gpu_uct_norm import NormPuctRestatement, _empty, _same, scaled_evaluator
from test_gpu_uct_paths import _outputs
from test_gpu_uct_puct import C as CPUCT
from test_gpu_uct_puct import GAMMA
from test_gpu_uct_selfplay import _near_the_end, pick, restart

pytestmark = pytest.mark.gpu

VL = 0.5
C_VISIT, C_SCALE = 50.0, 1.0                                         # the defaults of UCTSearch
# improved_policy(): both sides are float64 computations rounded to float32 probabilities <= 1, whose ulp is at most 6e-8; about 16 ulp
# cover the differing exp / log implementations
PI_ATOL = 1.0e-6


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def _phases(n, m):
    """[(halve, i)] of n iterations over m candidates, restated: ceil(log2 m) phases (at least one), the last takes the remainder."""
    phases = 1
    while (1 << phases) < m:
        phases += 1
    assert n >= phases
    L = n // phases
    lengths = [L] * (phases - 1) + [n - L * (phases - 1)]
    return [(p > 0 and i == 0, i) for p, ln in enumerate(lengths) for i in range(ln)]


def _take(rank, members, keep):
    """`keep` of `members` one at a time: the largest remaining rank by strict >, scanning a upward.  Returns the mask."""
    out = 0
    for _ in range(keep):
        best, br = -1, 0.0
        for a in members:
            if out >> a & 1:
                continue
            if best < 0 or rank[a] > br:
                best, br = a, rank[a]
        if best >= 0:
            out |= 1 << best
    return out


def _score(x):
    x = float(np.float32(x))
    return -np.inf if x != x else x


class GumbelRestatement(NormPuctRestatement):
    """The normalised PUCT search with the Gumbel rule at the root, the candidate sets and the final move."""

    def __init__(self, *args, m, c_visit=C_VISIT, c_scale=C_SCALE, **kw):
        super().__init__(*args, **kw)
        self.m, self.c_visit, self.c_scale = m, float(c_visit), float(c_scale)
        self.cand = np.zeros(self.B, np.int64)
        self.scores = np.zeros((self.B, self.A), np.float32)
        self.offset = 0
        self.root_stops = 0                                          # paths that stopped at a root for want of budget

    # selection: NormPuctRestatement._select_tree with the root rule
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
                if depth == 0 and cs:                                # the candidate whose turn it is; the in-flight counts play no part
                    best, tried = cs[(self.offset + k) % len(cs)], -1
                else:
                    sq = self._tab(self.stab, int(self.visits[n]) + P.get(n, 0))
                    best, bu, tried, tu = -1, 0.0, -1, 0.0
                    for a in range(self.A):
                        ch = int(self.child[n, a])
                        if ch >= 0:
                            pc = P.get(ch, 0)
                            npc = int(self.visits[ch]) + pc
                            q = self._q(b, (float(self.W[ch]) - self.vl * float(pc)) / float(npc))
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
                    if tried < 0:                                    # no children, or a candidate's turn, and the budget spent
                        self.root_stops += depth == 0 and bool(cs)
                        break
                    best = tried
                n = int(self.child[n, best])
            if res is None:
                res = (leaf, scratch, 0, leaf, False, r, -1)
            for x in path:
                P[x] = P.get(x, 0) + 1
            out.append(res)
        return out

    # the candidate sets
    def begin(self, scores):
        self.scores = np.asarray(scores, np.float32).reshape(self.B, self.A).copy()
        for b in range(self.B):
            rank = [_score(x) for x in self.scores[b]]
            self.cand[b] = 0 if self.terminal[self.roots[b]] else _take(rank, range(self.A), min(self.m, self.A))

    def rank(self, b):
        root = int(self.roots[b])
        ch = [int(c) for c in self.child[root]]
        N = [max(int(self.visits[c]), 0) if c >= 0 else 0 for c in ch]
        max_n = max([n for n, c in zip(N, ch) if c >= 0], default=0)
        lo, hi = float(self.bounds[b, 0]), float(self.bounds[b, 1])
        out = []
        for a in range(self.A):
            visited = ch[a] >= 0 and N[a] > 0
            q = float(self.W[ch[a]]) / float(N[a]) if visited else self.fpv
            if visited and hi > lo:
                q = (q - lo) / (hi - lo)
            s1 = self.c_visit + float(max_n)
            s2 = s1 * self.c_scale
            x = _score(self.scores[b, a]) + s2 * q
            out.append(-np.inf if x != x else x)
        return out

    def members(self, b):
        return [a for a in range(self.A) if int(self.cand[b]) >> a & 1]

    def halve(self):
        for b in range(self.B):
            cs = self.members(b)
            self.cand[b] = _take(self.rank(b), cs, (len(cs) + 1) // 2)

    def pick_moves(self):
        out = np.zeros(self.B, np.int8)
        for b in range(self.B):
            cs = self.members(b)
            if cs:
                out[b] = _take(self.rank(b), cs, 1).bit_length() - 1
            else:
                ch = self.child[self.roots[b]]
                N = np.where(ch >= 0, np.maximum(self.visits[np.maximum(ch, 0)], 0), 0)
                out[b] = int(np.argmax(N)) if N.any() else 0
        return out

    def run(self, n):
        for halve, i in _phases(n, min(self.m, self.A)):
            if halve:
                self.halve()
            self.offset = i * self.K
            self.iteration()

    def advance(self, actions):
        out = super().advance(actions)
        self.cand[:] = 0
        return out

    def improved_policy(self):
        """[B, A] float32, in NumPy float64."""
        out = np.zeros((self.B, self.A), np.float32)
        for b in range(self.B):
            root = int(self.roots[b])
            ch = self.child[root]
            N = np.where(ch >= 0, self.visits[np.maximum(ch, 0)], 0).astype(np.float64)
            W = np.where(ch >= 0, self.W[np.maximum(ch, 0)], 0.0)
            visited = N > 0
            with np.errstate(divide="ignore"):
                x = np.log(self.prior[root].astype(np.float64))
            if visited.any():
                q = np.where(visited, W / np.where(visited, N, 1.0), W[visited].sum() / N[visited].sum())
                lo, hi = self.bounds[b]
                if hi > lo:
                    q = (q - lo) / (hi - lo)
                x = x + (self.c_visit + N.max()) * self.c_scale * q
            e = np.exp(x - x.max())
            out[b] = (e / e.sum()).astype(np.float32)
        return out


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _search(env, B, cap, K, m, budget, fn=None, **kw):
    from snac_amd import UCTSearch

    fn = scaled_evaluator(env.num_actions) if fn is None else fn
    s = UCTSearch(env, cap, 0, GAMMA, c=CPUCT, max_iterations=budget, trees=B, paths=K, virtual_loss=VL, evaluator=fn, q_normalise=True,
                  gumbel=m, **kw)
    s.reset()
    return s


def _pair(env, B, cap, K, m, budget, renv=None):
    fn = scaled_evaluator(env.num_actions)
    search = _search(env, B, cap, K, m, budget, fn)
    ref = GumbelRestatement(env if renv is None else renv, B, cap, K, VL, 0, GAMMA, CPUCT, fn, 0.0, budget, m=m)
    return search, ref


def _cand(search):
    import torch

    torch.cuda.synchronize()
    assert search.cand.dtype == torch.int32 and tuple(search.cand.shape) == (search.trees,)
    return search.cand.cpu().numpy().astype(np.int64)


def _lockstep(search, ref, n):
    """gumbel_run(n) with the restatement following launch by launch: after every HALVE the candidate sets, after every iteration every
    statistics word, tree size, record, select output, est and bounds byte are compared.  Returns the number of halvings."""
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


def _noisy_scores(search, seed):
    import torch

    g = torch.Generator(device=search.env.device)
    g.manual_seed(seed)
    return search.gumbel_scores(noise=True, generator=g)


# ---- a. zero candidates: the normalised PUCT search -----------------------------------------------------------------------------------------
def test_without_candidates_the_search_is_the_normalised_puct_search():
    """B = 70: two blocks of the lane-per-tree kernel.  cap = 9 spends the node budget of some trees."""
    import torch

    from snac_amd import UCTSearch

    B, cap, K = 70, 9, 2
    env = _env(2, True, B, 29)
    fn = scaled_evaluator(env.num_actions)
    gum = _search(env, B, cap, K, 4, 16, fn)
    ref = UCTSearch(env, cap, 0, GAMMA, c=CPUCT, max_iterations=16, trees=B, paths=K, virtual_loss=VL, evaluator=fn, q_normalise=True)
    ref.reset()
    assert gum.cand is not None and not _cand(gum).any() and ref.cand is None

    def same():
        torch.cuda.synchronize()
        assert torch.equal(gum.stats, ref.stats) and torch.equal(gum.tree_sizes(), ref.tree_sizes())
        assert torch.equal(gum.pool.records, ref.pool.records)
        oa, ob = _outputs(gum), _outputs(ref)
        for k in oa:
            assert oa[k].tobytes() == ob[k].tobytes(), k
        assert gum._est.cpu().numpy().tobytes() == ref._est.cpu().numpy().tobytes()
        assert gum.q_bounds.cpu().numpy().tobytes() == ref.q_bounds.cpu().numpy().tobytes()

    for _ in range(6):                                               # every launch
        gum.run(1)
        ref.run(1)
        same()
    assert (gum.tree_sizes() == cap).any()                           # the input: a spent budget somewhere
    picks = ref.best_actions()
    gum.advance(picks)
    ref.advance(picks)
    for _ in range(3):
        gum.run(1)
        ref.run(1)
        same()
    assert not _cand(gum).any()
    most = np.argmax(ref.root_visits().cpu().numpy(), axis=1)        # PICK without candidates: the most-visited action, ties lowest
    assert np.array_equal(gum.gumbel_actions().cpu().numpy(), most)


# ---- b. the restatement -------------------------------------------------------------------------------------------------------------------
CASES = [(kind, dyn, m) for kind, dyn, A in ((1, False, 3), (2, True, 5), (3, True, 8)) for m in sorted({2, 3, A})]


@pytest.mark.parametrize("cap", [24, 64])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("B", [5, 70])
@pytest.mark.parametrize("kind,dyn,m", CASES)
def test_gumbel_search_equals_the_restatement_bit_for_bit(kind, dyn, m, B, K, cap):
    """Two moves of n = 9 iterations each; rows 0::3 are one step before the time limit, so root children of theirs are terminal and,
    in 1D and 2D, their second roots are terminal (no candidates).  cap = 24 with K = 3: 27 simulations spend the node budget."""
    import torch

    n = 9
    env = _env(kind, dyn, B, 5 + kind + dyn)
    _near_the_end(kind, dyn)(env)
    A = env.num_actions
    search, ref = _pair(env, B, cap, K, m, 2 * n)
    ref.advanced = False
    _same(search, ref)                                               # the primed roots, empty bounds
    assert _empty(ref.bounds).all()
    halvings = 0
    for move in range(2):
        assert not _cand(search).any()
        scores = _noisy_scores(search, 100 + move)
        search.gumbel_begin(scores)
        ref.begin(scores.cpu().numpy())
        assert np.array_equal(_cand(search), ref.cand)
        live = ~ref.terminal[ref.roots]
        assert (np.array([bin(int(c)).count("1") for c in ref.cand]) == np.where(live, min(m, A), 0)).all()
        halvings += _lockstep(search, ref, n)
        got = search.gumbel_actions()
        assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), ref.pick_moves())
        assert np.array_equal(_cand(search), ref.cand)               # PICK leaves the candidates
        left = np.array([bin(int(c)).count("1") for c in ref.cand])
        assert (left[live] == min(m, 2)).all()                       # halved down to two (m >= 2)
        if move == 0:
            assert live.all()
            r, d = search.advance(got)
            er, ed = ref.advance(got.cpu().numpy())
            ref.advanced = True
            assert r.cpu().numpy().tobytes() == er.tobytes() and np.array_equal(d.cpu().numpy(), ed)
            assert not _cand(search).any()                           # a stale candidate set never steers a new root
            _same(search, ref, live_only=True, outputs=False)
            assert np.array_equal(ref.terminal[ref.roots], ed)
            if kind != 3:                                            # the second move's inputs: roots without candidates beside live ones
                assert ed[0::3].all() and not ed.all()               # (3D: a successful build does not test the time limit)
    assert halvings == 2 * sum(h for h, _ in _phases(n, min(m, A)))  # launched for every tree, with candidates or without
    assert search.iterations == 2 * n
    if cap == 24 and K == 3:
        print("trees with the budget spent: %d of %d" % (int((ref.used == cap).sum()), B))


@pytest.mark.parametrize("cap", [1, 2, 4])
def test_a_candidate_without_budget_stops_the_path_at_the_root(cap):
    """cap in {1, 2, 4} against A = 5 candidates and K = 3 paths: the turn of an untried candidate comes with the budget spent."""
    B, K, m, n = 5, 3, 5, 6
    env = _env(2, True, B, 31)
    search, ref = _pair(env, B, cap, K, m, n)
    ref.advanced = False
    scores = _noisy_scores(search, 7)
    search.gumbel_begin(scores)
    ref.begin(scores.cpu().numpy())
    _lockstep(search, ref, n)
    assert ref.root_stops > 0 and (ref.used == cap).all()
    o = _outputs(search)                                             # the last launch (every launch was compared with the restatement's)
    at_root = (o["leaf"] == np.repeat(np.arange(B) * cap, K)) & ~o["expanded"]
    assert (o["first_slot"][at_root] == -1).all() and (o["src"][at_root] == o["leaf"][at_root]).all()
    if cap <= 2:                                                     # at most one root child: one of the last two candidates is untried
        assert at_root.reshape(B, K).any(1).all()
    assert np.array_equal(search.gumbel_actions().cpu().numpy(), ref.pick_moves())


# ---- c. score edge cases on written statistics -------------------------------------------------------------------------------------------
def _written(m):
    """A search over B = 8 trees of A = 5 actions whose roots the test writes: (search, visits [B, A], W [B, A], child [B, A], bounds)."""
    import torch

    from snac_amd import _lib

    B, cap, A = 8, 16, 5
    env = _env(2, True, B, 3)
    env._hdr.view(torch.int8).view(B, 16)[7, 2] |= _lib.FLAG_NEED_RESET       # root 7 is terminal
    search = _search(env, B, cap, 1, m, 4)
    roots = np.arange(B) * cap
    child = np.full((B, A), -1, np.int32)
    visits = np.zeros((B, A), np.int32)
    W = np.zeros((B, A), np.float64)
    bounds = np.tile(np.array([np.inf, -np.inf]), (B, 1))
    # tree 0: nothing visited (every q is first_play_value).  tree 1: children 0 .. 3 visited, equal means.  tree 2: means that reorder
    # the scores, bounds on.  tree 3: a child row with 0 visits is not visited; maxN ignores a count without a child.  tree 4: bounds with
    # hi == lo (off).  trees 5, 6: as tree 2 with other scores.  tree 7: terminal.
    child[1, :4], visits[1, :4], W[1, :4] = roots[1] + 1 + np.arange(4), [2, 4, 6, 8], [1.0, 2.0, 3.0, 4.0]
    for b in (2, 5, 6):
        child[b], visits[b], W[b] = roots[b] + 1 + np.arange(A), [3, 1, 4, 1, 5], [30.0, -20.0, 10.0, 90.0, -50.0]
        bounds[b] = (-20.0, 90.0)
    child[3, :3], visits[3, :3], W[3, :3] = roots[3] + 1 + np.arange(3), [0, 7, 2], [5.0, 70.0, -6.0]
    visits[3, 4] = 1000                                              # no child: not counted
    bounds[3] = (-3.0, 10.0)
    child[4, :2], visits[4, :2], W[4, :2] = roots[4] + 1 + np.arange(2), [2, 2], [8.0, 6.0]
    bounds[4] = (3.5, 3.5)
    stats = search.stats.cpu().numpy()
    stats[roots, 0:A], stats[roots, 8:8 + A] = child, visits
    stats[roots, 16:16 + 2 * A] = W.view(np.int32).reshape(B, 2 * A)
    search.stats.copy_(torch.as_tensor(stats))
    search.q_bounds.copy_(torch.as_tensor(bounds))
    return search, visits, W, child, bounds


class _Written:
    """GumbelRestatement's candidate rules over the arrays of _written()."""
    begin, rank, members, halve, pick_moves = (GumbelRestatement.__dict__[k] for k in ("begin", "rank", "members", "halve", "pick_moves"))

    def __init__(self, m, visits, W, child, bounds, terminal):
        B, A = visits.shape
        self.B, self.A, self.m, self.fpv, self.c_visit, self.c_scale = B, A, m, 0.0, C_VISIT, C_SCALE
        self.roots = np.arange(B) * (A + 1)                          # row b * (A + 1) is root b, the next A rows its children
        rows = B * (A + 1)
        self.child = np.full((rows, A), -1, np.int64)
        self.visits, self.W, self.terminal = np.zeros(rows, np.int64), np.zeros(rows), np.zeros(rows, bool)
        for b in range(B):
            for a in range(A):
                if child[b, a] >= 0:
                    x = self.roots[b] + 1 + a
                    self.child[self.roots[b], a], self.visits[x], self.W[x] = x, visits[b, a], W[b, a]
        self.terminal[self.roots] = terminal
        self.bounds, self.cand = bounds, np.zeros(B, np.int64)


NINF, NAN = -np.inf, np.nan
SCORES = np.array([[1.0, 1.0, 1.0, 1.0, 1.0],                        # 0: ties everywhere: the lowest actions
                   [0.5, 0.5, 0.5, 0.5, 90.0],                       # 1: equal scores and equal means: ties in the rank
                   [0.0, 0.0, 0.0, 0.0, 0.0],                        # 2: the rank is sigma(q) alone
                   [NINF, 2.0, NAN, 1.0, 1.0],                       # 3: -inf and NaN lose to everything, and tie with each other
                   [3.0, 3.0, NINF, NINF, NINF],                     # 4: fewer finite scores than m
                   [40.0, 0.0, 40.0, 0.0, 80.0],                     # 5: scores that outweigh some of the q's
                   [NAN, NAN, NAN, NAN, NAN],                        # 6: all NaN: all -inf
                   [5.0, 4.0, 3.0, 2.0, 1.0]], np.float32)           # 7: the terminal root


@pytest.mark.parametrize("m", [3, 5, 8])
def test_candidates_on_written_statistics(m):
    """m = 8 > A = 5: every action begins; M = 5 keeps 3, then 2, then 1."""
    import torch

    search, visits, W, child, bounds = _written(m)
    B, A = visits.shape
    terminal = np.arange(B) == 7
    ref = _Written(m, visits, W, child, bounds, terminal)
    search.gumbel_begin(torch.as_tensor(SCORES))
    ref.begin(SCORES)
    got = _cand(search)
    assert np.array_equal(got, ref.cand), (got, ref.cand)
    want = {3: [0b00111, 0b10011, 0b00111, 0b11010, 0b00111, 0b10101, 0b00111, 0],
            5: [0b11111] * 7 + [0], 8: [0b11111] * 7 + [0]}[m]
    assert list(got) == want                                         # written out: ties to the lowest a, -inf / NaN last, terminal none
    sizes = [min(m, A)]
    while sizes[-1] > 1:
        sizes.append((sizes[-1] + 1) // 2)
    assert sizes == {3: [3, 2, 1], 5: [5, 3, 2, 1], 8: [5, 3, 2, 1]}[m]
    for size in sizes[1:]:
        before = got
        search._candidates(1)
        ref.halve()
        got = _cand(search)
        assert np.array_equal(got, ref.cand), (size, got, ref.cand)
        assert ([bin(int(c)).count("1") for c in got] == [size] * 7 + [0]) and ((got & ~before) == 0).all()
        if size == 3 and m >= 5:
            # tree 0: equal ranks keep 0, 1, 2.  tree 1: the score 90 wins, then equal ranks (equal scores, equal means, no bounds) keep 0, 1.
            # tree 2: sigma alone, q normalised over (-20, 90): means 10, -20, 2.5, 90, -10 keep 3, 0, 2.  tree 3: child 0 has no visits
            # (q = fpv = 0) and score -inf, child 1 (mean 10 -> q 1) wins, then actions 3 and 4 (score 1, unvisited) beat NaN and -inf.
            # tree 6: all -inf keep 0, 1, 2.
            assert [int(got[b]) for b in (0, 1, 2, 3, 6)] == [0b00111, 0b10011, 0b01101, 0b11010, 0b00111]
    action = search.gumbel_actions().cpu().numpy()
    assert np.array_equal(action, ref.pick_moves())
    assert np.array_equal(_cand(search), got)
    assert [1 << int(a) for a in action[:7]] == [int(c) for c in got[:7]] and action[7] == 0
    if m >= 5:
        assert list(action) == [0, 4, 3, 1, 0, 4, 0, 0]
    # PICK with several candidates left: the largest rank, ties lowest
    search.gumbel_begin(torch.as_tensor(SCORES))
    ref.begin(SCORES)
    assert np.array_equal(search.gumbel_actions().cpu().numpy(), ref.pick_moves())
    # without candidates: the most-visited action, the lowest of equals, 0 without visits (the count without a child included, as pick_moves)
    search.cand.zero_()
    assert list(search.gumbel_actions().cpu().numpy()) == [0, 3, 4, 4, 0, 4, 4, 0]
    assert np.array_equal(search.gumbel_actions().cpu().numpy(), search.pick_moves()[0].cpu().numpy())


# ---- d. properties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dyn,m,K,n", [(2, True, 4, 3, 9), (3, True, 8, 2, 12), (1, False, 3, 1, 7), (2, True, 1, 4, 3)])
def test_the_budget_goes_to_the_candidates(kind, dyn, m, K, n):
    import torch

    B, cap = 6, 256
    env = _env(kind, dyn, B, 41)
    A = env.num_actions
    search = _search(env, B, cap, K, m, n)
    assert not search.terminal[search._roots].any()
    scores = _noisy_scores(search, 3)
    forced = torch.arange(B, device=env.device) % A
    scores[torch.arange(B, device=env.device), forced] = 1.0e6       # far above every sigma(q) <= (50 + n * K) * 1
    search.gumbel_begin(scores)
    begin = _cand(search)
    search.gumbel_run(n)
    torch.cuda.synchronize()
    visits = search.root_visits().cpu().numpy()
    member = (begin[:, None] >> np.arange(A)[None, :] & 1) != 0
    assert (member.sum(1) == min(m, A)).all() and member[np.arange(B), forced.cpu().numpy()].all()
    assert (visits.sum(1) == n * K).all() and (search.visits[search._roots] == n * K).all()
    assert not visits[~member].any()
    phases = max(1, (min(m, A) - 1).bit_length())
    floor = (n // phases) * K // min(m, A)
    assert floor >= 1 and (visits[member] >= floor).all()
    assert torch.equal(search.gumbel_actions().long(), forced)
    assert search.iterations == n
    with pytest.raises(ValueError, match="max_iterations"):
        search.gumbel_run(phases)
    search.advance(search.gumbel_actions())
    with pytest.raises(ValueError, match="gumbel_begin"):
        search._gumbel_run(phases)


# ---- e. the improved policy ---------------------------------------------------------------------------------------------------------------
def test_improved_policy_against_numpy():
    import torch

    B, cap, K, m, n = 9, 64, 3, 4, 9
    env = _env(2, True, B, 43)
    _near_the_end(2, True)(env)
    search, ref = _pair(env, B, cap, K, m, 2 * n)
    p0 = search.improved_policy()
    assert p0.dtype == torch.float32 and tuple(p0.shape) == (B, env.num_actions)
    prior = ref.prior[ref.roots].astype(np.float64)
    assert np.abs(p0.cpu().numpy() - prior / prior.sum(1, keepdims=True)).max() <= PI_ATOL       # no visited child: the normalised priors
    assert np.abs(ref.improved_policy() - p0.cpu().numpy()).max() <= PI_ATOL
    for move in range(2):
        scores = _noisy_scores(search, 11 + move)
        search.gumbel_begin(scores)
        ref.begin(scores.cpu().numpy())
        search.gumbel_run(n)
        ref.run(n)
        _same(search, ref, live_only=move > 0)
        got, want = search.improved_policy().cpu().numpy(), ref.improved_policy()
        print("move %d: max |pi' - restatement| = %.3g" % (move, np.abs(got - want).max()))
        assert np.abs(got - want).max() <= PI_ATOL
        assert np.abs(got.astype(np.float64).sum(1) - 1.0).max() <= PI_ATOL
        live = ~ref.terminal[ref.roots]
        if move == 0:
            assert live.all()
            unvisited = search.root_visits().cpu().numpy() == 0
            assert unvisited.any() and (got[unvisited] > 0).all()    # an action the search never visited keeps a target above zero
            assert np.abs(got - prior / prior.sum(1, keepdims=True)).max() > 1.0e-3      # and the search moved the policy
            a = search.gumbel_actions()
            search.advance(a)
            ref.advance(a.cpu().numpy())
        else:
            assert not live.all() and live.any()                     # terminal roots: no visited child, the normalised priors


# ---- f. self-play -------------------------------------------------------------------------------------------------------------------------
def _play(seed_gen, sample_moves, moves=5, its=6, B=6, K=3, m=4, cap=48, capture=None):
    import torch

    from snac_amd import SelfPlay, _lib

    ts = _lib.env_sizes(2, True).total_step
    env = _env(2, True, B, 39)
    _near_the_end(2, True)(env)
    search = _search(env, B, cap, K, m, (ts + 1) * its)
    gen = None
    if seed_gen is not None:
        gen = torch.Generator(device=env.device)
        gen.manual_seed(seed_gen)
    if capture is not None:                                          # the scores each move began with
        begin = search.gumbel_begin

        def on_begin(scores):
            capture.append(scores.clone())
            begin(scores)

        search.gumbel_begin = on_begin
    play = SelfPlay(search, moves, sample_moves=sample_moves, gumbel=True, generator=gen)
    play.play(2, its)
    play.play(moves - 2, its)
    torch.cuda.synchronize()
    return play, search, env


def test_gumbel_self_play_equals_the_restatement_move_by_move():
    import torch

    from snac_amd import _lib

    B, cap, K, m, its, moves = 6, 48, 3, 4, 6, 5
    captured = []
    play, search, env = _play(None, 0, moves, its, B, K, m, cap, capture=captured)
    assert len(captured) == moves
    renv = _env(2, True, B, 39)                                      # play() resets env rows: the restatement follows on a twin
    _near_the_end(2, True)(renv)
    ts = _lib.env_sizes(2, True).total_step
    fn = scaled_evaluator(env.num_actions)
    ref = GumbelRestatement(renv, B, cap, K, VL, 0, GAMMA, CPUCT, fn, 0.0, (ts + 1) * its, m=m)
    A = env.num_actions
    want = dict(value=np.zeros((moves, B), np.float32), action=np.zeros((moves, B), np.int8), reward=np.zeros((moves, B), np.float32),
                done=np.zeros((moves, B), np.uint8), move=np.zeros((moves, B), np.int32))
    want_pi = np.zeros((moves, B, A), np.float32)
    obs = []
    in_episode, restarts = np.zeros(B, np.int64), np.zeros(B, np.int64)
    roots = torch.arange(B, device=env.device) * cap
    for mv in range(moves):
        scores = captured[mv].cpu().numpy()
        with np.errstate(divide="ignore"):                           # sample_moves = 0: the log-priors alone, float32
            assert np.allclose(scores, np.log(ref.prior[ref.roots]), rtol=1.0e-5, atol=1.0e-6)
        ref.begin(scores)
        ref.run(its)
        obs.append(ref.pool.observe(roots))
        a = ref.pick_moves()
        want_pi[mv] = ref.improved_policy()
        _, _, v = pick(ref, True, mv)
        r, d = ref.advance(a)
        want["value"][mv], want["action"][mv], want["reward"][mv], want["done"][mv], want["move"][mv] = v, a, r, d, in_episode
        renv.reset(mask=torch.as_tensor(d, device=env.device), want_obs=False)
        restart(ref, d)
        ref.rebound(d)
        restarts += d
        in_episode = np.where(d, 0, in_episode + 1)
    assert (restarts > 0).any() and (restarts == 0).any()            # the inputs: trees that restarted and trees that did not
    for s in range(moves):
        assert torch.equal(play.obs[s], obs[s]), s
    for k, w in want.items():
        assert getattr(play, k).cpu().numpy().tobytes() == w.tobytes(), k
    got_pi = play.pi.cpu().numpy()
    assert np.abs(got_pi - want_pi).max() <= PI_ATOL and np.abs(got_pi.astype(np.float64).sum(2) - 1.0).max() <= PI_ATOL
    _same(search, ref, live_only=True, outputs=False)
    assert not _cand(search).any() and torch.equal(env._hdr, renv._hdr)


def test_seeded_gumbel_self_play_repeats_itself():
    rings = []
    for _ in range(2):
        scores = []
        play, search, env = _play(5, 3, capture=scores)
        rings.append({k: getattr(play, k).cpu().numpy().tobytes() for k in ("obs", "pi", "value", "action", "reward", "done", "move")})
        rings[-1]["scores"] = b"".join(s.cpu().numpy().tobytes() for s in scores)
        rings[-1]["stats"] = search.stats.cpu().numpy().tobytes()
    for k in rings[0]:
        assert rings[0][k] == rings[1][k], k
    logits = np.log(search.root_priors().cpu().numpy())
    assert np.isfinite(logits).all()
    first = scores[0].cpu().numpy()                                  # move 0 of every tree is inside sample_moves: noisy scores
    assert (first != first[:, :1]).any(1).all() and len(np.unique(first)) > first.size // 2


def test_gumbel_self_play_does_not_synchronise_with_the_host():
    import torch

    from snac_amd import SelfPlay, _lib

    B, its = 64, 3
    ts = _lib.env_sizes(2, True).total_step
    env = _env(2, True, B, 3)
    _near_the_end(2, True)(env)
    search = _search(env, B, 64, 4, 4, (ts + 1) * its)
    gen = torch.Generator(device=env.device)
    gen.manual_seed(1)
    play = SelfPlay(search, 8, sample_moves=2, gumbel=True, generator=gen)
    play.play(1, its)                                                # warm-up: rows 0::3 end here
    play.targets()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        play.play(4, its)                                            # rows 1::3 end at the third move of their episode
        play.targets()
        search.gumbel_begin(search.gumbel_scores())                  # and the search's own calls
        search.gumbel_run(its)
        search.gumbel_actions()
        search.improved_policy()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    done = play.done.cpu().numpy()[:5]
    assert done[0, 0::3].all() and done[1:, 1::3].any() and not done[:, 2::3].all()
    assert play.moves == 5 and search.iterations == 6 * its


# ---- g. sharding --------------------------------------------------------------------------------------------------------------------------
def test_a_sharded_gumbel_search_is_the_whole_search():
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
                      evaluator=scaled_evaluator(A), q_normalise=True, gumbel=m)
        s.reset()
        out = []
        for mv in range(2):
            x = torch.as_tensor(scores[mv][off:off + s.trees], device=env.device)
            s.gumbel_begin(s.gumbel_scores(noise=False) + x)
            first = s.cand.clone()
            s.gumbel_run(n)
            a, pi = s.gumbel_actions(), s.improved_policy()
            out.append((first, s.cand.clone(), a, pi, s.q_bounds_of_trees()))
            if mv == 0:
                s.advance(a)
        torch.cuda.synchronize()
        return s, out

    whole, wout = make(whole_env, 0)
    assert len({int(c) for c in wout[0][0].cpu().numpy()}) > 1 and len(set(wout[0][2].cpu().numpy().tolist())) > 1
    for off, e in shards:
        s, out = make(e, off)
        cnt = s.trees
        for mv in range(2):
            for got, want in zip(out[mv], wout[mv]):
                assert got.cpu().numpy().tobytes() == want[off:off + cnt].cpu().numpy().tobytes(), (off, mv)
        sh._same_trees(s, whole, off, live_only=True)
