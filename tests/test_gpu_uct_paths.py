"""GPU: K paths per tree and iteration with virtual loss (UCTSearch(paths=K); snac_uct_select_paths / snac_uct_backup_paths, k_uct.hip)
against a restatement in python of the rules of include/snac_hip.h ("K paths per tree and iteration").

The rules, restated.  Slot s = b * K + k is path k of tree b; scratch rows are B * cap + s; pool and statistics have B * (cap + K) rows.
Selection, per tree, paths in order: u0 = used[b] on entry, a row >= b * cap + u0 is fresh; P(x) counts the earlier paths of the launch
through or ending at x.  A path walks from the root as the one-path search does, but stops on arriving at a fresh row (not expanded,
first_slot = the expander's slot, src = the root row), and compares
    Np = N_c + P_c;  q = (W_c - vl * P_c) / Np;  e = L[N(n) + P(n)] * R[Np];  u = q + c * e        (float64, ties to the lowest a);
with its leaf found, P += 1 on every node of the path.  first_slot is s for an expanded slot and -1 for a stored leaf.  The leaf's
first reward is reward[first_slot] where first_slot >= 0, else r_leaf; the edges draw counter word it * (H + 1), the leaves
it * (H + 1) + 1, both keyed by the slot of the unsharded search, (env_id_base + b) * K + k.  Backup, per tree: every expanded row is
written, then the walks run in slot order.
The restatement runs the same B * K-edge pool.transition and B * K-leaf pool.evaluate calls on a second pool of the same env.  Every
statistic (W as raw float64 bytes), every tree size, every node and scratch record and the last launch's select outputs must be equal."""
import contextlib
import math

import numpy as np
import pytest

from devmem import _env, _subtree
from test_gpu_uct import NON_DEFAULT, NON_DEFAULT_SEED

pytestmark = pytest.mark.gpu

KINDS = [(1, False), (1, True), (2, False), (2, True), (3, False), (3, True)]
H = {1: 300, 2: 600, 3: 200}
VL = 0.5                                                             # of the order of a step reward


class Restatement:
    """The multi-path search in python floats, tree by tree, on its own node pool."""

    def __init__(self, env, B, cap, K, vl, horizon, gamma, c, rows=None):
        import torch
        from snac_amd import NodePool

        self.env, self.B, self.cap, self.K, self.vl, self.H, self.gamma, self.c = env, B, cap, K, float(vl), horizon, gamma, c
        self.A = env.num_actions
        R = B * (cap + K)
        self.pool = NodePool(env, R)
        rows = torch.arange(B, device=env.device) if rows is None else torch.as_tensor(rows, device=env.device)
        roots = torch.arange(B, device=env.device) * cap
        self.pool.load(rows=rows, node_rows=roots)
        self.pool.load(rows=rows, node_rows=B * cap + torch.arange(B, device=env.device))
        self.child = np.full((R, self.A), -1, np.int64)
        self.parent = np.full(R, -1, np.int64)
        self.action = np.full(R, -1, np.int64)
        self.reward = np.zeros(R, np.float32)
        self.terminal = np.zeros(R, bool)
        self.terminal[roots.cpu().numpy()] = self.pool.need_reset[roots].cpu().numpy()
        self.visits = np.zeros(R, np.int64)
        self.W = np.zeros(R, np.float64)
        self.used = np.ones(B, np.int64)
        self.leaf_count = np.zeros(R, np.int64)
        self.it = 0
        self.last = None                                             # the last launch's select outputs
        self.fresh_hits = []                                         # per iteration: slots that stopped on a fresh row

    @contextlib.contextmanager
    def slot_keys(self):
        """The pool calls key edge / leaf s of a call by env_id_base + s; an iteration's words are keyed by (env_id_base + b) * K + k, the
        slot in the unsharded search, which is (env_id_base * K) + s: the calls inside run on the descriptor with that base."""
        desc = self.env._desc
        desc.env_id_base = self.env.env_id_base * self.K
        try:
            yield
        finally:
            desc.env_id_base = self.env.env_id_base

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
                    q = (float(self.W[ch]) - self.vl * float(pc)) / float(npc)
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
        assert not np.isin(src, dst).any()                           # no edge's source is an edge's destination
        t = self.it * (self.H + 1)
        with self.slot_keys():
            _, rew, done = self.pool.transition(torch.as_tensor(act.astype(np.int8)), src=src, dst=dst, t=t, want_obs=False)
            rew, done = rew.cpu().numpy(), done.cpu().numpy()
            first_r = np.where(first >= 0, rew[np.maximum(first, 0)], rleaf.astype(np.float32)).astype(np.float64)
            est, _ = self.pool.evaluate(torch.as_tensor(leaf), self.H, self.gamma, first_reward=torch.as_tensor(first_r), t0=t + 1)
        est = est.cpu().numpy()
        for s in np.nonzero(exp)[0]:                                 # first every expanded row, whole
            x = int(leaf[s])
            self.parent[x], self.action[x], self.reward[x], self.terminal[x] = src[s], act[s], rew[s], done[s]
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
        self.it += 1

    # ---- advance(), restated from "Re-rooting after a move" ----------------------------------------------------------------
    def advance(self, actions):
        import torch

        B, cap, dev = self.B, self.cap, self.env.device
        actions = np.asarray(actions, np.int64)
        roots = np.arange(B) * cap
        untried = np.array([not self.terminal[roots[b]] and self.child[roots[b], actions[b]] < 0 for b in range(B)])
        dst = np.where(untried, roots, B * cap + np.arange(B))
        _, rew, done = self.pool.transition(torch.as_tensor(actions.astype(np.int8)), src=roots, dst=dst, t=self.it * (self.H + 1),
                                            want_obs=False)
        rew, done = rew.cpu().numpy(), done.cpu().numpy()
        out_r, out_d = np.zeros(B, np.float32), np.zeros(B, bool)
        arrays = (self.action, self.reward, self.terminal, self.visits, self.W, self.leaf_count)
        for b in range(B):
            base, used = roots[b], int(self.used[b])
            if self.terminal[base]:
                out_r[b], out_d[b] = 0.0, True
                continue
            c = int(self.child[base, actions[b]])
            if c < 0:
                self._clear(base, base + cap)
                self.terminal[base] = done[b]
                self.used[b] = 1
                out_r[b], out_d[b] = rew[b], done[b]
                continue
            out_r[b], out_d[b] = self.reward[c], self.terminal[c]
            old = [c]
            for i in range(c + 1, base + used):                      # rows whose parent chain reaches c, in increasing order
                x = i
                while x > c:
                    x = int(self.parent[x])
                if x == c:
                    old.append(i)
            old = np.array(old)
            n = len(old)
            new = base + np.arange(n)
            o2n = {int(o): base + j for j, o in enumerate(old)}
            ch = np.array([[o2n[int(x)] if x >= 0 else -1 for x in r] for r in self.child[old]], np.int64).reshape(n, self.A)
            par = np.array([o2n.get(int(p), -1) for p in self.parent[old]], np.int64)
            fields = [a[old].copy() for a in arrays]
            self.pool.records[torch.as_tensor(new, device=dev)] = self.pool.records[torch.as_tensor(old, device=dev)].clone()
            self._clear(base, base + cap)
            self.child[new], self.parent[new] = ch, par
            for a, f in zip(arrays, fields):
                a[new] = f
            self.parent[base], self.action[base], self.reward[base] = -1, -1, 0.0
            self.used[b] = n
        return out_r, out_d

    def _clear(self, lo, hi):
        self.child[lo:hi], self.parent[lo:hi], self.action[lo:hi] = -1, -1, -1
        self.reward[lo:hi], self.terminal[lo:hi], self.visits[lo:hi], self.W[lo:hi], self.leaf_count[lo:hi] = 0, False, 0, 0.0, 0


def _outputs(search):
    """The last launch's select outputs of the device search."""
    return dict(src=search._src.cpu().numpy(), dst=search._dst.cpu().numpy(), action=search._action.cpu().numpy(),
                leaf=search._leaf.cpu().numpy(), expanded=search._expanded.cpu().numpy() != 0, r_leaf=search._r_leaf.cpu().numpy(),
                first_slot=search._first_slot.cpu().numpy())


def _same_outputs(search, ref):
    got = _outputs(search)
    for k, want in ref.last.items():
        if k == "r_leaf":
            assert got[k].tobytes() == want.tobytes(), k
        else:
            assert np.array_equal(got[k], want), k


def _same(search, ref, live_only=False):
    """Every statistics word, tree size and record; live_only: rows [base, base + used) only (after advance() the rest is unspecified)."""
    import torch

    torch.cuda.synchronize()
    A, B, cap = ref.A, ref.B, ref.cap
    used = search.tree_sizes().cpu().numpy()
    assert np.array_equal(used, ref.used)
    rows = np.concatenate([b * cap + np.arange(int(used[b])) for b in range(B)]) if live_only else np.arange(B * (cap + ref.K))
    assert np.array_equal(search.children.cpu().numpy()[rows], ref.child[rows])
    assert np.array_equal(search.parent.cpu().numpy()[rows], ref.parent[rows])
    assert np.array_equal(search.action.cpu().numpy()[rows], ref.action[rows])
    assert search.reward.cpu().numpy()[rows].tobytes() == ref.reward[rows].tobytes()
    assert np.array_equal(search.terminal.cpu().numpy()[rows], ref.terminal[rows])
    assert np.array_equal(search.visits.cpu().numpy()[rows], ref.visits[rows])
    assert search.value_sum.cpu().numpy()[rows].tobytes() == ref.W[rows].tobytes()
    ri = torch.as_tensor(rows, device=search.env.device)
    assert torch.equal(search.pool.records[ri], ref.pool.records[ri])
    mirror_n = search.stats[:, 8:8 + A].cpu().numpy()[rows]
    mirror_w = search.stats[:, 16:32].contiguous().view(torch.float64)[:, :A].cpu().numpy()[rows]
    ch = ref.child[rows]
    has = ch >= 0
    assert np.array_equal(mirror_n[has], ref.visits[ch[has]])
    assert mirror_w[has].tobytes() == ref.W[ch[has]].tobytes()
    assert not mirror_n[~has].any()
    assert not search.stats[ri, 39:].any()                          # the in-flight words are zero outside an iteration


def _invariants(search, ref, iterations, since_reset=True):
    """root visits == iterations * K; visits == the children's visits + the times the node was the leaf; words 39.. zero; child[] and
    parent / action agree; every index inside its tree."""
    B, cap, A, K = search.trees, search.nodes_per_tree, search.num_actions, search.paths
    ch = search.children.cpu().numpy()
    par, act = search.parent.cpu().numpy(), search.action.cpu().numpy()
    vis = search.visits.cpu().numpy()
    sizes = search.tree_sizes().cpu().numpy()
    roots = np.arange(B) * cap
    if since_reset:
        assert (vis[roots] == iterations * K).all()
        assert (search.root_visits().cpu().numpy().sum(1) <= iterations * K).all()
    live = np.concatenate([b * cap + np.arange(int(sizes[b])) for b in range(B)])
    kids = np.where(ch >= 0, vis[np.maximum(ch, 0)], 0).sum(1)
    assert np.array_equal(vis[live], (kids + ref.leaf_count)[live])
    assert not search.stats[live, 39:].any()
    tree = np.arange(B * (cap + K)) // cap
    for x in live:
        for a in range(A):
            c = ch[x, a]
            if c >= 0:
                assert tree[c] == tree[x] and c % cap != 0 and par[c] == x and act[c] == a
        if x % cap == 0:
            assert par[x] == -1 and act[x] == -1
        else:
            assert tree[par[x]] == tree[x] and ch[par[x], act[x]] == x
    if since_reset:
        assert (ch[B * cap:] == -1).all() and (vis[B * cap:] == 0).all()


def _pair(env, B, cap, K, vl, horizon, iterations, rows=None, gamma=0.97, c=math.sqrt(2), chunks=(None,)):
    from snac_amd import UCTSearch

    search = UCTSearch(env, cap, horizon, gamma, c=c, max_iterations=iterations, trees=B, paths=K, virtual_loss=vl)
    search.reset(rows=rows)
    ref = Restatement(env, B, cap, K, vl, horizon, gamma, c, rows)
    done = 0
    for k in chunks:
        k = iterations - done if k is None else k
        search.run(k)
        for _ in range(k):
            ref.iteration()
        done += k
        _same(search, ref)
        _same_outputs(search, ref)
        _invariants(search, ref, done)
    return search, ref


@pytest.mark.parametrize("vl", [0.0, VL])
@pytest.mark.parametrize("K,its", [(2, 40), (5, 18), (16, 7)])
@pytest.mark.parametrize("kind,dyn", KINDS)
def test_multi_path_search_equals_the_restatement_bit_for_bit(kind, dyn, K, its, vl):
    import torch

    B, cap = 24, 48
    env = _env(kind, dyn, B, 5 + kind + dyn)
    rows = torch.arange(B, device=env.device) // 2
    search, ref = _pair(env, B, cap, K, vl, H[kind] // 2, its, rows, chunks=(its // 3, None))
    assert (search.tree_sizes().cpu().numpy() > 1).all()
    assert np.array_equal(search.best_actions().cpu().numpy(), np.argmax(search.root_visits().cpu().numpy(), axis=1))


@pytest.mark.parametrize("kind,dyn", [(2, True), (3, False), (1, True)])
def test_one_path_is_the_default_search(kind, dyn):
    """paths=1 runs the one-path entry points: statistics, records and tree sizes equal a default UCTSearch's bit for bit."""
    import torch

    from snac_amd import UCTSearch

    B, cap, n = 48, 40, 60
    env = _env(kind, dyn, B, 11 + kind)
    a = UCTSearch(env, cap, H[kind] // 2, 0.97, max_iterations=n, trees=B)
    b = UCTSearch(env, cap, H[kind] // 2, 0.97, max_iterations=n, trees=B, paths=1, virtual_loss=VL)
    assert b.rows == a.rows == B * (cap + 1)
    for s in (a, b):
        s.reset()
        s.run(n)
    torch.cuda.synchronize()
    assert torch.equal(a.stats, b.stats) and torch.equal(a.pool.records, b.pool.records)
    assert torch.equal(a.tree_sizes(), b.tree_sizes())
    assert (a.visits[a._roots] == n).all()


@pytest.mark.parametrize("kind,dyn,K", [(1, False, 7), (2, True, 16), (3, True, 12)])
def test_paths_stop_on_fresh_rows_and_step_the_root(kind, dyn, K):
    """K > A and cap > A: the first iteration of every tree expands A children and sends K - A paths onto fresh rows."""
    B, cap, its = 16, 40, 6
    env = _env(kind, dyn, B, 17 + kind)
    A = env.num_actions
    assert K > A and cap > A
    from snac_amd import UCTSearch

    search = UCTSearch(env, cap, H[kind] // 4, 0.97, max_iterations=its, trees=B, paths=K, virtual_loss=VL)
    search.reset()
    ref = Restatement(env, B, cap, K, VL, H[kind] // 4, 0.97, math.sqrt(2))
    roots = np.repeat(np.arange(B) * cap, K)
    for it in range(its):
        search.run(1)
        ref.iteration()
        _same(search, ref)
        _same_outputs(search, ref)
        o = _outputs(search)
        assert not np.isin(o["src"], o["dst"]).any()                 # no edge's src is any edge's dst
        assert len(np.unique(o["dst"])) == B * K
        on_fresh = (~o["expanded"]) & (o["first_slot"] >= 0) & (o["src"] == roots)
        assert np.array_equal(on_fresh, (~o["expanded"]) & (o["first_slot"] >= 0))      # a fresh leaf always steps the root
        if it == 0:
            per_tree = on_fresh.reshape(B, K).sum(1)
            assert (per_tree >= K - A).all(), per_tree
            assert (o["expanded"].reshape(B, K).sum(1) == A).all()
        hit = np.nonzero(on_fresh)[0]
        exp = o["first_slot"][hit]
        assert (exp // K == hit // K).all() and (exp < hit).all() and o["expanded"][exp].all()
        assert np.array_equal(o["leaf"][hit], o["dst"][exp])         # the fresh leaf is its expander's new row
        stored = (~o["expanded"]) & (o["first_slot"] < 0)
        assert np.array_equal(o["src"][stored], o["leaf"][stored])
        own = np.nonzero(o["expanded"])[0]
        assert np.array_equal(o["first_slot"][own], own)
    _invariants(search, ref, its)


@pytest.mark.parametrize("kind,dyn,cap", [(2, True, 1), (2, True, 2), (1, False, 4), (3, True, 9)])
def test_budget_exhaustion_with_several_paths(kind, dyn, cap):
    """cap in {1, 2, A + 1}: the paths pile up on the same few leaves and take scratch edges."""
    B, K = 16, 5
    env = _env(kind, dyn, B, 21 + cap)
    assert cap in (1, 2, env.num_actions + 1)
    search, ref = _pair(env, B, cap, K, VL, H[kind] // 4, 12, chunks=(1, 4, None))
    assert (search.tree_sizes().cpu().numpy() == cap).all()
    assert ref.leaf_count[:B * cap].max() > 1
    if cap == 2:
        assert ref.fresh_hits[0].reshape(B, K).sum(1).tolist() == [K - 1] * B


@pytest.mark.parametrize("kind,dyn", KINDS)
def test_terminal_roots_and_terminal_fresh_nodes(kind, dyn):
    import torch

    from snac_amd import _lib

    B, cap, K, its = 24, 32, 10, 6                                   # K > A: the first iteration sends paths onto fresh rows
    env = _env(kind, dyn, B, 31 + kind)
    ts = _lib.env_sizes(kind, dyn).total_step
    cs = env._hdr.view(torch.int16).view(B, 8)[:, 3]
    cs[0::3] = ts - 1                                                # children come back done: fresh rows that are terminal
    cs[1::3] = ts - 2                                                # grandchildren
    env._hdr.view(torch.int8).view(B, 16)[2::9, 2] |= _lib.FLAG_NEED_RESET   # terminal roots
    search, ref = _pair(env, B, cap, K, VL, H[kind] // 4, its, chunks=(1, 3, None))
    assert ref.fresh_hits[0].reshape(B, K)[0::3].any()               # paths stopped on fresh rows that came back done
    term = search.terminal.cpu().numpy()
    ch = search.children.cpu().numpy()
    vis, W, r = search.visits.cpu().numpy(), search.value_sum.cpu().numpy(), search.reward.cpu().numpy()
    roots = np.arange(B) * cap
    nonroot = np.arange(len(term)) % cap != 0
    nonroot[B * cap:] = False
    assert term[roots[2::9]].all() and term[nonroot].any()
    assert (ch[term] == -1).all()                                    # terminal nodes are never expanded
    for x in np.nonzero(term)[0]:
        w = 0.0
        for _ in range(int(vis[x])):
            w += float(r[x])                                          # every visit adds exactly the stored reward (0 at a root)
        assert W[x].tobytes() == np.float64(w).tobytes()
    assert (search.tree_sizes().cpu().numpy()[2::9] == 1).all() and (vis[roots[2::9]] == its * K).all()


@pytest.mark.parametrize("kind,dyn,K", [(2, True, 5), (3, False, 16), (1, True, 4)])
def test_advance_after_a_multi_path_run(kind, dyn, K):
    """The kept subtree is the old one node for node; further multi-path iterations on it still match the restatement."""
    import torch

    from snac_amd import UCTSearch

    B, cap, n = 16, 64, 8
    env = _env(kind, dyn, B, 71 + kind)
    hz = H[kind] // 4
    search = UCTSearch(env, cap, hz, 0.97, max_iterations=3 * n, trees=B, paths=K, virtual_loss=VL)
    search.reset()
    ref = Restatement(env, B, cap, K, VL, hz, 0.97, math.sqrt(2))
    search.run(n)
    for _ in range(n):
        ref.iteration()
    _same(search, ref)
    a = search.best_actions().cpu().numpy()
    before, rec_before = search.stats.clone().cpu().numpy(), search.pool.records.clone()
    r, d = search.advance(torch.as_tensor(a, device=env.device))
    er, ed = ref.advance(a)
    _same(search, ref, live_only=True)
    assert r.cpu().numpy().tobytes() == er.tobytes() and np.array_equal(d.cpu().numpy(), ed)
    after, rec_after = search.stats.cpu().numpy(), search.pool.records
    A = search.num_actions
    sizes = search.tree_sizes().cpu().numpy()
    for b in range(B):
        base = b * cap
        c = int(before[base, a[b]])
        assert c > base
        old = _subtree(before[:, :A], c, [])
        new = _subtree(after[:, :A], base, [])
        assert len(old) == len(new) == sizes[b]
        assert sorted(new) == list(range(base, base + sizes[b]))
        assert before[c, 35] == after[base, 35] and before[c, 36:38].tobytes() == after[base, 36:38].tobytes()
        assert np.array_equal(before[old][:, 8:32], after[new][:, 8:32])           # mirrors: child visits and values
        assert np.array_equal(before[old][:, 34:38], after[new][:, 34:38])         # terminal, visits, W
        assert np.array_equal(before[old[1:]][:, 33], after[new[1:]][:, 33])        # actions below the root
        assert np.array_equal(before[old[1:]][:, 38], after[new[1:]][:, 38])        # rewards below the root
        assert not after[new][:, 39:].any()
        assert after[base, 32] == -1 and after[base, 33] == -1 and after[base, 38] == 0
        oi, ni = torch.as_tensor(old, device=env.device), torch.as_tensor(new, device=env.device)
        assert torch.equal(rec_before[oi], rec_after[ni])
    for chunk in (3, n - 3):                                         # fresh rows now lie in rows advance() left unspecified
        search.run(chunk)
        for _ in range(chunk):
            ref.iteration()
        _same(search, ref, live_only=True)
        _same_outputs(search, ref)
        _invariants(search, ref, None, since_reset=False)
    search.store_roots()
    assert search.iterations == 2 * n


def test_multi_path_run_does_not_synchronise_with_the_host():
    import torch

    from snac_amd import UCTSearch

    env = _env(2, True, 64, 3)
    search = UCTSearch(env, 64, 100, 0.97, max_iterations=32, paths=8, virtual_loss=VL)
    search.reset()
    search.run(2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        search.run(10)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert (search.visits[search._roots] == 12 * 8).all()
    with pytest.raises(ValueError):
        search.run(21)                                               # 12 + 21 > max_iterations


@pytest.mark.parametrize("kind,dyn", [(2, True), (3, False)])
def test_a_captured_multi_path_run_replays_as_the_search(kind, dyn):
    """A graph of run(n) (one stream, no parallel branches) replayed after reset() leaves what run(n) leaves."""
    import torch

    from snac_amd import UCTSearch

    B, n, K = 32, 12, 6
    env = _env(kind, dyn, B, 41 + kind)
    search = UCTSearch(env, 48, H[kind] // 4, 0.95, max_iterations=n, paths=K, virtual_loss=VL)
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


@pytest.mark.parametrize("kind,dyn,probs", [(3, True, [4, 1, 1, 1, 1, 0, 2, 3]), (2, False, [1, 3, 0, 2, 2])])
def test_multi_path_search_follows_the_action_distribution(kind, dyn, probs):
    B = 16
    env = _env(kind, dyn, B, 51 + kind, action_probs=probs)
    _pair(env, B, 32, 4, VL, H[kind] // 4, 12)


@pytest.mark.parametrize("kind,dyn,K", [(2, True, 4)])
def test_multi_path_search_on_a_non_default_env_equals_the_restatement_bit_for_bit(kind, dyn, K):
    """env_id_base 1000, a 64-bit seed, brick_gt / time_gt, total_step 9 and an action distribution: the slots' keys start at 1000 * K."""
    B = 16
    env = _env(kind, dyn, B, NON_DEFAULT_SEED, **NON_DEFAULT)
    assert env.env_id_base == 1000 and env.seed >> 32 == 9 and env.total_step == 9 and env.brick_gt and env.time_gt
    search, ref = _pair(env, B, 32, K, VL, H[kind] // 4, 12, chunks=(5, None))
    assert (search.tree_sizes().cpu().numpy() > 1).all()
    assert env._desc.env_id_base == 1000                             # the restatement left the descriptor as it was
