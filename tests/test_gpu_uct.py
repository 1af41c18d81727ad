"""GPU: batched UCT search on node pools (UCTSearch; snac_uct_select / snac_uct_backup, k_uct.hip) against a restatement of the rules
of include/snac_hip.h ("UCT tree search") in python: selection and backup per tree on the host, the same B-edge pool.transition and
B-leaf pool.evaluate calls on a second pool of the same env.  Every statistic (W as raw float64 bytes), every tree size and every node
and scratch record must be equal."""
import math

import numpy as np
import pytest

from devmem import _env, _raw

pytestmark = pytest.mark.gpu

KINDS = [(1, False), (1, True), (2, False), (2, True), (3, False), (3, True)]
H = {1: 300, 2: 600, 3: 200}
# a 2D env away from every default: a shard's base, a seed with a high word, the strict termination rules, a short time limit and the 2D
# action mix of test_search_follows_the_action_distribution (the restatements read env.seed and env.env_id_base)
NON_DEFAULT_SEED = (9 << 32) | 3
NON_DEFAULT = dict(env_id_base=1000, brick_gt=True, time_gt=True, total_step=9, action_probs=[1, 3, 0, 2, 2])


class Restatement:
    """The search of include/snac_hip.h in python floats, tree by tree, on its own node pool."""

    def __init__(self, env, B, cap, horizon, gamma, c, rows):
        import torch
        from snac_amd import NodePool

        self.env, self.B, self.cap, self.H, self.gamma, self.c = env, B, cap, horizon, gamma, c
        self.A = env.num_actions
        R = B * (cap + 1)
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

    def _select(self, b):
        base, cap = b * self.cap, self.cap
        n = leaf = base
        for _ in range(cap):
            leaf, r = n, self.reward[n]
            if self.terminal[n]:
                break
            untried = [a for a in range(self.A) if self.child[n, a] < 0]
            if untried and self.used[b] < cap:
                new = base + self.used[b]
                self.used[b] += 1
                self.child[n, untried[0]] = new
                return n, new, untried[0], new, True, np.float32(0)
            best, bu = -1, 0.0
            for a in range(self.A):
                ch = int(self.child[n, a])
                if ch < 0:
                    continue
                nc = int(self.visits[ch])
                u = float(self.W[ch]) / nc + self.c * (math.sqrt(math.log(int(self.visits[n]))) * (1.0 / math.sqrt(nc)))
                if best < 0 or u > bu:
                    best, bu = a, u
            if best < 0:
                break
            n = int(self.child[n, best])
        return leaf, self.B * cap + b, 0, leaf, False, r

    def iteration(self):
        import torch

        sel = [self._select(b) for b in range(self.B)]
        src, dst, act, leaf, exp, rleaf = (np.array(x) for x in zip(*sel))
        t = self.it * (self.H + 1)
        _, rew, done = self.pool.transition(torch.as_tensor(act.astype(np.int8)), src=src, dst=dst, t=t, want_obs=False)
        rew, done = rew.cpu().numpy(), done.cpu().numpy()
        first = np.where(exp, rew, rleaf.astype(np.float32)).astype(np.float64)
        est, _ = self.pool.evaluate(torch.as_tensor(leaf), self.H, self.gamma, first_reward=torch.as_tensor(first), t0=t + 1)
        est = est.cpu().numpy()
        for b in range(self.B):
            x = int(leaf[b])
            self.leaf_count[x] += 1
            if exp[b]:
                self.parent[x], self.action[x], self.reward[x], self.terminal[x] = src[b], act[b], rew[b], done[b]
            g = float(est[b])
            for _ in range(self.cap):
                self.visits[x] += 1
                self.W[x] = float(self.W[x]) + g
                p = int(self.parent[x])
                if p < 0:
                    break
                g = float(self.reward[p]) + self.gamma * g
                x = p
        self.it += 1


def _same(search, ref):
    import torch

    torch.cuda.synchronize()
    A = ref.A
    assert np.array_equal(search.children.cpu().numpy(), ref.child)
    assert np.array_equal(search.parent.cpu().numpy(), ref.parent)
    assert np.array_equal(search.action.cpu().numpy(), ref.action)
    assert _raw(search.reward) == ref.reward.tobytes()
    assert np.array_equal(search.terminal.cpu().numpy(), ref.terminal)
    assert np.array_equal(search.visits.cpu().numpy(), ref.visits)
    assert _raw(search.value_sum) == ref.W.tobytes()
    assert np.array_equal(search.tree_sizes().cpu().numpy(), ref.used)
    assert torch.equal(search.pool.records, ref.pool.records)
    # the children's statistics mirrored in the parent's record
    mirror_n = search.stats[:, 8:8 + A].cpu().numpy()
    mirror_w = search.stats[:, 16:32].contiguous().view(torch.float64)[:, :A].cpu().numpy()
    has = ref.child >= 0
    assert np.array_equal(mirror_n[has], ref.visits[ref.child[has]])
    assert mirror_w[has].tobytes() == ref.W[ref.child[has]].tobytes()
    assert not mirror_n[~has].any()


def _invariants(search, ref, iterations):
    """root visits == iterations; visits == the children's visits + the times the node was the leaf; child[] and parent / action
    agree; every index inside its tree."""
    B, cap, A = search.trees, search.nodes_per_tree, search.num_actions
    ch = search.children.cpu().numpy()
    par, act = search.parent.cpu().numpy(), search.action.cpu().numpy()
    vis = search.visits.cpu().numpy()
    roots = np.arange(B) * cap
    assert (vis[roots] == iterations).all()
    assert (search.root_visits().cpu().numpy().sum(1) <= iterations).all()
    kids = np.where(ch >= 0, vis[np.maximum(ch, 0)], 0).sum(1)
    assert np.array_equal(vis, kids + ref.leaf_count)
    tree = np.arange(B * (cap + 1)) // cap
    sizes = search.tree_sizes().cpu().numpy()
    for x in range(B * cap):
        for a in range(A):
            c = ch[x, a]
            if c >= 0:
                assert tree[c] == tree[x] and c % cap != 0 and par[c] == x and act[c] == a
        if x % cap == 0:
            assert par[x] == -1 and act[x] == -1
        elif x % cap < sizes[x // cap]:
            assert tree[par[x]] == tree[x] and ch[par[x], act[x]] == x
    assert (ch[B * cap:] == -1).all() and (vis[B * cap:] == 0).all()


def _pair(env, B, cap, horizon, iterations, rows, gamma=0.97, c=math.sqrt(2), chunks=(None,)):
    from snac_amd import UCTSearch

    search = UCTSearch(env, cap, horizon, gamma, c=c, max_iterations=iterations, trees=B)
    search.reset(rows=rows)
    ref = Restatement(env, B, cap, horizon, gamma, c, rows)
    done = 0
    for k in chunks:
        k = iterations - done if k is None else k
        search.run(k)
        for _ in range(k):
            ref.iteration()
        done += k
        _same(search, ref)
        _invariants(search, ref, done)
    return search, ref


@pytest.mark.parametrize("kind,dyn", KINDS)
def test_search_equals_the_restatement_bit_for_bit(kind, dyn):
    import torch

    B = 64 if kind == 3 else 96
    env = _env(kind, dyn, B, 5 + kind + dyn)
    rows = torch.arange(B, device=env.device) // 2                  # pairs of trees over one state: root parallelism
    search, ref = _pair(env, B, 64, H[kind], 100, rows, chunks=(37, None))
    sizes = search.tree_sizes().cpu().numpy()
    assert sizes.max() == 64 and sizes.min() > 1                     # budgets spent, revisits taken
    rv = search.root_visits().view(B // 2, 2, -1)
    assert bool((rv[:, 0] != rv[:, 1]).any())                        # copies of one state draw different words
    q = search.root_q()
    assert bool(torch.isnan(q[search.stats[search._roots][:, :env.num_actions] < 0]).all())
    best = search.best_actions()
    assert best.dtype == torch.int64
    assert np.array_equal(best.cpu().numpy(), np.argmax(search.root_visits().cpu().numpy(), axis=1))   # the first maximum


@pytest.mark.parametrize("kind,dyn,cap", [(2, True, 2), (1, False, 3), (3, True, 4)])
def test_budget_exhaustion_revisits_leaves_and_takes_scratch_edges(kind, dyn, cap):
    B = 64
    env = _env(kind, dyn, B, 21 + cap)
    search, ref = _pair(env, B, cap, H[kind] // 4, 80, None, chunks=(1, 9, None))
    assert (search.tree_sizes().cpu().numpy() == cap).all()
    assert ref.leaf_count[:B * cap].max() > 1


@pytest.mark.parametrize("kind,dyn", KINDS)
def test_terminal_nodes_are_never_expanded(kind, dyn):
    import torch

    from snac_amd import _lib

    B, cap, its = 64, 32, 60
    env = _env(kind, dyn, B, 31 + kind)
    ts = _lib.env_sizes(kind, dyn).total_step
    cs = env._hdr.view(torch.int16).view(B, 8)[:, 3]
    cs[0::3] = ts - 1                                                # children come back done
    cs[1::3] = ts - 2                                                # grandchildren
    env._hdr.view(torch.int8).view(B, 16)[2::9, 2] |= _lib.FLAG_NEED_RESET   # terminal roots
    search, ref = _pair(env, B, cap, H[kind] // 4, its, None, chunks=(7, None))
    term = search.terminal.cpu().numpy()
    ch = search.children.cpu().numpy()
    vis, W, r = search.visits.cpu().numpy(), search.value_sum.cpu().numpy(), search.reward.cpu().numpy()
    roots = np.arange(B) * cap
    nonroot = np.arange(len(term)) % cap != 0
    nonroot[B * cap:] = False
    assert term[roots[2::9]].all() and term[nonroot].any()
    assert (ch[term] == -1).all()
    for x in np.nonzero(term)[0]:
        w = 0.0
        for _ in range(int(vis[x])):
            w += float(r[x])                                          # every visit adds exactly the stored reward (0 at a root)
        assert W[x].tobytes() == np.float64(w).tobytes()
    assert (search.tree_sizes().cpu().numpy()[2::9] == 1).all() and (vis[roots[2::9]] == its).all()


def test_run_does_not_synchronise_with_the_host():
    import torch

    from snac_amd import UCTSearch

    env = _env(2, True, 256, 3)
    search = UCTSearch(env, 32, 100, 0.97, max_iterations=64)
    search.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        search.run(20)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert (search.visits[search._roots] == 20).all()
    with pytest.raises(ValueError):
        search.run(45)                                               # 20 + 45 > max_iterations


@pytest.mark.parametrize("kind,dyn", [(2, True), (3, False)])
def test_a_captured_run_replays_as_the_search(kind, dyn):
    """A graph of run(n) (one stream, no parallel branches) replayed after reset() leaves what run(n) leaves."""
    import torch

    from snac_amd import UCTSearch

    B, n = 128, 24
    env = _env(kind, dyn, B, 41 + kind)
    search = UCTSearch(env, 48, H[kind] // 2, 0.95, max_iterations=n)
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
    assert (search.visits[search._roots] == n).all()


@pytest.mark.parametrize("kind,dyn,probs", [(3, True, [4, 1, 1, 1, 1, 0, 2, 3]), (2, False, [1, 3, 0, 2, 2])])
def test_search_follows_the_action_distribution(kind, dyn, probs):
    B = 64
    env = _env(kind, dyn, B, 51 + kind, action_probs=probs)
    _pair(env, B, 32, H[kind] // 2, 48, None)


@pytest.mark.parametrize("kind,dyn", [(2, True)])
def test_search_on_a_non_default_env_equals_the_restatement_bit_for_bit(kind, dyn):
    """env_id_base 1000, a 64-bit seed, brick_gt / time_gt, total_step 9 and an action distribution: rollouts run into the time limit."""
    B = 64
    env = _env(kind, dyn, B, NON_DEFAULT_SEED, **NON_DEFAULT)
    assert env.env_id_base == 1000 and env.seed >> 32 == 9 and env.total_step == 9 and env.brick_gt and env.time_gt
    search, ref = _pair(env, B, 32, H[kind] // 2, 48, None, chunks=(17, None))
    assert (search.tree_sizes().cpu().numpy() > 1).all()
