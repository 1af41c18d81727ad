"""GPU: re-rooting UCT trees after a move (UCTSearch.advance; snac_uct_advance, k_uct.hip) against a restatement of the rules of
include/snac_hip.h ("Re-rooting after a move") in numpy: the kept rows found by walking parents, the records moved by torch indexing on
the restatement's own pool, the untried case by an in-place pool.transition with the same counter words.  Only live rows are compared
([base, base + used) of each tree: statistics and records), with the tree sizes and the outputs; rows above them are unspecified."""
import math

import numpy as np
import pytest

from devmem import _env, _subtree
import helpers  # noqa: F401
import rng_spec
from test_gpu_uct import H, KINDS, NON_DEFAULT, NON_DEFAULT_SEED, Restatement

pytestmark = pytest.mark.gpu


def _kept(parent, c, end):
    """Rows of [c, end) whose parent chain reaches c, in increasing order (c first)."""
    rows = [c]
    for i in range(c + 1, end):
        x = i
        while x > c:
            x = int(parent[x])
        if x == c:
            rows.append(i)
    return rows


class Advancing(Restatement):
    """Restatement + advance(actions)."""

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
            old = np.array(_kept(self.parent, c, base + used))
            n = len(old)
            new = base + np.arange(n)
            o2n = {int(o): base + j for j, o in enumerate(old)}
            ch = self.child[old]
            ch = np.array([[o2n[int(x)] if x >= 0 else -1 for x in r] for r in ch], np.int64).reshape(n, self.A)
            par = np.array([o2n.get(int(p), -1) for p in self.parent[old]], np.int64)
            fields = [a[old].copy() for a in (self.action, self.reward, self.terminal, self.visits, self.W, self.leaf_count)]
            self.pool.records[torch.as_tensor(new, device=dev)] = self.pool.records[torch.as_tensor(old, device=dev)].clone()
            self._clear(base, base + cap)
            self.child[new], self.parent[new] = ch, par
            for a, f in zip((self.action, self.reward, self.terminal, self.visits, self.W, self.leaf_count), fields):
                a[new] = f
            self.parent[base], self.action[base], self.reward[base] = -1, -1, 0.0
            self.used[b] = n
        return out_r, out_d

    def _clear(self, lo, hi):
        self.child[lo:hi], self.parent[lo:hi], self.action[lo:hi] = -1, -1, -1
        self.reward[lo:hi], self.terminal[lo:hi], self.visits[lo:hi], self.W[lo:hi], self.leaf_count[lo:hi] = 0, False, 0, 0.0, 0


def _live(B, cap, used):
    return np.concatenate([b * cap + np.arange(int(used[b])) for b in range(B)])


def _same_live(search, ref):
    import torch

    torch.cuda.synchronize()
    A, B, cap = ref.A, ref.B, ref.cap
    used = search.tree_sizes().cpu().numpy()
    assert np.array_equal(used, ref.used)
    rows = _live(B, cap, used)
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
    assert not search.stats[ri, 39:].any()                          # the zero words


def _pair(env, B, cap, iterations, rows=None, gamma=0.97):
    from snac_amd import UCTSearch

    horizon = H[env.kind] // 4
    search = UCTSearch(env, cap, horizon, gamma, max_iterations=iterations, trees=B)
    search.reset(rows=rows)
    ref = Advancing(env, B, cap, horizon, gamma, math.sqrt(2), rows)
    return search, ref


def _run(search, ref, n):
    search.run(n)
    for _ in range(n):
        ref.iteration()
    _same_live(search, ref)


def _advance(search, ref, actions):
    import torch

    a = torch.as_tensor(np.asarray(actions), device=search.env.device)
    r, d = search.advance(a)
    er, ed = ref.advance(np.asarray(actions))
    _same_live(search, ref)
    assert r.dtype == torch.float32 and d.dtype == torch.bool
    assert r.cpu().numpy().tobytes() == er.tobytes()
    assert np.array_equal(d.cpu().numpy(), ed)
    return r, d


def _mixed(search, rng):
    """Per tree: the lowest untried root action where there is one (every other tree), else a random one."""
    B, A = search.trees, search.num_actions
    ch = search.stats[search._roots][:, :A].cpu().numpy()
    a = rng.integers(0, A, B)
    for b in range(0, B, 2):
        u = np.nonzero(ch[b] < 0)[0]
        if len(u):
            a[b] = u[0]
    return a, ch


@pytest.mark.parametrize("kind,dyn", KINDS)
def test_advance_equals_the_restatement_bit_for_bit(kind, dyn):
    rng = np.random.default_rng(kind * 2 + dyn)
    B, cap = 48, 24
    env = _env(kind, dyn, B, 61 + kind + dyn)
    search, ref = _pair(env, B, cap, 90)
    _run(search, ref, 30)
    assert (search.tree_sizes().cpu().numpy() == cap).any()         # exhausted budgets among the trees
    _advance(search, ref, search.best_actions().cpu().numpy())
    _run(search, ref, 20)
    untried = tried = 0
    for _ in range(2):                                               # the second move from the first one's (smaller) tree
        a, ch = _mixed(search, rng)
        untried += int((ch[np.arange(B), a] < 0).sum())
        tried += int((ch[np.arange(B), a] >= 0).sum())
        _advance(search, ref, a)
    assert untried and tried                                         # untried and tried actions both played
    _run(search, ref, 25)
    assert search.iterations == 75


@pytest.mark.parametrize("kind,dyn", [(2, True)])
def test_advance_on_a_non_default_env_equals_the_restatement_bit_for_bit(kind, dyn):
    """env_id_base 1000, a 64-bit seed, brick_gt / time_gt, total_step 9 and an action distribution: the move's edge is keyed by
    (1000 + b, it * (H + 1)); after three moves the episodes are a few steps from the time limit."""
    rng = np.random.default_rng(7)
    B, cap = 16, 24
    env = _env(kind, dyn, B, NON_DEFAULT_SEED, **NON_DEFAULT)
    assert env.env_id_base == 1000 and env.seed >> 32 == 9 and env.total_step == 9 and env.brick_gt and env.time_gt
    search, ref = _pair(env, B, cap, 90)
    _run(search, ref, 30)
    _advance(search, ref, search.best_actions().cpu().numpy())
    _run(search, ref, 20)
    untried = tried = 0
    for _ in range(2):
        a, ch = _mixed(search, rng)
        untried += int((ch[np.arange(B), a] < 0).sum())
        tried += int((ch[np.arange(B), a] >= 0).sum())
        _advance(search, ref, a)
    assert untried and tried
    _run(search, ref, 25)
    assert search.iterations == 75


@pytest.mark.parametrize("kind,dyn", [(2, True), (3, False), (1, True)])
def test_the_kept_subtree_is_the_old_subtree(kind, dyn):
    import torch

    B, cap = 32, 96
    env = _env(kind, dyn, B, 71 + kind)
    search, _ = _pair(env, B, cap, 80)
    search.run(80)
    torch.cuda.synchronize()
    a = search.best_actions().cpu().numpy()
    before, rec_before = search.stats.clone().cpu().numpy(), search.pool.records.clone()
    search.advance(a)
    torch.cuda.synchronize()
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
        assert after[base, 32] == -1 and after[base, 33] == -1 and after[base, 38] == 0
        oi, ni = torch.as_tensor(old, device=env.device), torch.as_tensor(new, device=env.device)
        assert torch.equal(rec_before[oi], rec_after[ni])


@pytest.mark.parametrize("kind,dyn", [(2, True), (3, True), (1, False)])
def test_an_untried_action_leaves_the_transition_of_the_root(kind, dyn):
    import torch

    from snac_amd import NodePool

    B, cap = 64, 4
    env = _env(kind, dyn, B, 81 + kind)
    search, _ = _pair(env, B, cap, 10)
    search.run(2)                                                    # two children tried at most: untried actions remain
    torch.cuda.synchronize()
    A = search.num_actions
    ch = search.stats[search._roots][:, :A].cpu().numpy()
    a = np.array([int(np.nonzero(r < 0)[0][-1]) for r in ch])
    old_roots = search.pool.records[search._roots].clone()
    t = search.iterations * (search.horizon + 1)
    r, d = search.advance(a)
    twin = NodePool(env, B)
    twin.records.copy_(old_roots)
    _, er, ed = twin.transition(torch.as_tensor(a.astype(np.int8)), t=t, want_obs=False)
    torch.cuda.synchronize()
    assert torch.equal(search.pool.records[search._roots], twin.records)
    assert (search.tree_sizes().cpu().numpy() == 1).all()
    assert torch.equal(r, er) and torch.equal(d, ed)
    root = search.stats[search._roots].cpu().numpy()
    assert (root[:, 0:8] == -1).all() and not root[:, 8:32].any()
    assert (root[:, 32:34] == -1).all() and np.array_equal(root[:, 34] != 0, ed.cpu().numpy())
    assert not root[:, 35:].any()


def test_a_terminal_root_is_left_unchanged():
    import torch

    from snac_amd import _lib

    B, cap = 64, 16
    env = _env(2, True, B, 91)
    env._hdr.view(torch.int8).view(B, 16)[1::3, 2] |= _lib.FLAG_NEED_RESET
    search, _ = _pair(env, B, cap, 40)
    search.run(20)
    torch.cuda.synchronize()
    stats, records, used = search.stats.clone(), search.pool.records.clone(), search.tree_sizes()
    a = torch.randint(0, env.num_actions, (B,), device=env.device)
    r, d = search.advance(a)
    torch.cuda.synchronize()
    term = np.zeros(B, bool)
    term[1::3] = True
    rows = torch.as_tensor(_live(B, cap, np.full(B, cap))[np.repeat(term, cap)], device=env.device)
    assert torch.equal(search.stats[rows], stats[rows]) and torch.equal(search.pool.records[rows], records[rows])
    assert torch.equal(search.tree_sizes()[1::3], used[1::3])
    assert (r.cpu().numpy()[term] == 0).all() and d.cpu().numpy()[term].all()
    assert (search.tree_sizes().cpu().numpy()[~term] < cap).any()   # the other trees did re-root


@pytest.mark.parametrize("kind,dyn", [(2, True), (3, True), (1, True)])
def test_moves_follow_the_env(kind, dyn):
    """M moves on B envs: the roots' records are the rows of a fork of the env stepped with the same actions, and the move's rewards and
    done flags are env.step's.  Each step takes the step size of the counter word of the edge that made the new root: the edge of the
    iteration that expanded the child, or the move's own edge for an untried action."""
    import torch

    from snac_amd import NodePool

    B, cap, M, per = 64, 48, 6, 12
    env = _env(kind, dyn, B, 101 + kind)
    twin = env.fork(torch.arange(B, device=env.device))
    search, _ = _pair(env, B, cap, M * per)
    Hs = search.horizon
    made = np.zeros(B * (cap + 1), np.int64)                         # t of the edge that made each node
    roots = np.arange(B) * cap
    alive = np.ones(B, bool)
    for _ in range(M):
        for _ in range(per):
            before, t = search.tree_sizes().cpu().numpy(), search.iterations * (Hs + 1)
            search.run(1)
            after = search.tree_sizes().cpu().numpy()
            made[(roots + after - 1)[after > before]] = t
        a = search.best_actions()
        ch, par, used = search.children.cpu().numpy(), search.parent.cpu().numpy(), search.tree_sizes().cpu().numpy()
        t_move, tk, moved = search.iterations * (Hs + 1), np.zeros(B, np.int64), made.copy()
        for b in np.nonzero(alive)[0]:                              # a done tree's root is terminal: nothing moves
            c = int(ch[roots[b], int(a[b])])
            if c < 0:
                tk[b] = moved[roots[b]] = t_move
            else:
                kept = _kept(par, c, roots[b] + int(used[b]))
                tk[b] = made[c]
                moved[roots[b]:roots[b] + len(kept)] = made[kept]
        ks = rng_spec.step_size_of(rng_spec.words(env.seed, rng_spec.STREAM_STEP, env.env_id_base + np.arange(B), tk)).astype(np.int8)
        r, d = search.advance(a)
        _, er, ed = twin.step(a.to(torch.int8), step_size=torch.as_tensor(ks, device=env.device), want_obs=False)
        packed = NodePool(twin, B)
        packed.load()
        torch.cuda.synchronize()
        live = torch.as_tensor(np.nonzero(alive)[0], device=env.device)
        made = moved
        assert torch.equal(search.pool.records[search._roots][live], packed.records[live])
        assert torch.equal(r[live], er[live]) and torch.equal(d[live], ed[live])
        alive &= ~d.cpu().numpy()
    assert alive.any()
    search.store_roots()
    torch.cuda.synchronize()
    live = torch.as_tensor(np.nonzero(alive)[0], device=env.device)
    assert torch.equal(env.observe()[live], twin.observe()[live])
    assert torch.equal(env.iou()[live], twin.iou()[live])


@pytest.mark.parametrize("kind,dyn,B,cap,its", [(2, True, 3, 4608, 4600), (3, True, 2, 4800, 4700), (1, True, 16, 1, 3)])
def test_large_trees_tiny_trees_and_exhausted_budgets(kind, dyn, B, cap, its):
    """Trees of more than 4096 nodes (2D: the walk and the move over many chunks), long runs of 3D records, and trees of one node,
    against the restatement of advance applied to the device's own statistics and records just before the call."""
    import torch

    env = _env(kind, dyn, B, 111 + kind)
    search, ref = _pair(env, B, cap, its + 1)
    search.run(its)
    torch.cuda.synchronize()
    if kind == 2:
        assert search.tree_sizes().max().item() >= 4096
    # load the device's state into the restatement
    ref.child[:] = search.children.cpu().numpy()
    ref.parent[:], ref.action[:] = search.parent.cpu().numpy(), search.action.cpu().numpy()
    ref.reward[:], ref.terminal[:] = search.reward.cpu().numpy(), search.terminal.cpu().numpy()
    ref.visits[:], ref.W[:] = search.visits.cpu().numpy(), search.value_sum.cpu().numpy()
    ref.used[:] = search.tree_sizes().cpu().numpy()
    ref.pool.records.copy_(search.pool.records)
    ref.it = search.iterations
    a = search.best_actions().cpu().numpy()
    if cap == 1:
        a = np.arange(B) % env.num_actions
    _advance(search, ref, a)
    if cap == 1:
        assert (search.tree_sizes().cpu().numpy() == 1).all()
    search.run(1)
    ref.iteration()
    _same_live(search, ref)


def test_advance_does_not_synchronise_with_the_host():
    import torch

    from snac_amd import UCTSearch

    env = _env(2, True, 256, 121)
    search = UCTSearch(env, 32, 100, 0.97, max_iterations=64)
    search.reset()
    search.run(10)
    a = torch.randint(0, env.num_actions, (256,), device=env.device)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r, d = search.advance(a, check=False)
        search.run(5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert r.shape == (256,) and d.shape == (256,)
    assert (search.visits[search._roots] >= 5).all()


@pytest.mark.parametrize("kind,dyn", [(2, True), (3, False)])
def test_a_captured_run_advance_run_replays_as_the_eager_sequence(kind, dyn):
    import torch

    from snac_amd import UCTSearch

    B, n, m = 128, 16, 12
    env = _env(kind, dyn, B, 131 + kind)
    search = UCTSearch(env, 40, H[kind] // 2, 0.95, max_iterations=n + m)
    a = torch.randint(0, env.num_actions, (B,), device=env.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # warm-up outside capture
        search.reset()
        search.run(2)
        search.advance(a, check=False)
    torch.cuda.current_stream().wait_stream(side)
    search.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        search.run(n)
        r_g, d_g = search.advance(a, check=False)
        search.run(m)
    search.reset()
    g.replay()
    torch.cuda.synchronize()
    stats, records, used = search.stats.clone(), search.pool.records.clone(), search.tree_sizes()
    r_g, d_g = r_g.clone(), d_g.clone()
    search.reset()
    search.run(n)
    r, d = search.advance(a, check=False)
    search.run(m)
    torch.cuda.synchronize()
    assert torch.equal(search.stats, stats) and torch.equal(search.pool.records, records)
    assert torch.equal(search.tree_sizes(), used)
    assert torch.equal(r, r_g) and torch.equal(d, d_g)


def test_advance_rejects_bad_actions_and_keeps_counting_iterations():
    import torch

    from snac_amd import UCTSearch

    B = 64
    env = _env(2, False, B, 141)
    search = UCTSearch(env, 16, 50, 0.97, max_iterations=30)
    search.reset()
    search.run(10)
    A = env.num_actions
    for bad in (np.zeros(B - 1, np.int64), np.zeros(B + 1, np.int64), np.full(B, A), np.full(B, -1), np.zeros(B, np.float32)):
        with pytest.raises(ValueError):
            search.advance(torch.as_tensor(bad, device=env.device))
    assert search.iterations == 10
    search.advance([A - 1] * B)                                      # a python sequence
    assert search.iterations == 10
    search.run(20)
    with pytest.raises(ValueError):
        search.run(1)                                                # 10 + 20 + 1 > max_iterations across the move
    search.advance(search.best_actions())
    with pytest.raises(ValueError):
        search.run(1)
    torch.cuda.synchronize()
    assert (search.tree_sizes().cpu().numpy() >= 1).all()
