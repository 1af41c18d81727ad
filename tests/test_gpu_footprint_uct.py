"""GPU: no UCT, self-play or reanalyse kernel writes outside its outputs (tests/guard.py; the other half of the ABI after
tests/test_gpu_footprint.py, tests/test_gpu_footprint_nodes.py and tests/test_gpu_footprint_state.py).

UCTSearch, SelfPlay, NodePool and PriorityTree allocate in their constructors and keep raw pointers, so the objects under test are BUILT
inside guard.allocations(module, arena=A) for snac_amd.uct, .nodes, .selfplay and .priority: statistics, node records, used, the slot
arrays, q_bounds, cand, the work array and the ring all lie in one arena, each with 64 KiB of 0xA5 on both sides, and so does every
result a call allocates itself.  The reference is a twin built the same way in plain torch tensors (guard.fresh_allocations) over a twin
env of the same seed that takes the same public calls in the same order; those paths are pinned against their python restatements by
tests/test_gpu_uct*.py, so equality with the twin is equality with the specification.  After EVERY public call: every tensor attribute
of search, pool, self-play, tree and env equals the twin's of the same name byte for byte (vars() is walked), then arena.check().  The
clauses the header documents as "not written" are asserted beside that (see _Pair and the self-play configurations).

Shapes: CONFIGS, a covering list.  Trees B in 1 3 63 64 65 129 (one lane per tree in 64-thread blocks; a wave per tree, four per block;
256-thread blocks over B * K slots), nodes per tree in 1 2 9 40 (a root that never expands; two sizes that the iterations exhaust, so the
used[b] == cap branch and the last row of the last tree are written; one that stays open), paths K in 1 3 16 with B * K on both sides
of 256, the three kinds (records of 128 and 896 bytes), total_step 5 with every third env row, counted from the last,
one step and three steps before it (_stagger), so that roots are terminal at some advance() and not at others, a ring of 3 moves with 7
played.  The returns kernels over a wrapped part of the ring are called through the C ABI: targets() names the whole ring once it wraps.

The objects' `_lib` is replaced by a recorder of attribute look-ups; the last test fails if one of the UCT entry points (the header's 23
snac_uct_* functions) was never called, and prints the table entry point x modes x shapes."""
import ctypes as C
import os
import time

import pytest

from devmem import _env
import guard
from test_gpu_uct_puct import make_evaluator

pytestmark = pytest.mark.gpu

ENTRY_POINTS = ["snac_uct_select", "snac_uct_backup", "snac_uct_advance", "snac_uct_select_paths", "snac_uct_select_paths_norm",
                "snac_uct_backup_paths", "snac_uct_backup_paths_norm", "snac_uct_select_puct", "snac_uct_select_puct_norm", "snac_uct_set_priors",
                "snac_uct_set_priors_value", "snac_uct_select_gumbel", "snac_uct_select_gumbel_interior", "snac_uct_gumbel_candidates",
                "snac_uct_improved_policy", "snac_uct_bounds", "snac_uct_pick_moves", "snac_uct_restart", "snac_uct_returns", "snac_uct_returns_nstep",
                "snac_uct_save_roots", "snac_uct_load_roots", "snac_uct_store_targets"]
# (23 names: every snac_uct_* function the header declares -- the last test holds the list against the header)
TOTAL_STEP, MOVES, RING = 5, 7, 3
GAMMA, C_PUCT, VL, HORIZON = 0.97, 1.25, 0.5, 6

# name: (mode, kind, B, cap, K, iterations per move)
CONFIGS = {
    "rollout-1 2D B65 cap9": ("rollout", 2, 65, 9, 1, 12),
    "rollout-1 1D B1 cap1": ("rollout", 1, 1, 1, 1, 2),
    "rollout-K 3D B65 cap9 K3": ("rollout", 3, 65, 9, 3, 8),
    "rollout-K 2D B16 cap40 K16": ("rollout", 2, 16, 40, 16, 1),
    "rollout-norm 1D B129 cap2 K3": ("rollout_norm", 1, 129, 2, 3, 2),
    "rollout-norm 2D B63 cap9 K1": ("rollout_norm", 2, 63, 9, 1, 12),
    "puct 2D B64 cap9 K3": ("puct", 2, 64, 9, 3, 8),
    "puct 3D B3 cap40 K16": ("puct", 3, 3, 40, 16, 1),
    "puct-norm 1D B65 cap2 K16": ("puct_norm", 1, 65, 2, 16, 2),
    "gumbel 2D B129 cap9 K3": ("gumbel", 2, 129, 9, 3, 8),
    "gumbel-interior 3D B63 cap40 K3": ("gumbel_interior", 3, 63, 40, 3, 4),
    "gumbel-interior 1D B64 cap1 K1": ("gumbel_interior", 1, 64, 1, 1, 2),
    "selfplay 2D B65 cap9 K3": ("selfplay", 2, 65, 9, 3, 4),
    "selfplay 3D B3 cap40 K3": ("selfplay", 3, 3, 40, 3, 2),
}
MODULES = ("uct", "nodes", "selfplay", "priority")
REACH = {}                                                             # entry point -> [configuration names]
_DONE, _FAILED = {}, set()                                             # configuration name -> seconds; the ones that raised


class Recorder:
    """The library handle of an object under test: counts the attribute look-ups by name, and is the library otherwise."""

    def __init__(self, lib, counts):
        self.__dict__["_lib"], self.__dict__["_counts"] = lib, counts

    def __getattr__(self, name):
        self._counts[name] = self._counts.get(name, 0) + 1
        return getattr(self._lib, name)


def _patched(arena):
    """The four modules' allocations from the arena (None: plain tensors, empty() fresh -- the twin)."""
    import contextlib
    import importlib

    stack = contextlib.ExitStack()
    for m in MODULES:
        mod = importlib.import_module("snac_amd." + m)
        stack.enter_context(guard.allocations(mod, arena=arena) if arena is not None else guard.fresh_allocations(mod))
    return stack


def _raw(t):
    import torch

    t = t.reshape(-1)
    if t.numel() and t.stride(0) != 1:                                 # (a one-element slice keeps its stride through contiguous())
        t = torch.empty(t.shape, dtype=t.dtype, device=t.device).copy_(t)
    return t.view(torch.uint8) if t.numel() else t


def _eq(a, b):
    import torch

    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_raw(a), _raw(b))


def _tensors(obj):
    import torch

    return {k: v for k, v in vars(obj).items() if torch.is_tensor(v)}


def _stagger(env):
    """count_step of every third row, counted from the last, one / three steps before the time limit: their episodes end at the first /
    third move.  The last row (the last tree, whose rows end the arrays) starts a full episode."""
    import torch

    n = env.num_envs
    cs = env._hdr.view(torch.int16).view(n, 8)[:, 3]
    back = n - 1 - torch.arange(n, device=env.device)
    cs[back % 3 == 1] = TOTAL_STEP - 1
    cs[back % 3 == 2] = TOTAL_STEP - 3


def _build(mode, kind, B, cap, K, its, trees=None, env=None):
    from snac_amd import UCTSearch

    env = env or _env(kind, True, B, 20 + kind, total_step=TOTAL_STEP)
    A = env.num_actions
    kw = dict(max_iterations=(2 * MOVES + 2) * its, paths=K, trees=trees)
    if mode in ("rollout", "rollout_norm"):
        s = UCTSearch(env, cap, HORIZON, GAMMA, virtual_loss=VL if K > 1 else 0.0, q_normalise=mode == "rollout_norm", **kw)
    else:
        fn = make_evaluator(A, False)
        g = dict(gumbel=4, gumbel_interior=mode == "gumbel_interior") if mode.startswith("gumbel") else {}
        s = UCTSearch(env, cap, 0, GAMMA, c=C_PUCT, virtual_loss=VL, evaluator=fn, q_normalise=mode != "puct" and mode != "selfplay", **kw, **g)
    return env, s


class _Pair:
    """The objects under test in the arena and their twins in plain tensors.  call(name, ...) makes one public call on both, compares what
    it returns, then every tensor attribute of every object, then checks the bands."""

    def __init__(self, name):
        import torch

        self.name = name
        self.mode, self.kind, self.B, self.cap, self.K, self.its = CONFIGS[name]
        self.counts = {}
        with _patched(None):                                           # the twin first: what it holds sizes the arena
            self.tenv, self.tw = _build(*CONFIGS[name])
        held = sum(v.numel() * v.element_size() for o in (self.tw, self.tw.pool) for v in _tensors(o).values())
        ring = RING * self.B * (self.tenv.obs_dim * 8 + 8 * 4 + self.tw.pool.WORDS * 4 + 64) + 64 * RING * self.B
        carves = sum(len(_tensors(o)) for o in (self.tw, self.tw.pool)) * 2 + 260
        self.A = guard.Arena(3 * held + 3 * ring + carves * (guard.BAND + 4096), self.tenv.device)
        with _patched(self.A):
            self.env, self.s = _build(*CONFIGS[name])
        for e in (self.env, self.tenv):
            _stagger(e)
        self.objs, self.twins = {"search": self.s, "pool": self.s.pool, "env": self.env}, {"search": self.tw, "pool": self.tw.pool, "env": self.tenv}
        self.watch(self.s), self.watch(self.s.pool)
        self.flags = dict(terminal_advance=False, live_advance=False, restarted=False, left_alone=False)
        self.torch = torch

    def watch(self, obj):
        obj._lib = Recorder(obj._lib, self.counts)

    def inside(self, t):
        lo = self.A.buf.data_ptr()
        return lo <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= lo + self.A.buf.numel()

    def owned(self, obj, names):
        for n in names:
            t = getattr(obj, n)
            assert t is not None and self.inside(t), "%s.%s is not in the arena" % (type(obj).__name__, n)

    def same(self, what):
        for key, o in self.objs.items():
            a, b = _tensors(o), _tensors(self.twins[key])
            assert a.keys() == b.keys(), (self.name, what, key, sorted(set(a) ^ set(b)))
            for k in a:
                assert _eq(a[k], b[k]), "%s, after %s: %s.%s differs from the twin's" % (self.name, what, key, k)
        self.A.check()

    def call(self, key, method, *args, twin_args=None, **kw):
        """objs[key].method(*args) and the twin's; tensors among the results must be equal; then same()."""
        with _patched(self.A):                                         # what the call allocates itself is carved too
            got = getattr(self.objs[key], method)(*args, **kw)
        with _patched(None):
            want = getattr(self.twins[key], method)(*(args if twin_args is None else twin_args), **kw)
        g, w = (got, want) if isinstance(got, (tuple, list)) else ((got,), (want,))
        assert len(g) == len(w)
        for x, y in zip(g, w):
            if self.torch.is_tensor(x):
                assert _eq(x, y), "%s: what %s returns differs from the twin's" % (self.name, method)
            else:
                assert x == y, (self.name, method, x, y)
        self.same(method)
        return got

    # ---- the documented clauses ------------------------------------------------------------------------------------------------------
    def trees_of(self, s):
        """(statistics, records, used) with the trees' rows as [B, cap, words]: the scratch rows behind them left out."""
        B, cap = s.trees, s.nodes_per_tree
        return s.stats[:B * cap].view(B, cap, -1), s.pool.records[:B * cap].view(B, cap, -1), s._used

    def advance(self, actions):
        """snac_uct_advance on a terminal root: "the tree is unchanged (statistics, records, used[b])"."""
        term = self.tw.terminal[self.tw._roots].clone()
        before = [t.clone() for t in self.trees_of(self.s)]
        r, d = self.call("search", "advance", actions)
        assert self.inside(r) and self.inside(d), "advance() allocates its results through the module's torch"
        for t, b, what in zip(self.trees_of(self.s), before, ("statistics", "records", "used")):
            assert _eq(t[term], b[term]), "%s: advance() changed the %s of a tree whose root is terminal" % (self.name, what)
        assert bool(d[term].all()) and not bool(r[term].any())
        self.flags["terminal_advance"] |= bool(term.any())
        self.flags["live_advance"] |= not bool(term.all())
        return r, d

    def restart(self, mask):
        """restart(mask): the unmasked trees' rows, records and sizes are unchanged."""
        keep = ~mask
        before = [t.clone() for t in self.trees_of(self.s)]
        for e in (self.env, self.tenv):
            e.reset(mask=mask.to(e.device), want_obs=False)            # the finished trees' env rows: the next episode
        self.call("search", "restart", mask)
        for t, b, what in zip(self.trees_of(self.s), before, ("statistics", "records", "used")):
            assert _eq(t[keep], b[keep]), "%s: restart() changed the %s of a tree outside the mask" % (self.name, what)
        assert bool((self.tw.tree_sizes()[mask] == 1).all())
        self.flags["restarted"] |= bool(mask.any())
        self.flags["left_alone"] |= bool(keep.any())


def _search_config(name):
    """reset, then MOVES moves of: the search, the bounds, a move from the visit counts (or the Gumbel search's), advance -- with a
    restart of some trees after moves 2, 3 and 5, store_roots after move 4 -- then load_roots from stored records."""
    import torch

    p = _Pair(name)
    s, tw, B, cap, its = p.s, p.tw, p.B, p.cap, p.its
    dev, A = p.env.device, p.env.num_actions
    p.owned(s, ["stats", "_used", "_src", "_dst", "_leaf", "_action", "_expanded", "_r_leaf", "_reward", "_first", "_done", "_est", "_work",
                "_adv_action", "_adv_reward", "_adv_done", "_rs_mask", "_rs_term", "_rs_flags"])
    p.owned(s.pool, ["records"])
    if s.q_normalise:
        p.owned(s, ["q_bounds"])
    if s.gumbel is not None:
        p.owned(s, ["cand", "_gscores"])
    assert s.stats.data_ptr() % 128 == 0 and s.pool.records.data_ptr() % 128 == 0
    p.call("search", "reset")
    if s.evaluator is not None:
        p.call("search", "set_root_priors", s.root_priors() * 0.75 + 0.25 / A, twin_args=(tw.root_priors() * 0.75 + 0.25 / A,))
    arange = torch.arange(B, device=dev)
    stored = None
    for mv in range(MOVES):
        if s.gumbel is not None:
            p.call("search", "gumbel_begin", s.gumbel_scores(False), twin_args=(tw.gumbel_scores(False),))
            p.call("search", "gumbel_run", its)
        else:
            p.call("search", "run", its)
        if mv == 0 and cap in (2, 9):                              # exhausted: the used[b] == cap branch, the last row of the last tree
            deep = (B - 1 - arange) % 3 != 1 if cap == 9 else arange >= 0      # a root one step before the limit has its A children at most
            assert not bool(tw.terminal[tw._roots].any()) and bool(deep[-1])
            assert bool((tw.tree_sizes()[deep] == cap).all()), (name, tw.tree_sizes().tolist())
        if cap == 1:
            assert bool((tw.tree_sizes() == 1).all())
        if s.q_normalise:
            p.call("search", "q_bounds_of_trees")
        picked = p.call("search", "pick_moves", False, mv)
        assert all(p.inside(x) for x in picked)
        act = picked[0]
        if s.gumbel is not None:
            cand = s.cand.clone()
            act = p.call("search", "gumbel_actions")               # PICK: "cand is not written"
            assert _eq(s.cand, cand), "%s: gumbel_actions() wrote cand" % name
            pi = p.call("search", "improved_policy")
            assert p.inside(act) and (not s.gumbel_interior or p.inside(pi))
        if mv == 1:
            stored = p.A.carve(tuple(s.pool.records.shape), torch.int32, name="stored records (input)").copy_(s.pool.records)
        p.advance(act.long())
        if mv == 2:
            p.restart((B - 1 - arange) % 3 == 1)                   # the trees that ended at the first move (B = 1: none)
        if mv == 3:
            p.restart(arange < 0)                                  # no tree
        if mv == 5:
            p.restart(torch.ones(B, dtype=torch.bool, device=dev) if B == 1 else arange % 2 == 1)
        if mv == 4:
            p.call("search", "store_roots")
    # load_roots: stored records, an index that is clamped on both sides
    rows = int(stored.shape[0])
    index = (arange * 7 + 3) % rows
    index[0] = -5
    index[-1] = rows + 9
    keep = stored.clone()
    p.call("search", "load_roots", stored.view(torch.uint8).view(rows, -1), index)
    assert _eq(stored, keep), "the stored records are an input"
    assert bool((tw.tree_sizes() == 1).all())
    p.call("search", "run", its)
    assert p.flags["terminal_advance"] and p.flags["live_advance"], (name, p.flags)
    assert p.flags["restarted"] and p.flags["left_alone"], (name, p.flags)
    return p.counts


def _selfplay_config(name):
    """SelfPlay(keep_states=True, prioritized=True) on a PUCT search: MOVES moves into RING slots one by one, targets(), targets(td_steps=2),
    the two returns kernels over part of the ring (a wrapped range included), reanalyse uniform, prioritised and with a -1 entry."""
    import torch
    from snac_amd import SelfPlay

    p = _Pair(name)
    s, tw, B, its = p.s, p.tw, p.B, p.its
    dev = p.env.device
    R = min(8, B + 1)
    with _patched(p.A):
        play = SelfPlay(s, RING, sample_moves=2, keep_states=True, prioritized=True)
        _, again = _build("puct", p.kind, B, p.cap, 1, its, trees=R, env=p.env)
    with _patched(None):
        tplay = SelfPlay(tw, RING, sample_moves=2, keep_states=True, prioritized=True)
        _, tagain = _build("puct", p.kind, B, p.cap, 1, its, trees=R, env=p.tenv)
    p.objs.update(play=play, tree=play.tree, again=again, again_pool=again.pool)
    p.twins.update(play=tplay, tree=tplay.tree, again=tagain, again_pool=tagain.pool)
    for o in (play.tree, again, again.pool):
        p.watch(o)
    ring = ["obs", "pi", "value", "reward", "z", "action", "done", "move", "state", "refreshed"]
    p.owned(play, ring)
    p.owned(play.tree, ["buffer"])
    p.owned(again, ["stats", "_used", "_work"])
    assert play.state.data_ptr() % 128 == 0
    p.call("search", "reset")
    p.same("construction")
    mixed = False
    for mv in range(MOVES):
        h = play.head
        before = {n: getattr(play, n).clone() for n in ring}
        p.call("play", "play", 1, its)
        others = [i for i in range(RING) if i != h]
        for n in ring:                                             # save_roots: slot h of state only; pick_moves: slot h of action / pi / value only
            assert _eq(getattr(play, n)[others], before[n][others]), "%s: play() wrote `%s` outside slot %d" % (name, n, h)
        d = tplay.done[h].bool()
        mixed |= bool(d.any()) and not bool(d.all())               # the restart inside play(): some trees, not all
        if mv == 1:                                                # two of three slots hold a move: slot 2 is outside the count
            guard.fresh(play.z), guard.fresh(tplay.z)
            p.call("play", "targets")
            guard.view_untouched(play.z[2], "z of the slot outside the count (snac_uct_returns)")
            guard.fresh(play.z), guard.fresh(tplay.z)
            p.call("play", "targets", td_steps=2)
            guard.view_untouched(play.z[2], "z of the slot outside the count (snac_uct_returns_nstep)")
    assert play.moves == MOVES and play.head == MOVES % RING and play.valid_moves() == RING, "the ring has wrapped"
    assert mixed or B == 1, "a restart inside play() took some trees and left others"
    p.call("play", "targets")
    p.call("play", "targets", td_steps=2)
    p.call("play", "targets", bootstrap=False)
    # the returns kernels over part of the ring: "Slots outside the count are not written"; first 2, count 2 wraps: slots 2 and 0
    stream = lambda e: C.c_void_p(torch.cuda.current_stream(e.device).cuda_stream)  # noqa: E731
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    from snac_amd import _lib
    for first, count, out in ((2, 2, 1), (1, 1, (0, 2)), (0, 2, 2)):
        for nstep in (False, True):
            for q, L, e in ((play, s._lib, p.env), (tplay, tw._lib, p.tenv)):
                guard.fresh(q.z)
                if nstep:
                    _lib.check(L.snac_uct_returns_nstep(B, RING, first, count, 2, GAMMA, vp(q.reward), vp(q.done), vp(q.value), None, vp(q.z), stream(e)))
                else:
                    _lib.check(L.snac_uct_returns(B, RING, first, count, GAMMA, vp(q.reward), vp(q.done), None, vp(q.z), stream(e)))
            what = "%s over slots %d + %d" % ("snac_uct_returns_nstep" if nstep else "snac_uct_returns", first, count)
            guard.view_untouched(play.z[torch.as_tensor(out).reshape(-1)], "z outside the count: " + what)
            assert bool((play.z[first].view(torch.uint8) != guard.FRESH_BYTE).any()), what + ": the first slot of the count is written"
            p.same(what)
    p.call("play", "targets")

    def reanalyse(what, **kw):
        """snac_uct_store_targets: pi, value, refreshed of entries not in index are unchanged; a -1 entry stores nothing."""
        before = {n: getattr(play, n).clone() for n in ring}
        flat = p.call("play", "reanalyse", again, its, **kw, twin_args=(tagain, its))
        keep = torch.ones(RING * B, dtype=torch.bool, device=dev)
        keep[flat[flat >= 0]] = False
        for n in ("pi", "value", "refreshed"):
            assert _eq(getattr(play, n).view(RING * B, -1)[keep], before[n].view(RING * B, -1)[keep]), "%s: %s wrote `%s` outside the index" % (name, what, n)
        assert bool((play.refreshed.view(-1)[~keep] == before["refreshed"].view(-1)[~keep] + 1).all())
        for n in ("obs", "reward", "z", "action", "done", "move", "state"):
            assert _eq(getattr(play, n), before[n]), (name, what, n)
        return flat

    gens = [torch.Generator(device=dev).manual_seed(5) for _ in range(2)]
    before_head = play.head
    # uniform: the twin needs its own generator of the same seed, so the two calls are made by hand
    snap = {n: getattr(play, n).clone() for n in ring}
    with _patched(p.A):
        f1 = play.reanalyse(again, its, generator=gens[0])
    with _patched(None):
        f2 = tplay.reanalyse(tagain, its, generator=gens[1])
    assert _eq(f1, f2) and int(torch.unique(f1).numel()) == R
    p.same("reanalyse (uniform)")
    keep = torch.ones(RING * B, dtype=torch.bool, device=dev)
    keep[f1] = False
    for n in ("pi", "value", "refreshed"):
        assert _eq(getattr(play, n).view(RING * B, -1)[keep], snap[n].view(RING * B, -1)[keep]), "%s: reanalyse wrote `%s` outside the index" % (name, n)
    assert bool((play.refreshed.view(-1)[f1] == 1).all()) and play.head == before_head
    p.call("play", "update_priorities", f1, (play.value.view(-1)[f1] - play.z.view(-1)[f1]).abs() + 0.125,
           twin_args=(f2, (tplay.value.view(-1)[f2] - tplay.z.view(-1)[f2]).abs() + 0.125))
    reanalyse("reanalyse (prioritised)", prioritized=True)
    index = ((torch.arange(R, device=dev) * 5 + 1) % (RING * B)).to(torch.int64)
    assert int(torch.unique(index).numel()) == R
    index[R // 2] = -1
    flat = reanalyse("reanalyse (index with a -1)", index=index, check=False)
    assert int((flat < 0).sum()) == 1
    return p.counts


@pytest.mark.parametrize("name", list(CONFIGS))
def test_uct_footprint(name):
    _run(name)


def _run(name):
    assert name not in _FAILED, "%s failed earlier in this process: not run again" % name
    if name not in _DONE:
        t0 = time.time()
        _FAILED.add(name)
        counts = (_selfplay_config if CONFIGS[name][0] == "selfplay" else _search_config)(name)
        _FAILED.discard(name)
        _DONE[name] = time.time() - t0
        for entry in ENTRY_POINTS:
            if counts.get(entry):
                REACH.setdefault(entry, []).append(name)
    return _DONE[name]


def test_every_uct_entry_point_was_reached():
    """Runs whatever configuration has not run in this process (so the test stands alone), then: each of the entry points was looked
    up on the library by some configuration.  Prints the table entry point x configurations (mode, kind, trees, nodes per tree, paths)."""
    for name in CONFIGS:
        _run(name)
    from snac_amd import _lib

    assert sorted(ENTRY_POINTS) == sorted(n for n in _lib.PROTOTYPES if n.startswith("snac_uct_")), "the list is the header's"
    lines = ["%-34s %s" % (e, "; ".join(REACH.get(e, [])) or "NEVER CALLED") for e in ENTRY_POINTS]
    lines += ["%-34s %.2f s" % (n, _DONE[n]) for n in CONFIGS]
    text = "\n".join(lines)
    print(text)
    d = os.environ.get("SNAC_FOOTPRINT_TABLE_DIR")
    if d:
        with open(os.path.join(d, "footprint_uct.txt"), "w") as f:
            f.write(text + "\n")
    missing = [e for e in ENTRY_POINTS if not REACH.get(e)]
    assert not missing, "never called: %s" % missing
