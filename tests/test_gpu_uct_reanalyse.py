"""GPU: Reanalyse (SelfPlay(keep_states=True) / reanalyse() / targets(td_steps=n), UCTSearch.load_roots(); snac_uct_save_roots /
snac_uct_load_roots / snac_uct_store_targets / snac_uct_returns_nstep, k_uct_reanalyse.hip) against the rules of include/snac_hip.h
("Reanalyse"), on top of the restatements of self-play (tests/test_gpu_uct_selfplay.py) and of PUCT (tests/test_gpu_uct_puct.py).

The rules, restated.  A ring with keep_states keeps, per move, the root records as they stood when the move was chosen; nothing else of
play() changes.  load_roots is reset() from records instead of env rows.  reanalyse() of R entries is what existing code gives for the
same states: the records unpacked into the rows of a twin env, reset(rows) of R trees in the same order, the same iterations, and
pick_moves() -- or the Gumbel search's improved_policy() -- for pi and value; only the indexed entries' pi, value and refreshed change.
The n-step target is the numpy restatement of tests/test_uct_reanalyse_host.py.  Every comparison is bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

from devmem import _env
from test_gpu_uct_puct import C as CPUCT
from test_gpu_uct_puct import GAMMA, VL, PuctRestatement, make_evaluator
from test_gpu_uct_puct import _same as _same_puct
from test_gpu_uct_selfplay import _bytes, _near_the_end, _pair, _run_both, _same, pick, restart, returns
from test_uct_reanalyse_host import nstep

pytestmark = pytest.mark.gpu

RING = ("obs", "pi", "value", "action", "reward", "done", "move", "z")
B1, CAP1, K1, ITS1, MOVES1, SLOTS1, SAMPLE1 = 12, 48, 3, 4, 7, 5, 2   # the shape of test_gpu_uct_selfplay._play_move_by_move


# ---- 1. the states are saved, and nothing else changes ------------------------------------------------------------------------------------
def _play(kind, dyn, keep_states):
    """(play, search, ref, env) after the move-by-move play of tests/test_gpu_uct_selfplay.py: 7 moves into 5 slots, PUCT."""
    import torch

    from snac_amd import SelfPlay, _lib

    ts = _lib.env_sizes(kind, dyn).total_step
    search, ref, env = _pair(kind, dyn, B1, 37 + kind, CAP1, K1, True, (ts + 1) * ITS1, prep=_near_the_end(kind, dyn), twin=True)
    play = SelfPlay(search, SLOTS1, sample_moves=SAMPLE1, keep_states=keep_states)
    play.play(3, ITS1)
    play.play(MOVES1 - 3, ITS1)
    torch.cuda.synchronize()
    return play, search, ref, env


@functools.lru_cache(maxsize=None)
def _played(kind, dyn):
    """The play with keep_states=True, shared by the tests below: none of them leaves it changed."""
    return _play(kind, dyn, True)


@pytest.mark.parametrize("kind,dyn", [(1, False), (2, True), (3, True)])
def test_play_keeps_the_root_records_and_changes_nothing_else(kind, dyn):
    import torch

    play, search, ref, env = _played(kind, dyn)
    renv = ref.env
    rb = search.pool.WORDS * 4
    assert rb == (896 if kind == 3 else 128)
    assert tuple(play.state.shape) == (SLOTS1, B1, rb) and play.state.dtype == torch.uint8
    assert tuple(play.refreshed.shape) == (SLOTS1, B1) and play.refreshed.dtype == torch.int32 and not play.refreshed.any()
    # the restatement, move by move: the root records before each advance
    roots = torch.arange(B1, device=env.device) * CAP1
    want = [None] * SLOTS1
    in_episode = np.zeros(B1, np.int64)
    restarts = np.zeros(B1, np.int64)
    for mv in range(MOVES1):
        for _ in range(ITS1):
            ref.iteration()
        want[mv % SLOTS1] = ref.pool.records[roots].clone()
        a = pick(ref, in_episode >= SAMPLE1, mv)[0]
        _, d = ref.advance(a)
        renv.reset(mask=torch.as_tensor(d, device=env.device), want_obs=False)
        restart(ref, d)
        restarts += d
        in_episode = np.where(d, 0, in_episode + 1)
    assert (restarts > 0).any() and (restarts == 0).any()            # the inputs: some trees started over inside the ring
    _same(search, ref, live_only=True)                               # the play itself is the restatement's
    for s in range(SLOTS1):
        assert torch.equal(play.state[s], want[s].view(torch.uint8)), s
    assert len({_bytes(play.state[s]) for s in range(SLOTS1)}) == SLOTS1          # the roots moved on between the slots
    # a twin run without the states: every other tensor of the ring, the trees and the env
    twin, tsearch, _, tenv = _play(kind, dyn, False)
    assert twin.state is None and twin.refreshed is None
    for k in RING:
        assert torch.equal(getattr(play, k), getattr(twin, k)), k
    assert torch.equal(play._move, twin._move) and (play.head, play.moves) == (twin.head, twin.moves)
    assert torch.equal(search.stats, tsearch.stats) and torch.equal(search.pool.records, tsearch.pool.records)
    assert torch.equal(search.tree_sizes(), tsearch.tree_sizes())
    for k in ("_hdr", "_episode", "_grid"):
        assert torch.equal(getattr(env, k), getattr(tenv, k)), k
    assert "refreshed" in play.sample(4) and "refreshed" not in twin.sample(4)


# ---- 2. load_roots is reset() -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dyn", [(2, True), (3, False)])
def test_load_roots_equals_reset(kind, dyn):
    import torch

    from snac_amd import NodePool, UCTSearch

    B, cap, K, n = 70, 24, 2, 3                                      # 18 workgroups of four trees, the last one half filled
    env = _env(kind, dyn, B, 51 + kind)
    _near_the_end(kind, dyn, terminal_roots=True)(env)
    A, dev = env.num_actions, env.device
    fn = make_evaluator(A, False)
    src = NodePool(env, B)
    src.load()                                                       # record i <- env row i
    records = src.records.view(torch.uint8)
    assert tuple(records.shape) == (B, 896 if kind == 3 else 128)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5)).to(dev)
    assert not torch.equal(perm, torch.arange(B, device=dev))
    need = src.need_reset[perm].cpu().numpy()
    assert need.any() and not need.all()                             # the input: terminal and live roots

    def make():
        return UCTSearch(env, cap, 0, GAMMA, c=CPUCT, max_iterations=2 * n, trees=B, paths=K, virtual_loss=VL, evaluator=fn)

    roots = torch.arange(B, device=dev) * cap
    scratch = B * cap + torch.arange(B, device=dev)

    def same_roots(a, b):
        assert torch.equal(a.stats[roots], b.stats[roots])           # the whole statistics rows, the priors in them
        assert torch.equal(a.pool.records[roots], b.pool.records[roots]) and torch.equal(a.pool.records[scratch], b.pool.records[scratch])
        assert torch.equal(a.tree_sizes(), b.tree_sizes()) and (a.tree_sizes() == 1).all()
        assert torch.equal(a.terminal[roots], b.terminal[roots])
        assert _bytes(a.root_priors()) == _bytes(b.root_priors()) and a.root_priors().any()
        assert a.iterations == b.iterations == 0

    fresh, loaded = make(), make()
    fresh.reset(rows=perm)
    loaded.reset()
    loaded.run(n)                                                    # trees to start over from: statistics, records and an iteration count
    assert (loaded.tree_sizes() > 1).any() and loaded.iterations == n
    loaded.load_roots(records, index=perm)
    torch.cuda.synchronize()
    same_roots(loaded, fresh)
    assert np.array_equal(loaded.terminal[roots].cpu().numpy(), need)
    assert torch.equal(loaded.pool.records[roots], src.records[perm])
    ref = PuctRestatement(env, B, cap, K, VL, 0, GAMMA, CPUCT, fn, 0.0, 2 * n, perm)
    fresh.run(n)
    loaded.run(n)
    for _ in range(n):
        ref.iteration()
    _same_puct(fresh, ref, live_only=True)
    _same_puct(loaded, ref, live_only=True)
    assert (loaded.tree_sizes().cpu().numpy()[~need] > 1).all()
    # index=None: record b
    fresh.reset()
    loaded.load_roots(records)
    torch.cuda.synchronize()
    same_roots(loaded, fresh)
    # an index outside [0, n) is clamped
    wild = perm.clone()
    wild[0], wild[1], wild[B - 1] = -5, B + 100, 1 << 30
    clamped = wild.clamp(0, B - 1)
    assert not torch.equal(wild, clamped)
    fresh.reset(rows=clamped)
    loaded.load_roots(records, index=wild.to(torch.int32))
    torch.cuda.synchronize()
    same_roots(loaded, fresh)
    assert torch.equal(loaded.pool.records[roots], src.records[clamped])
    assert torch.equal(src.records.view(torch.uint8), records)       # the source is read only


# ---- 3. reanalyse end to end --------------------------------------------------------------------------------------------------------------
R3 = 8
# slot 2 holds move 2, the last move of trees 1::3's first episode: their env rows have since started the next episode and plan
ENTRIES = [2 * B1 + 1, 0 * B1 + 2, 2 * B1 + 4, 3 * B1 + 0, 4 * B1 + 5, 2 * B1 + 7, 1 * B1 + 10, 3 * B1 + 11]


def _second(env, fn, mode, n):
    from snac_amd import UCTSearch

    kw = {} if mode == "puct" else dict(q_normalise=True, gumbel=4, gumbel_interior=mode == "interior")
    return UCTSearch(env, 32, 0, GAMMA, c=CPUCT, max_iterations=n, trees=R3, paths=2, virtual_loss=VL, evaluator=fn, **kw)


@pytest.mark.parametrize("mode", ["puct", "gumbel", "interior"])
@pytest.mark.parametrize("kind,dyn", [(2, True), (3, True)])
def test_reanalyse_equals_a_search_of_the_same_states(kind, dyn, mode):
    import torch

    from snac_amd import NodePool

    play, search, _, env = _played(kind, dyn)
    dev, A, n = env.device, env.num_actions, 6
    assert len(set(ENTRIES)) == R3 and play.valid_moves() == SLOTS1 and len(play) == SLOTS1 * B1
    index = torch.as_tensor(ENTRIES, device=dev)
    flat_state = play.state.view(SLOTS1 * B1, -1)
    chosen = flat_state[index]
    # the input: a chosen record's plan is not the plan its env row plays now
    then = chosen.view(torch.int16)[:, 5].cpu().numpy()
    now = env._hdr.view(torch.int16).view(B1, 8)[:, 5][index % B1].cpu().numpy()
    assert (then != now).any()
    before = {k: getattr(play, k).clone() for k in RING + ("state", "refreshed")}
    trees = (search.stats.clone(), search.pool.records.clone(), env._hdr.clone(), env._grid.clone())
    fn = make_evaluator(A, False)
    again = _second(env, fn, mode, n)
    try:
        got = play.reanalyse(again, n, index=index)
        torch.cuda.synchronize()
        assert torch.equal(got, index) and got.dtype == torch.int64
        # the reference: the same states in the rows of a twin env, searched by existing code
        tenv = _env(kind, dyn, B1, 37 + kind)
        pool = NodePool(tenv, R3)
        pool.records.copy_(chosen.view(torch.int32))
        pool.store(node_rows=torch.arange(R3, device=dev), rows=torch.arange(R3, device=dev))
        ref = _second(tenv, fn, mode, n)
        ref.reset(rows=torch.arange(R3, device=dev))
        if mode == "puct":
            ref._run(n)
            _, pi, value = ref.pick_moves()
        else:
            ref.gumbel_begin(ref.gumbel_scores(False))
            ref.gumbel_run(n)
            pi, value = ref.improved_policy(), ref.pick_moves()[2]
        torch.cuda.synchronize()
        assert torch.equal(again.pool.records[again._roots], chosen.view(torch.int32))               # the stored records were searched
        assert torch.equal(again.tree_sizes(), ref.tree_sizes())
        live = torch.cat([b * again.nodes_per_tree + torch.arange(int(u), device=dev) for b, u in enumerate(ref.tree_sizes().tolist())])
        assert torch.equal(again.stats[live], ref.stats[live]) and torch.equal(again.pool.records[live], ref.pool.records[live])
        assert (ref.visits[ref._roots] == n * 2).all() and pi.any() and value.any()
        flat_pi, flat_value, flat_n = play.pi.view(-1, A), play.value.view(-1), play.refreshed.view(-1)
        assert _bytes(flat_pi[index]) == _bytes(pi) and _bytes(flat_value[index]) == _bytes(value)
        assert (flat_n[index] == 1).all() and int(flat_n.sum()) == R3
        assert _bytes(flat_pi[index]) != _bytes(before["pi"].view(-1, A)[index])                     # the targets moved
        # everything else: byte for byte
        rest = torch.ones(SLOTS1 * B1, dtype=torch.bool, device=dev)
        rest[index] = False
        assert torch.equal(flat_pi[rest], before["pi"].view(-1, A)[rest]) and torch.equal(flat_value[rest], before["value"].view(-1)[rest])
        for k in RING + ("state",):
            if k not in ("pi", "value"):
                assert torch.equal(getattr(play, k), before[k]), k
        assert torch.equal(search.stats, trees[0]) and torch.equal(search.pool.records, trees[1])
        assert torch.equal(env._hdr, trees[2]) and torch.equal(env._grid, trees[3])
        # check=True: entries twice, or outside the ring
        for bad in ([ENTRIES[0]] * 2 + ENTRIES[2:], ENTRIES[:-1] + [SLOTS1 * B1], ENTRIES[:-1] + [-1]):
            with pytest.raises(ValueError):
                play.reanalyse(again, n, index=torch.as_tensor(bad, device=dev))
    finally:                                                         # the shared play stays as it was
        for k in ("pi", "value", "refreshed"):
            getattr(play, k).copy_(before[k])
        torch.cuda.synchronize()


# ---- 4. n-step targets --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _searched():
    search, ref, env = _pair(2, True, 70, 13, 16, 2, False, 8)
    _run_both(search, ref, 5)
    return search, pick(ref, True, 0)[2]


@pytest.mark.parametrize("moves", [4, 6, 9])
def test_n_step_targets_equal_the_restatement(moves):
    """The setup of test_targets_equal_the_recurrence, and random values in the ring: 4 moves leave two of six slots outside the valid
    range, 9 wrap the ring."""
    import torch

    from snac_amd import SelfPlay

    B, slots, gamma = 70, 6, 0.9                                     # two waves, the second partly filled
    search, boot = _searched()
    play = SelfPlay(search, slots, gamma=gamma)
    rng = np.random.default_rng(moves)
    reward = (rng.integers(-100, 11, size=(slots, B)) + rng.random((slots, B))).astype(np.float32)
    done = (rng.random((slots, B)) < 0.3).astype(np.uint8)
    value = (rng.integers(-50, 50, size=(slots, B)) + rng.random((slots, B))).astype(np.float32)
    play.reward.copy_(torch.as_tensor(reward))
    play.done.copy_(torch.as_tensor(done))
    play.value.copy_(torch.as_tensor(value))
    play.moves, play.head = moves, moves % slots
    valid = min(moves, slots)
    first = (play.head - valid) % slots
    assert boot.any() and done.any() and not done.all()
    sentinel = lambda: np.full((slots, B), -7.5, np.float32)  # noqa: E731
    seen = set()
    for bootstrap in (False, True):
        bt = boot if bootstrap else None
        play.z.fill_(-7.5)
        mc = _bytes(play.targets(bootstrap=bootstrap))
        assert mc == returns(reward, done, first, valid, gamma, bt, sentinel()).tobytes()
        for n in (1, 2, 3, 6, 100):
            play.z.fill_(-7.5)
            z = play.targets(bootstrap=bootstrap, td_steps=n)
            torch.cuda.synchronize()
            want = nstep(reward, done, value, first, valid, n, gamma, bt, sentinel())
            assert z is play.z and _bytes(z) == want.tobytes(), (bootstrap, n)
            if moves < slots:
                assert (want[moves:] == -7.5).all()                  # the slots outside the valid range keep the sentinel
            if n >= valid:
                assert _bytes(z) == mc, n                            # the Monte-Carlo targets, byte for byte
            seen.add(_bytes(z))
        assert _bytes(play.value) == value.tobytes()                 # read only
    assert len(seen) >= 6                                            # n = 1, 2, 3 and the whole window differ, with and without the bootstrap


def test_returns_nstep_over_a_part_of_the_ring():
    """The entry point itself, a window that wraps: slots 4, 5, 0, 1 of six; 2 and 3 keep the sentinel."""
    import torch

    from snac_amd import _lib

    B, slots, gamma = 130, 6, 0.97
    dev = torch.device("cuda")
    rng = np.random.default_rng(3)
    reward = rng.normal(size=(slots, B)).astype(np.float32)
    done = (rng.random((slots, B)) < 0.25).astype(np.uint8)
    value = rng.normal(size=(slots, B)).astype(np.float32)
    boot = rng.normal(size=B).astype(np.float32)
    r, d, v, bt = (torch.as_tensor(x, device=dev) for x in (reward, done, value, boot))
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n in (1, 2, 3, 4, 5, 0x7FFFFFFF):
        z = torch.full((slots, B), 3.25, dtype=torch.float32, device=dev)
        _lib.check(L.snac_uct_returns_nstep(B, slots, 4, 4, n, gamma, p(r), p(d), p(v), p(bt), p(z), stream))
        torch.cuda.synchronize()
        want = nstep(reward, done, value, 4, 4, n, gamma, boot, np.full((slots, B), 3.25, np.float32))
        assert _bytes(z) == want.tobytes(), n
        assert (want[2:4] == 3.25).all() and (want[[4, 5, 0, 1]] != 3.25).any()
        if n >= 4:
            assert want.tobytes() == returns(reward, done, 4, 4, gamma, boot, np.full((slots, B), 3.25, np.float32)).tobytes()
    z = torch.full((slots, B), 3.25, dtype=torch.float32, device=dev)
    _lib.check(L.snac_uct_returns_nstep(B, slots, 2, 1, 2, gamma, p(r), p(d), p(v), None, p(z), stream))     # one slot, no bootstrap
    torch.cuda.synchronize()
    assert _bytes(z[2]) == reward[2].tobytes() and (z[[0, 1, 3, 4, 5]] == 3.25).all()


# ---- 5. no host synchronisation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gumbel", [False, True])
def test_play_reanalyse_and_targets_do_not_synchronise_with_the_host(gumbel):
    import torch

    from snac_amd import SelfPlay, UCTSearch, _lib

    B, its, R = 64, 3, 16
    ts = _lib.env_sizes(2, True).total_step
    env = _env(2, True, B, 3)
    _near_the_end(2, True)(env)
    fn = make_evaluator(env.num_actions, False)
    search = UCTSearch(env, 64, 0, GAMMA, c=CPUCT, max_iterations=(ts + 1) * its, paths=4, virtual_loss=VL, evaluator=fn)
    search.reset()
    kw = dict(q_normalise=True, gumbel=4) if gumbel else {}
    again = UCTSearch(env, 32, 0, GAMMA, c=CPUCT, max_iterations=its, trees=R, paths=2, virtual_loss=VL, evaluator=fn, **kw)
    play = SelfPlay(search, 8, sample_moves=2, keep_states=True)
    g = torch.Generator(device=env.device).manual_seed(7)
    play.play(1, its)                                                # warm-up: rows 0::3 end here
    warm = play.reanalyse(again, its, generator=g)
    play.targets(td_steps=3)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        play.play(4, its)                                            # rows 1::3 end at the third move of their episode
        drawn = play.reanalyse(again, its, generator=g)              # index=None: drawn on the device
        given = play.reanalyse(again, its, index=drawn.flip(0), check=False)
        play.targets(td_steps=3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    done = play.done.cpu().numpy()[:5]
    assert done[0, 0::3].all() and done[1:, 1::3].any() and not done[:, 2::3].all()
    assert play.moves == 5 and search.iterations == 5 * its and again.iterations == its
    flat = drawn.cpu().numpy()
    assert len(set(flat.tolist())) == R and flat.min() >= 0 and flat.max() < 5 * B          # distinct entries of the five valid slots
    assert torch.equal(given, drawn.flip(0))
    warm = warm.cpu().numpy()
    assert len(set(warm.tolist())) == R and warm.min() >= 0 and warm.max() < B              # the warm-up's: slot 0, which play() has not filled again
    want = np.bincount(warm, minlength=8 * B) + 2 * np.bincount(flat, minlength=8 * B)
    assert np.array_equal(play.refreshed.view(-1).cpu().numpy(), want) and want.sum() == 3 * R
    assert "refreshed" in play.sample(8) and play.z[:5].any()
