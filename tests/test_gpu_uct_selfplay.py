"""GPU: self-play on the device (UCTSearch.pick_moves / restart, SelfPlay; snac_uct_pick_moves / snac_uct_restart / snac_uct_returns,
k_uct_play.hip) against a restatement in numpy of the rules of include/snac_hip.h ("Self-play"), on top of the restatements of the
rollout search (tests/test_gpu_uct_paths.py) and of PUCT (tests/test_gpu_uct_puct.py).

The rules, restated.  pick: N_a = the visits of the root's child a (0 where untried), total = their sum; pi = float32(N_a / total) in
float64, value = float32(W / N) of the root, both 0 without visits; the move is 0 without child visits, the lowest argmax of N where
greedy, else with w = word(seed, 3, env_id_base + b, t) and u = (w * total) >> 32 the lowest a whose running sum of N passes u.
restart: a masked tree becomes one node, the record of its env row, with fresh statistics (terminal = the record's NEED_RESET; PUCT: the
evaluator's priors); every other tree keeps every byte.  returns: from the newest slot back, g = reward + (done ? 0 : gamma * g) in
float64, z = float32(g).  Every comparison is bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

from devmem import _env
import rng_spec
from test_gpu_uct import NON_DEFAULT, NON_DEFAULT_SEED
from test_gpu_uct_paths import H, KINDS, Restatement
from test_gpu_uct_paths import _same as _same_rollout
from test_gpu_uct_puct import C as CPUCT
from test_gpu_uct_puct import GAMMA, HIGH, VL, PuctRestatement, make_evaluator
from test_gpu_uct_puct import _same as _same_puct

pytestmark = pytest.mark.gpu

STREAM_PICK = 3


# ---- the restatements -----------------------------------------------------------------------------------------------------------------
def pick(ref, greedy, t):
    """(action int8 [B], pi float32 [B, A], value float32 [B]) of ref's roots."""
    B, cap, env = ref.B, ref.cap, ref.env
    roots = np.arange(B) * cap
    ch = ref.child[roots]
    N = np.where(ch >= 0, ref.visits[np.maximum(ch, 0)], 0).astype(np.uint64)
    total = N.sum(1)
    has = total > 0
    pi = np.zeros((B, ref.A), np.float32)
    pi[has] = (N[has].astype(np.float64) / total[has, None].astype(np.float64)).astype(np.float32)
    v = ref.visits[roots]
    value = np.zeros(B, np.float32)
    value[v > 0] = (ref.W[roots][v > 0] / v[v > 0].astype(np.float64)).astype(np.float32)
    w = rng_spec.words(env.seed, STREAM_PICK, np.uint64(env.env_id_base) + np.arange(B, dtype=np.uint64), t)
    u = (w * total) >> np.uint64(32)
    sampled = (np.cumsum(N, 1) <= u[:, None]).sum(1)
    g = np.broadcast_to(np.asarray(greedy, bool), (B,))
    action = np.where(has, np.where(g, np.argmax(N, 1), sampled), 0).astype(np.int8)
    return action, pi, value


def restart(ref, mask, rows=None):
    """ref's masked trees <- env rows (of ref.env), as reset() makes a root; PUCT: then the priming of the unvisited roots."""
    import torch

    B, cap, dev = ref.B, ref.cap, ref.env.device
    rows = torch.arange(B, device=dev) if rows is None else torch.as_tensor(rows, device=dev)
    ref.pool.load(rows=rows, node_rows=B * cap + torch.arange(B, device=dev))
    idx = np.nonzero(np.asarray(mask))[0]
    if len(idx):
        roots = torch.as_tensor(idx * cap, device=dev)
        ref.pool.load(rows=rows[torch.as_tensor(idx, device=dev)], node_rows=roots)
        nr = ref.pool.need_reset[roots].cpu().numpy()
        for j, b in enumerate(idx):
            base = int(b) * cap
            ref._clear(base, base + cap)
            ref.terminal[base] = nr[j]
            ref.used[b] = 1
            if hasattr(ref, "prior"):
                ref.prior[base:base + cap] = 0
    if hasattr(ref, "prime_roots"):
        ref.prime_roots()


def returns(reward, done, first, count, gamma, bootstrap, z):
    """z's `count` slots from `first` on (modulo the ring), in place."""
    cap, B = reward.shape
    g = np.zeros(B, np.float64) if bootstrap is None else bootstrap.astype(np.float64)
    for i in range(count - 1, -1, -1):
        s = (first + i) % cap
        t = np.float64(gamma) * g
        g = reward[s].astype(np.float64) + np.where(done[s] != 0, 0.0, t)
        z[s] = g.astype(np.float32)
    return z


def _pair(kind, dyn, B, seed, cap, K, puct, budget, fpv=None, prep=None, twin=False, **env_kw):
    """(search, ref, env): a device search after reset() and its restatement; twin: the restatement on a second env made the same way
    (a whole play() resets env rows, and the restatement follows move by move afterwards)."""
    from snac_amd import UCTSearch

    envs = [_env(kind, dyn, B, seed, **env_kw) for _ in range(2 if twin else 1)]
    for e in envs:
        if prep is not None:
            prep(e)
    env, renv = envs[0], envs[-1]
    if puct:
        fn = make_evaluator(env.num_actions, False)
        search = UCTSearch(env, cap, 0, GAMMA, c=CPUCT, max_iterations=budget, paths=K, virtual_loss=VL, evaluator=fn, first_play_value=fpv)
        search.reset()
        ref = PuctRestatement(renv, B, cap, K, VL, 0, GAMMA, CPUCT, fn, 0.0 if fpv is None else fpv, budget)
    else:
        hz = H[kind] // 8
        search = UCTSearch(env, cap, hz, GAMMA, max_iterations=budget, paths=K, virtual_loss=VL)
        search.reset()
        ref = Restatement(renv, B, cap, K, VL, hz, GAMMA, math.sqrt(2))
    return search, ref, env


def _same(search, ref, live_only=False):
    (_same_puct if search.evaluator is not None else _same_rollout)(search, ref, live_only=live_only)


def _near_the_end(kind, dyn, terminal_roots=False, total_step=None):
    """count_step of rows 0::3 / 1::3 one / three steps before the time limit (total_step: the env's own, where it is not the kind's):
    their episodes end at the first / third move, one move later under time_gt."""
    import torch

    from snac_amd import _lib

    ts = _lib.env_sizes(kind, dyn).total_step if total_step is None else total_step

    def prep(env):
        B = env.num_envs
        cs = env._hdr.view(torch.int16).view(B, 8)[:, 3]
        cs[0::3] = ts - 1
        cs[1::3] = ts - 3
        if terminal_roots:
            env._hdr.view(torch.int8).view(B, 16)[2::9, 2] |= _lib.FLAG_NEED_RESET
    return prep


def _run_both(search, ref, n):
    search._run(n)
    for _ in range(n):
        ref.iteration()


def _bytes(t):
    return t.cpu().numpy().tobytes()


# ---- 1. pick_moves ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("puct", [False, True])
@pytest.mark.parametrize("kind,dyn", KINDS)
def test_pick_moves_equals_the_restatement(kind, dyn, puct, K):
    import torch

    B, cap, its = 24, 40, 12
    # PUCT with a high first-play value tries every root action first: every live root has several visited children
    def terminal_roots(e):
        e._hdr.view(torch.int8).view(B, 16)[2::9, 2] |= 1            # NEED_RESET: roots 2::9 are terminal

    search, ref, env = _pair(kind, dyn, B, 3 + kind + dyn, cap, K, puct, its, fpv=HIGH if puct else None, prep=terminal_roots)
    A = env.num_actions
    _run_both(search, ref, its)
    _same(search, ref)
    mixed = np.arange(B) % 3 == 0
    # the inputs first: two move counters whose sampled moves differ from the argmax and from each other somewhere
    arg = pick(ref, True, 0)[0]
    ts = [t for t in range(64) if (pick(ref, False, t)[0] != arg).any()][:1]
    ts += [t for t in range(ts[0] + 1, 128) if (pick(ref, False, t)[0] != pick(ref, False, ts[0])[0]).any()][:1]
    assert len(ts) == 2
    for t in ts:
        assert np.array_equal(pick(ref, True, t)[0], arg)            # the argmax does not read the counter
    dead = np.zeros(B, bool)
    dead[2::9] = True
    assert (ref.terminal[np.arange(B) * cap] == dead).all() and dead.any()
    for t in ts:
        for greedy, flags in ((None, True), (True, True), (False, False), (torch.as_tensor(mixed, device=env.device), mixed),
                              (torch.as_tensor(mixed.astype(np.uint8)), mixed)):
            a, pi, v = search.pick_moves(greedy=greedy, t=t)
            wa, wpi, wv = pick(ref, flags, t)
            assert a.dtype == torch.int8 and tuple(pi.shape) == (B, A) and pi.dtype == torch.float32 and v.dtype == torch.float32
            assert np.array_equal(a.cpu().numpy(), wa), (t, greedy)
            assert _bytes(pi) == wpi.tobytes() and _bytes(v) == wv.tobytes()
            assert not a.cpu().numpy()[dead].any() and not pi.cpu().numpy()[dead].any()      # no child visits: action 0, pi 0
    assert np.array_equal(search.pick_moves()[0].cpu().numpy(), search.best_actions().cpu().numpy())
    live = ~dead
    s = pick(ref, True, 0)[1][live].astype(np.float64).sum(1)
    assert np.abs(s - 1.0).max() <= A * 2.0 ** -24                   # float32 roundings of A quotients that sum to 1
    out = (torch.full((B,), 9, dtype=torch.int8, device=env.device), torch.full((B, A), 9.0, dtype=torch.float32, device=env.device),
           torch.full((B,), 9.0, dtype=torch.float32, device=env.device))
    got = search.pick_moves(greedy=False, t=ts[1], out=out)
    wa, wpi, wv = pick(ref, False, ts[1])
    assert all(x is y for x, y in zip(got, out))
    assert np.array_equal(out[0].cpu().numpy(), wa) and _bytes(out[1]) == wpi.tobytes() and _bytes(out[2]) == wv.tobytes()
    _same(search, ref)                                               # the statistics are read only


@pytest.mark.parametrize("puct", [False, True])
def test_pick_moves_before_any_iteration(puct):
    B = 16
    search, ref, env = _pair(2, True, B, 5, 8, 2, puct, 4)
    search.run(0)
    for greedy in (True, False):
        a, pi, v = search.pick_moves(greedy=greedy, t=7)
        assert not a.cpu().numpy().any() and not pi.cpu().numpy().any() and not v.cpu().numpy().any()
        wa, wpi, wv = pick(ref, greedy, 7)
        assert not wa.any() and not wpi.any() and not wv.any()


# ---- 2. restart ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dyn,K,puct", [(1, False, 1, False), (2, True, 5, False), (3, True, 3, False), (1, True, 4, True), (2, False, 1, True),
                                             (3, False, 5, True)])
def test_restart_with_a_mixed_mask(kind, dyn, K, puct):
    import torch

    from snac_amd import UCTSearch

    B, cap, n = 12, 48, 8
    search, ref, env = _pair(kind, dyn, B, 23 + kind, cap, K, puct, 3 * n)
    A = env.num_actions
    _run_both(search, ref, n)
    _same(search, ref)
    mask = np.arange(B) % 3 != 1
    mask[0] = False
    env.rollout(5, obs=None)                                         # the env rows move on: new roots that differ from the old ones
    rows = (torch.arange(B, device=env.device) + 3) % B
    env._hdr.view(torch.int8).view(B, 16)[8, 2] |= 1                  # the row of masked tree 5 needs a reset: a terminal new root
    assert mask[5] and mask[2] and int(rows[5]) == 8
    torch.cuda.synchronize()
    stats, records, used = search.stats.clone(), search.pool.records.clone(), search.tree_sizes()
    search.restart(torch.as_tensor(mask, device=env.device), rows=rows)
    restart(ref, mask, rows)
    torch.cuda.synchronize()
    if puct:
        fresh = UCTSearch(env, cap, 0, GAMMA, c=CPUCT, max_iterations=3 * n, paths=K, virtual_loss=VL, evaluator=search.evaluator)
    else:
        fresh = UCTSearch(env, cap, H[kind] // 8, GAMMA, max_iterations=3 * n, paths=K, virtual_loss=VL)
    fresh.reset(rows=rows)
    torch.cuda.synchronize()
    now_used = search.tree_sizes()
    for b in range(B):
        lo, hi = b * cap, (b + 1) * cap
        if mask[b]:                                                  # what reset() makes of the same env row
            assert torch.equal(search.stats[lo], fresh.stats[lo]) and torch.equal(search.pool.records[lo], fresh.pool.records[lo])
            assert int(now_used[b]) == 1
        else:                                                        # every byte kept
            assert torch.equal(search.stats[lo:hi], stats[lo:hi]) and torch.equal(search.pool.records[lo:hi], records[lo:hi])
            assert int(now_used[b]) == int(used[b]) and int(used[b]) > 1
    need = (env._hdr.view(torch.int8).view(B, 16)[:, 2] & 1).bool()[rows].cpu().numpy()      # a new root is terminal iff its env row needs a reset
    term = search.terminal[torch.arange(B, device=env.device) * cap].cpu().numpy()
    assert np.array_equal(term[mask], need[mask]) and term[5] and not term[mask].all()
    if puct:
        assert search.root_priors()[torch.as_tensor(mask, device=env.device)].any()
    _same(search, ref, live_only=True)
    for chunk in (3, n - 3):
        _run_both(search, ref, chunk)
        _same(search, ref, live_only=True)
    assert search.iterations == 2 * n                                # not reset


# ---- 3. the whole loop ------------------------------------------------------------------------------------------------------------------
def _play_move_by_move(kind, dyn, puct, seed, **env_kw):
    import torch

    from snac_amd import SelfPlay, _lib

    B, cap, K, its, moves, slots, sample_moves = 12, 48, 3, 4, 7, 5, 2
    ts = _lib.env_sizes(kind, dyn).total_step
    prep = _near_the_end(kind, dyn, total_step=env_kw.get("total_step"))
    search, ref, env = _pair(kind, dyn, B, seed, cap, K, puct, (ts + 1) * its, prep=prep, twin=True, **env_kw)
    renv, A = ref.env, env.num_actions
    play = SelfPlay(search, slots, sample_moves=sample_moves)
    play.play(3, its)
    play.play(moves - 3, its)
    torch.cuda.synchronize()
    assert play.moves == moves and play.head == moves % slots and play.valid_moves() == slots and len(play) == slots * B

    want = dict(obs=[None] * slots, pi=np.zeros((slots, B, A), np.float32), value=np.zeros((slots, B), np.float32),
                action=np.zeros((slots, B), np.int8), reward=np.zeros((slots, B), np.float32), done=np.zeros((slots, B), np.uint8),
                move=np.zeros((slots, B), np.int32))
    in_episode = np.zeros(B, np.int64)
    restarts = np.zeros(B, np.int64)
    sampled_differs = False
    roots = torch.arange(B, device=env.device) * cap
    for mv in range(moves):
        for _ in range(its):
            ref.iteration()
        s = mv % slots
        want["obs"][s] = ref.pool.observe(roots)
        greedy = in_episode >= sample_moves
        a, pi, v = pick(ref, greedy, mv)
        sampled_differs |= bool((a != pick(ref, True, mv)[0]).any())
        r, d = ref.advance(a)
        want["pi"][s], want["value"][s], want["action"][s], want["reward"][s], want["done"][s], want["move"][s] = pi, v, a, r, d, in_episode
        renv.reset(mask=torch.as_tensor(d, device=env.device), want_obs=False)
        restart(ref, d)
        restarts += d
        in_episode = np.where(d, 0, in_episode + 1)
    assert (restarts > 0).any() and (restarts == 0).any() and restarts.max() >= 1 and sampled_differs      # the inputs
    for s in range(slots):
        assert torch.equal(play.obs[s], want["obs"][s]), s
    for k in ("pi", "value", "action", "reward", "done", "move"):
        assert _bytes(getattr(play, k)) == want[k].tobytes(), k
    assert not play.z.any()                                          # targets() was not called
    assert np.array_equal(play._move.cpu().numpy(), in_episode)
    _same(search, ref, live_only=True)
    assert torch.equal(env._episode, renv._episode) and torch.equal(env._hdr, renv._hdr)
    episode = env._episode.cpu().numpy()
    assert np.array_equal(episode, restarts)                         # episode 0 by the first reset, one more per restart
    if dyn:                                                          # the restarted trees play the plan the counter RNG gives their next episode
        ids = np.uint64(env.env_id_base) + np.arange(B, dtype=np.uint64)
        plan = rng_spec.plan_of(rng_spec.words(env.seed, rng_spec.STREAM_PLAN, ids, episode.astype(np.uint64)), env.num_plans)
        got = search.pool.plan_idx[roots].cpu().numpy()
        assert np.array_equal(got[restarts > 0], plan[restarts > 0])


@pytest.mark.parametrize("puct", [False, True])
@pytest.mark.parametrize("kind,dyn", [(1, False), (2, True), (3, True)])
def test_play_equals_the_restatement_move_by_move(kind, dyn, puct):
    _play_move_by_move(kind, dyn, puct, 37 + kind)


@pytest.mark.parametrize("kind,dyn,puct", [(2, True, True)])
def test_play_on_a_non_default_env_equals_the_restatement_move_by_move(kind, dyn, puct):
    """env_id_base 1000, a 64-bit seed, brick_gt / time_gt, total_step 9 and an action distribution: sampled moves and the restarted trees'
    plans are keyed by 1000 + b, the slots of the K = 3 paths from 1000 * K."""
    _play_move_by_move(kind, dyn, puct, NON_DEFAULT_SEED, **NON_DEFAULT)


def test_play_with_root_noise_and_a_sample():
    import torch

    from snac_amd import SelfPlay, _lib

    B, its = 32, 3
    ts = _lib.env_sizes(2, True).total_step
    search, ref, env = _pair(2, True, B, 9, 32, 2, True, (ts + 1) * its, prep=_near_the_end(2, True))
    A = env.num_actions
    calls = []

    def noise(p):
        calls.append(tuple(p.shape))
        return 0.75 * p + 0.25 / A

    play = SelfPlay(search, 6, sample_moves=1, root_noise=noise)
    play.play(4, its)
    play.targets()
    torch.cuda.synchronize()
    assert calls == [(B, A)] * 4 and play.valid_moves() == 4 and len(play) == 4 * B
    assert play.slots().tolist() == [0, 1, 2, 3]
    g = torch.Generator(device=env.device).manual_seed(1)
    batch = play.sample(50, generator=g)
    assert tuple(batch["obs"].shape) == (50, env.obs_dim) and batch["obs"].dtype == torch.float32
    assert tuple(batch["pi"].shape) == (50, A) and batch["action"].dtype == torch.int64 and batch["done"].dtype == torch.bool
    for k in ("z", "value", "reward"):
        assert tuple(batch[k].shape) == (50,) and batch[k].dtype == torch.float32
    flat_pi = play.pi[:4].reshape(-1, A)
    assert all((flat_pi == row).all(1).any() for row in batch["pi"])    # every sampled row is a row of the valid slots
    with pytest.raises(ValueError):
        SelfPlay(search, 6).play(1, its + 1)                          # the budget: (total_step + 1) * iterations


# ---- 4. targets ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moves", [4, 6, 9])
def test_targets_equal_the_recurrence(moves):
    """Random rewards and dones written into the ring: 4 moves leave two of six slots outside the valid range, 9 wrap the ring."""
    import torch

    from snac_amd import SelfPlay

    B, slots = 70, 6                                                 # two waves, the second partly filled
    search, ref, env = _pair(2, True, B, 13, 16, 2, False, 8)
    _run_both(search, ref, 5)
    play = SelfPlay(search, slots, gamma=0.9)
    rng = np.random.default_rng(moves)
    reward = (rng.integers(-100, 11, size=(slots, B)) + rng.random((slots, B))).astype(np.float32)
    done = (rng.random((slots, B)) < 0.3).astype(np.uint8)
    play.reward.copy_(torch.as_tensor(reward))
    play.done.copy_(torch.as_tensor(done))
    play.moves, play.head = moves, moves % slots
    valid = min(moves, slots)
    first = (play.head - valid) % slots
    boot = pick(ref, True, 0)[2]
    assert boot.any() and done.any() and not done.all()
    for bootstrap in (False, True):
        play.z.fill_(-7.5)
        z = play.targets(bootstrap=bootstrap)
        torch.cuda.synchronize()
        want = returns(reward, done, first, valid, 0.9, boot if bootstrap else None, np.full((slots, B), -7.5, np.float32))
        assert z is play.z and _bytes(z) == want.tobytes(), bootstrap
        if moves < slots:
            assert (want[moves:] == -7.5).all()
    newest = (play.head - 1) % slots
    carried = (done[newest] == 0) & (boot != 0)
    assert carried.any() and (want[newest][carried] != reward[newest][carried]).any()      # the bootstrap entered


def test_returns_over_a_part_of_the_ring():
    """The entry point itself, a window that wraps: slots 4, 5, 0, 1 of six; 2 and 3 keep the sentinel."""
    import torch

    from snac_amd import _lib

    B, slots, gamma = 130, 6, 0.97
    dev = torch.device("cuda")
    rng = np.random.default_rng(3)
    reward = rng.normal(size=(slots, B)).astype(np.float32)
    done = (rng.random((slots, B)) < 0.25).astype(np.uint8)
    boot = rng.normal(size=B).astype(np.float32)
    r, d, bt = (torch.as_tensor(x, device=dev) for x in (reward, done, boot))
    z = torch.full((slots, B), 3.25, dtype=torch.float32, device=dev)
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(L.snac_uct_returns(B, slots, 4, 4, gamma, p(r), p(d), p(bt), p(z), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    want = returns(reward, done, 4, 4, gamma, boot, np.full((slots, B), 3.25, np.float32))
    assert _bytes(z) == want.tobytes() and (want[2:4] == 3.25).all() and (want[[4, 5, 0, 1]] != 3.25).any()
    _lib.check(L.snac_uct_returns(B, slots, 2, 1, gamma, p(r), p(d), None, p(z), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    want = returns(reward, done, 2, 1, gamma, None, want)
    assert _bytes(z) == want.tobytes() and want[2].tobytes() == reward[2].tobytes()


# ---- 5. no host synchronisation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("puct", [False, True])
def test_play_does_not_synchronise_with_the_host(puct):
    import torch

    from snac_amd import SelfPlay, _lib

    B, its = 64, 3
    ts = _lib.env_sizes(2, True).total_step
    search, ref, env = _pair(2, True, B, 3, 64, 4, puct, (ts + 1) * its, prep=_near_the_end(2, True))
    play = SelfPlay(search, 8, sample_moves=2)
    play.play(1, its)                                                # warm-up: rows 0::3 end here
    play.targets()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        play.play(4, its)                                            # rows 1::3 end at the third move of their episode
        play.targets()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    done = play.done.cpu().numpy()[:5]
    assert done[0, 0::3].all() and done[1:, 1::3].any() and not done[:, 2::3].all()
    assert play.moves == 5 and search.iterations == 5 * its
    assert (play.move.cpu().numpy()[:5].max(0) >= 1).all()
