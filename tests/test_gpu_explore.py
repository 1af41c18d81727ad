"""GPU: self-play's exploration noise from the counter RNG (snac_explore_root_dirichlet / snac_explore_gumbel_scores, k_explore.hip;
snac_explore_pick_moves_temp, k_uct_play.hip; UCTSearch.add_dirichlet_noise / gumbel_scores(t=) / pick_moves(temperature=); SelfPlay(dirichlet=,
temperature=, counter_noise=)) against the numpy statement of the rules of include/snac_hip.h, "Exploration noise"
(tests/test_explore_host.py, which pins that statement on the host).  Byte for byte everywhere: through the C ABI on statistics rows of
random bytes inside guard arenas, so that every byte but the written prior words is seen to stay; through the wrappers on trees a real
search built; a whole play() against the host hook that applies the numpy rule; shards of a batch against the whole; no host
synchronisation; the example."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

from devmem import _raw, _tag
import guard
import helpers
from test_explore_host import (ACTIONS, ALPHAS, bad_rows_of, dirichlet_rule, env_ids_of, gumbel_rule, make_counts, make_priors, make_temps,
                               priors_bad, temp_rule)
from test_gpu_uct_puct import C as CPUCT
from test_gpu_uct_puct import make_evaluator

pytestmark = pytest.mark.gpu

SEED, BASE = (9 << 32) | 11, (1 << 33) + 40                          # a seed and a base with non-zero high words
KIND = {3: 1, 5: 2, 8: 3}
BATCHES = (1, 7, 8, 9, 63, 64, 65, 257)                              # a partial group, the group, the wave's and a block's edges
TS = (0, 1, (1 << 25) + 3)                                           # t * 128 wraps at the last
CAP = 3
PRIOR, VISITS = 48, 8                                                # the first words of prior[] and child_visits[] in a row of 64


def _desc(A, B):
    from snac_amd import _lib

    return _lib.EnvDesc(KIND[A], 1, B, 4, 0, 0, SEED, BASE, 0, 0, 0, 0, 0, 0)


def _stats(arena, rng, B, priors=None, counts=None):
    """Statistics rows of random bytes with the roots' priors / child visits set: (the carved tensor, its numpy copy)."""
    import torch

    rows = B * (CAP + 1)
    host = rng.integers(-(1 << 31), 1 << 31, (rows, 64), dtype=np.int64).astype(np.int32)
    roots = np.arange(B) * CAP
    if priors is not None:
        host[roots, PRIOR:PRIOR + priors.shape[1]] = priors.view(np.int32)
    if counts is not None:
        host[roots, VISITS:VISITS + counts.shape[1]] = counts
    dev = arena.carve((rows, 64), torch.int32, name="stats")
    dev.copy_(torch.from_numpy(host))
    return dev, host


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("A", ACTIONS)
def test_the_noise_kernels_equal_the_rule_byte_for_byte_and_write_nothing_else(A):
    import torch

    from snac_amd import _lib

    L = _lib.lib()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(100 + A)
    for i, B in enumerate(BATCHES):
        t = TS[i % len(TS)]
        env = env_ids_of(BASE, B)
        p = make_priors(rng, B, A, shift=i)
        mask = (np.arange(B) % 5 != 3).astype(np.uint8)
        arena = guard.Arena(B * (CAP + 1) * 256 + B * A * 4 + 8 * (guard.BAND + 4096), dev)
        stats, host = _stats(arena, rng, B, priors=p)
        bad = arena.carve(1, torch.int32, name="bad_rows")
        scores = arena.carve((B, A), torch.float32, name="scores")
        dmask = torch.from_numpy(mask).to(dev)
        d = _desc(A, B)
        roots = np.arange(B) * CAP
        for alpha in ALPHAS:
            for attempts in (1, 16):
                for m, dm in ((None, None), (mask, dmask)):
                    if m is not None and attempts == 1:
                        continue
                    stats.copy_(torch.from_numpy(host))
                    bad.zero_()
                    rc = L.snac_explore_root_dirichlet(C.byref(d), A, _ptr(stats), B * (CAP + 1), B, CAP, _ptr(dm), t, alpha, 0.25, attempts,
                                                       _ptr(bad), None)
                    assert rc == 0, L.snac_last_error()
                    want = dirichlet_rule(SEED, env, t, p, alpha, 0.25, attempts, m)
                    expect = host.copy()
                    expect[roots, PRIOR:PRIOR + A] = want["priors"].view(np.int32)
                    torch.cuda.synchronize()
                    what = (A, B, t, alpha, attempts, m is not None)
                    assert np.array_equal(stats.cpu().numpy(), expect), what     # every byte of stats: the prior words and nothing else
                    assert int(bad.cpu()[0]) == want["bad_rows"] == bad_rows_of(B, i, m), what
                    arena.check()
        # bad rows are untouched (above: their words are the rule's, which keeps them) and there are some; eps = 1 and no counter
        assert priors_bad(p).sum() == bad_rows_of(B, i)
        stats.copy_(torch.from_numpy(host))
        assert L.snac_explore_root_dirichlet(C.byref(d), A, _ptr(stats), B * (CAP + 1), B, CAP, None, t, 2.5, 1.0, 16, None, None) == 0
        expect = host.copy()
        expect[roots, PRIOR:PRIOR + A] = dirichlet_rule(SEED, env, t, p, 2.5, 1.0)["priors"].view(np.int32)
        torch.cuda.synchronize()
        assert np.array_equal(stats.cpu().numpy(), expect), (A, B, "eps 1")
        stats.copy_(torch.from_numpy(host))
        for m, dm in ((None, None), (mask, dmask), (np.zeros(B, np.uint8), torch.zeros(B, dtype=torch.uint8, device=dev))):
            guard.fresh(scores)
            assert L.snac_explore_gumbel_scores(C.byref(d), A, _ptr(stats), B * (CAP + 1), B, CAP, _ptr(dm), t, _ptr(scores), None) == 0
            torch.cuda.synchronize()
            got, want = scores.cpu().numpy(), gumbel_rule(SEED, env, t, p, m)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]), (A, B, t, "gumbel")
            assert np.array_equal(stats.cpu().numpy(), host)         # the statistics are read only
            arena.check()


@pytest.mark.parametrize("A", ACTIONS)
def test_the_temperature_move_equals_the_rule_and_pick_moves_outputs(A):
    import torch

    from snac_amd import _lib

    L = _lib.lib()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(200 + A)
    for i, B in enumerate(BATCHES):
        t = TS[i % len(TS)]
        env = env_ids_of(BASE, B)
        n = make_counts(rng, B, A)
        arena = guard.Arena(B * (CAP + 1) * 256 + 2 * B * (A * 4 + 8) + 12 * (guard.BAND + 4096), dev)
        stats, host = _stats(arena, rng, B, counts=n)
        act, pi, val = (arena.carve(s, dt, name=k) for k, s, dt in (("action", B, torch.int8), ("pi", (B, A), torch.float32),
                                                                    ("value", B, torch.float32)))
        act0, pi0, val0 = (torch.empty_like(x) for x in (act, pi, val))
        d = _desc(A, B)
        head = (C.byref(d), A, _ptr(stats), B * (CAP + 1), B, CAP)
        temps = make_temps(B)
        dtemps = torch.from_numpy(temps).to(dev)
        some = (np.arange(B) % 4 == 1).astype(np.uint8)
        for g, dg in ((None, None), (np.zeros(B, np.uint8), torch.zeros(B, dtype=torch.uint8, device=dev)), (some, torch.from_numpy(some).to(dev))):
            assert L.snac_uct_pick_moves(*head, _ptr(dg), t, _ptr(act0), _ptr(pi0), _ptr(val0), None) == 0
            for T in (temps, 1.0, 0.0, 0.5, 3.0, float("inf")):
                per = isinstance(T, np.ndarray)
                for x in (act, pi, val):
                    guard.fresh(x)
                rc = L.snac_explore_pick_moves_temp(*head, _ptr(dg), t, _ptr(dtemps) if per else None, 1.0 if per else T, _ptr(act), _ptr(pi),
                                                    _ptr(val), None)
                assert rc == 0, L.snac_last_error()
                torch.cuda.synchronize()
                what = (A, B, t, g is not None, None if per else T)
                assert np.array_equal(act.cpu().numpy(), temp_rule(SEED, env, t, n, g, T)), what
                assert torch.equal(pi.view(torch.int32), pi0.view(torch.int32)) and torch.equal(val.view(torch.int32), val0.view(torch.int32)), what
                if not per and T == 1.0:
                    assert torch.equal(act, act0), what              # the integer rule, bit for bit
                arena.check()
        assert np.array_equal(stats.cpu().numpy(), host)             # the statistics are read only
        # only the outputs given are written
        for x in (act, pi, val):
            guard.fresh(x)
        assert L.snac_explore_pick_moves_temp(*head, None, t, None, 0.5, _ptr(act), None, None, None) == 0
        torch.cuda.synchronize()
        guard.view_untouched(pi, "pi")
        guard.view_untouched(val, "value")
        arena.check()


# ---- the wrappers on trees a real search built --------------------------------------------------------------------------------------------
N, SHARDS = 8, ((0, 3), (3, 5))
GAMMA = 0.97
RING = ("obs", "pi", "value", "action", "reward", "done", "move", "z")


def _env(n, off=0, kind=2, **kw):
    """An env of n rows with base BASE + off over the kind's plan table, every plan fulfilled by its first 2 .. 5 bricks and a time limit
    of 6, so that episodes end at different moves."""
    from snac_amd import BatchedDMPEnv

    table = helpers.plan_table(kind, True, _tag(kind, True))
    full = table.reshape((-1, 30) if kind == 1 else (-1, 26, 26))
    env = BatchedDMPEnv(kind, True, n, plans=full, seed=SEED, env_id_base=BASE + off, plan_tb=2 + np.arange(len(full)) % 4, total_step=6,
                        time_gt=True, **kw)
    env.reset()
    return env


def _search(env, K=2, its=6, gumbel=None, cap=48):
    from snac_amd import UCTSearch

    kw = dict(q_normalise=True, gumbel=gumbel) if gumbel else {}
    s = UCTSearch(env, cap, 0, GAMMA, c=CPUCT, max_iterations=(env.total_step + 1) * its, paths=K, virtual_loss=0.5 if K > 1 else 0.0,
                  evaluator=make_evaluator(env.num_actions, False), **kw)
    s.reset()
    return s


@pytest.mark.parametrize("K", [1, 5])
def test_the_wrappers_on_searched_trees(K):
    import torch

    env = _env(N)
    s = _search(env, K, its=8)
    s.run(8)
    A, ids = env.num_actions, env_ids_of(BASE, N)
    # temperature 1 is pick_moves() byte for byte, greedy or sampled; other temperatures follow the rule on the root's visits
    for greedy in (None, False, True, torch.tensor([1, 0] * 4)):
        base = s.pick_moves(greedy=greedy, t=5)
        one = s.pick_moves(greedy=greedy, t=5, temperature=1.0)
        assert all(_raw(a) == _raw(b) for a, b in zip(base, one)), greedy
    visits = s.root_visits().cpu().numpy()
    assert (visits.sum(1) > 0).all() and (visits == 0).any() == (K == 1)
    temps = torch.tensor([0.25, 0.5, 2.0, 0.0, float("inf"), 1.0, float("nan"), 4.0], dtype=torch.float32, device=env.device)
    moves = set()
    for t in range(12):
        for T in (temps, 0.5, 3.0):
            a, pi, v = s.pick_moves(greedy=False, t=t, temperature=T)
            want = temp_rule(SEED, ids, t, visits, np.zeros(N, np.uint8), T.cpu().numpy() if torch.is_tensor(T) else T)
            assert np.array_equal(a.cpu().numpy(), want), (t, T)
            assert _raw(pi) == _raw(base[1]) and _raw(v) == _raw(base[2])
            moves.add(_raw(a))
    assert len(moves) > 6                                            # the counter words and the temperatures decide moves
    # the Dirichlet noise: the roots' prior words by the rule, every other byte of the statistics and every record as before
    before, records, p = s.stats.clone(), s.pool.records.clone(), s.root_priors().cpu().numpy()
    mask = torch.tensor([1, 1, 0, 1, 1, 1, 0, 1], device=env.device)
    s.add_dirichlet_noise(0.3, 0.25, t=9, mask=mask)
    want = dirichlet_rule(SEED, ids, 9, p, 0.3, 0.25, 16, mask.cpu().numpy())
    assert want["bad_rows"] == 0 and want["drew"].sum() == 6 * A
    assert np.array_equal(s.root_priors().cpu().numpy().view(np.int32), want["priors"].view(np.int32))
    after = s.stats.clone()
    roots = s._roots
    after[roots, PRIOR:PRIOR + A] = before[roots, PRIOR:PRIOR + A]
    assert torch.equal(after, before) and torch.equal(s.pool.records, records)
    assert int(s.noise_bad_rows.cpu()[0]) == 0
    s.set_root_priors(torch.tensor([[0.5, float("nan")] + [0.1] * (A - 2)] * 2 + [[0.2] * A] * (N - 2)))
    s.add_dirichlet_noise(1.0, 0.5, t=10)
    assert int(s.noise_bad_rows.cpu()[0]) == 2 and torch.isnan(s.root_priors()[:2, 1]).all()


def test_the_gumbel_scores_of_a_search_by_the_counter_rng():
    import torch

    env = _env(N)
    s = _search(env, 2, gumbel=4)
    ids, p = env_ids_of(BASE, N), s.root_priors().cpu().numpy()
    before = s.stats.clone()
    for noise, m in ((True, None), (False, np.zeros(N)), (torch.tensor([1, 0, 0, 1, 1, 0, 1, 1], device=env.device).view(N, 1) != 0, None)):
        got = s.gumbel_scores(noise, t=(1 << 25) + 3).cpu().numpy()
        m = noise.cpu().numpy().reshape(-1) if torch.is_tensor(noise) else m
        assert np.array_equal(got.view(np.int32), gumbel_rule(SEED, ids, (1 << 25) + 3, p, m).view(np.int32))
    assert torch.equal(s.stats, before)
    plain = s.gumbel_scores(False)                                   # the torch path is as it was: log of the priors in float32
    assert torch.allclose(plain, s.gumbel_scores(False, t=0), atol=1e-6)
    s.gumbel_begin(s.gumbel_scores(t=3))
    s.gumbel_run(6)
    assert bool((s.cand.cpu() != 0).all())


# ---- play() -----------------------------------------------------------------------------------------------------------------------------------
def _play(env, its=6, moves=9, K=2, m=None, **kw):
    """A SelfPlay(**kw) over a fresh search of env (m: a Gumbel search over m candidates) after `moves` moves and targets()."""
    import torch

    from snac_amd import SelfPlay

    play = SelfPlay(_search(env, K, its, m), capacity_moves=8, sample_moves=3, **kw)
    play.play(moves, iterations=its)
    play.targets()
    torch.cuda.synchronize()
    return play


def _same_rings(a, b, cols=slice(None)):
    for name in RING:
        assert _raw(getattr(a, name)) == _raw(getattr(b, name)[:, cols]), name


def test_play_with_dirichlet_noise_fills_the_ring_as_the_host_hook_with_the_numpy_rule_does():
    import torch

    dev_play = _play(_env(N), dirichlet=(0.3, 0.25))
    env = _env(N)
    box, calls = {}, []

    def hook(p):
        play = box["play"]
        calls.append(play.moves)
        want = dirichlet_rule(SEED, env_ids_of(BASE, N), play.moves, p.cpu().numpy(), 0.3, 0.25)
        return torch.from_numpy(want["priors"]).to(p.device)

    from snac_amd import SelfPlay

    host_play = box["play"] = SelfPlay(_search(env), capacity_moves=8, sample_moves=3, root_noise=hook)
    host_play.play(9, iterations=6)
    host_play.targets()
    torch.cuda.synchronize()
    assert calls == list(range(9))
    _same_rings(dev_play, host_play)
    assert torch.equal(dev_play.search.stats[dev_play.search._roots], host_play.search.stats[host_play.search._roots])
    assert int(dev_play.search.noise_bad_rows.cpu()[0]) == 0
    done = dev_play.done.cpu().numpy() != 0
    assert done.any() and not done.all() and dev_play.head == 1      # episodes ended, the ring wrapped
    plain = _play(_env(N))
    assert _raw(plain.pi) != _raw(dev_play.pi)                       # the noise changed the searches


def test_play_with_temperature_one_is_the_default_play():
    plain, one, half = _play(_env(N)), _play(_env(N), temperature=1.0), _play(_env(N), temperature=0.25)
    _same_rings(one, plain)
    assert _raw(half.action) != _raw(plain.action)


@pytest.mark.parametrize("mode", ["puct", "gumbel"])
def test_sharded_play_with_counter_noise_is_the_whole_play(mode):
    kw = dict(dirichlet=(0.3, 0.25), temperature=0.5) if mode == "puct" else dict(gumbel=True, counter_noise=True)
    g = 4 if mode == "gumbel" else None
    whole = _play(_env(N), m=g, **kw)
    assert (whole.done.cpu().numpy() != 0).any() and whole.z.any() and (whole.action.cpu().numpy() != 0).any()
    for off, n in SHARDS:
        shard = _play(_env(n, off), m=g, **kw)
        _same_rings(shard, whole, slice(off, off + n))


@pytest.mark.parametrize("mode", ["puct", "gumbel"])
def test_play_with_the_new_keywords_does_not_synchronise_with_the_host(mode):
    import torch

    from snac_amd import SelfPlay

    kw = dict(dirichlet=(0.3, 0.25), temperature=0.5) if mode == "puct" else dict(gumbel=True, counter_noise=True)
    play = SelfPlay(_search(_env(64), 2, 3, 4 if mode == "gumbel" else None), 8, sample_moves=2, **kw)
    play.play(1, 3)                                                  # warm-up
    play.targets()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        play.play(4, 3)
        play.targets()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert play.moves == 5 and play.search.iterations == 15 and bool(((play.pi[:5].sum(2) - 1).abs() < 1e-5).all())


def test_the_example_runs_with_the_new_flags():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "alphazero_selfplay.py")
    spec = importlib.util.spec_from_file_location("alphazero_selfplay", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    small = dict(kind=2, envs=32, steps=3, moves=3, iterations=4, paths=2, nodes=64, batch=64, capacity=8)
    for kw in (dict(dirichlet=0.3, temperature=0.5), dict(gumbel=4, counter_noise=True)):
        losses, play = mod.train(**small, **kw)
        assert len(losses) == 3 and all(math.isfinite(x) for x in losses), kw
        assert play.moves == 9 and bool(((play.pi.sum(2) - 1).abs() < 1e-5).all()) and bool(play.z.isfinite().all())
        assert (play.dirichlet, play.temperature, play.counter_noise) == (((0.3, 0.25), 0.5, False) if "dirichlet" in kw else (None, None, True))
