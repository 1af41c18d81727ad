"""GPU: the search stack does not depend on how the envs are sharded (include/snac_hip.h: "env = env_id_base + local index, so results do
not depend on how envs are sharded over GPUs"): UCTSearch (run, paths=K, PUCT, pick_moves, advance, restart) and SelfPlay on shards of a
batch against the same search on the whole batch.

The reference is the unsharded run: N = 12 env rows with env_id_base 40 (the whole has a non-zero base itself) and a seed with a non-zero
high word, split unevenly into shards of 5 and 7 rows with bases 40 and 45 -- another B, another pool, other launch shapes.  Tree b of the
shard with base E is tree E - 40 + b of the whole: its statistics (child and parent rows rebased to the tree's first row), its records,
its moves and its ring entries must be the whole's bit for bit.  No tolerance anywhere.

The counter words that this pins: edges and leaves of iteration `it` are keyed by ((env_id_base + b) * K + k, it * (H + 1) [+ 1 + t]), the
move's edge of advance() by (env_id_base + b, it * (H + 1)), a sampled move by stream 3 and (env_id_base + b, t), the plan of a restarted
tree by stream 1 and (env_id_base + b, episode)."""
import numpy as np
import pytest

from devmem import _raw, _tag
import helpers
import rng_spec
from test_gpu_uct_puct import C as CPUCT
from test_gpu_uct_puct import make_evaluator

pytestmark = pytest.mark.gpu

N, BASE = 12, 40
SHARDS = ((0, 5), (5, 7))                                            # (first row in the whole, rows): bases 40 and 45
SEED = (5 << 32) | 7
CAP, HZ, GAMMA, VL = 64, 20, 0.97, 0.5
KINDS = [(1, False), (2, True), (3, True)]
PATHS = [1, 4]
STREAM_PICK = 3
FIELDS = ("children", "parent", "action", "reward", "terminal", "visits", "value_sum", "tree_sizes", "records", "root_visits", "root_q",
          "root_priors", "prior")


def _same_env_rows(shard, whole, off):
    import torch

    n = shard.num_envs
    for name in ("_hdr", "_episode", "_grid", "plan_idx"):
        assert torch.equal(getattr(shard, name), getattr(whole, name)[off:off + n]), (name, off)


def _envs(kind, dyn, few_bricks=False, **kw):
    """(whole, [(off, shard)]): the same plan table, seed and options, each reset() from the counter RNG.  few_bricks: every plan row is
    fulfilled by its first 2 .. 5 bricks (plan_tb), so that episodes end at different moves."""
    from snac_amd import BatchedDMPEnv

    table = helpers.plan_table(kind, dyn, _tag(kind, dyn))
    full = table.reshape((-1, 30) if kind == 1 else (-1, 26, 26))
    if few_bricks:
        kw["plan_tb"] = 2 + np.arange(len(full)) % 4
    envs = [BatchedDMPEnv(kind, dyn, n, plans=full, seed=SEED, env_id_base=BASE + off, **kw) for off, n in ((0, N),) + SHARDS]
    for e in envs:
        e.reset()
    whole, shards = envs[0], [(off, e) for (off, _), e in zip(SHARDS, envs[1:])]
    for off, e in shards:                                            # the precondition (tests/test_gpu_parity.py has the env paths)
        _same_env_rows(e, whole, off)
    return whole, shards


def _near_the_end(env, off):
    """Rows with global index 0 mod 3 / 1 mod 3 one / two steps before the time limit: their children / grandchildren are terminal."""
    import torch

    g = off + torch.arange(env.num_envs, device=env.device)
    cs = env._hdr.view(torch.int16).view(env.num_envs, 8)[:, 3]
    cs[g % 3 == 0] = env.total_step - 1
    cs[g % 3 == 1] = env.total_step - 2


def _search(env, K, puct, budget):
    from snac_amd import UCTSearch

    kw = dict(c=CPUCT, evaluator=make_evaluator(env.num_actions, False)) if puct else {}
    search = UCTSearch(env, nodes_per_tree=CAP, horizon=HZ, gamma=GAMMA, max_iterations=budget, paths=K, virtual_loss=VL if K > 1 else 0.0,
                       **kw)
    search.reset()
    return search


def _bits(x):
    """Floats as the integers of their bytes (NaN compares equal to itself); everything else as it is."""
    x = np.ascontiguousarray(x)
    return x.view({4: np.int32, 8: np.int64}[x.itemsize]) if x.dtype.kind == "f" else x


def _trees(search, first, n, live_only):
    """Trees [first, first + n) of a search, every row index rebased to its tree's first row: {field: [n, ...]}.  live_only: rows
    [used, cap) of each tree are blanked (after advance() / restart() they are unspecified)."""
    import torch

    torch.cuda.synchronize()
    cap = search.nodes_per_tree
    lo, hi = first * cap, (first + n) * cap
    base = ((first + np.arange(n)) * cap)[:, None]
    used = search.tree_sizes().cpu().numpy()[first:first + n]

    def rows(t):
        a = _bits(t[lo:hi].cpu().numpy())
        return a.reshape((n, cap) + a.shape[1:])

    def rebased(t):
        a = rows(t).astype(np.int64)
        return np.where(a >= 0, a - base.reshape((n, 1) + (1,) * (a.ndim - 2)), a)

    out = dict(children=rebased(search.children), parent=rebased(search.parent), action=rows(search.action), reward=rows(search.reward),
               terminal=rows(search.terminal), visits=rows(search.visits), value_sum=rows(search.value_sum), prior=rows(search.prior),
               records=rows(search.pool.records))
    if live_only:
        dead = np.arange(cap)[None, :] >= used[:, None]
        for a in out.values():
            a[dead] = 0
    out.update(tree_sizes=used, root_visits=search.root_visits().cpu().numpy()[first:first + n],
               root_q=_bits(search.root_q().cpu().numpy()[first:first + n]),
               root_priors=_bits(search.root_priors().cpu().numpy()[first:first + n]))
    return out


def _same_trees(shard, whole, off, live_only=False):
    """Tree b of the shard is tree off + b of the whole in every field."""
    n = shard.trees
    got, want = _trees(shard, 0, n, live_only), _trees(whole, off, n, live_only)
    for name in FIELDS:
        a, b = got[name], want[name]
        assert a.shape == b.shape and a.dtype == b.dtype, name
        differs = [i for i in range(n) if not np.array_equal(a[i], b[i])]
        assert not differs, "%s: trees %s of the shard with base %d differ from the whole's" % (name, differs, shard.env.env_id_base)


def _not_vacuous(whole):
    """At least one tree reached a terminal node below its root, and the trees over full episodes differ from each other."""
    t = _trees(whole, 0, N, False)
    assert t["terminal"][:, 1:].any()
    full = range(2, N, 3)
    assert len({t["children"][g].tobytes() + t["visits"][g].tobytes() + t["value_sum"][g].tobytes() for g in full}) > 1
    assert (t["tree_sizes"] > 1).all()


def _run(kind, dyn, K, puct, chunks, **kw):
    """(whole search, [(off, shard search)]) after reset() and run(chunk) for every chunk; the budget leaves 16 iterations."""
    whole, shards = _envs(kind, dyn, **kw)
    _near_the_end(whole, 0)
    for off, e in shards:
        _near_the_end(e, off)
        _same_env_rows(e, whole, off)
    budget = sum(chunks) + 16
    searches = [_search(whole, K, puct, budget)] + [_search(e, K, puct, budget) for _, e in shards]
    for s in searches:
        for n in chunks:
            s.run(n)
    return searches[0], [(off, s) for (off, _), s in zip(shards, searches[1:])]


def _sampled(search, t):
    """The move pick_moves(greedy=False, t) draws, from the root visits and the host's counter words (include/snac_hip.h, "Self-play")."""
    env, B = search.env, search.trees
    visits = search.root_visits().cpu().numpy().astype(np.uint64)
    total = visits.sum(1)
    w = rng_spec.words(env.seed, STREAM_PICK, np.uint64(env.env_id_base) + np.arange(B, dtype=np.uint64), t)
    u = (w * total) >> np.uint64(32)
    return np.where(total > 0, (np.cumsum(visits, 1) <= u[:, None]).sum(1), 0).astype(np.int8)


# ---- 1. the search ------------------------------------------------------------------------------------------------------------------------
def _search_case(kind, dyn, K, puct, **kw):
    whole, shards = _run(kind, dyn, K, puct, (20, 28), **kw)
    assert whole.iterations == 48 and (whole.visits[whole._roots] == 48 * K).all()
    _not_vacuous(whole)
    for off, s in shards:
        _same_trees(s, whole, off)


@pytest.mark.parametrize("puct", [False, True])
@pytest.mark.parametrize("K", PATHS)
@pytest.mark.parametrize("kind,dyn", KINDS)
def test_a_sharded_search_is_the_whole_search(kind, dyn, K, puct):
    _search_case(kind, dyn, K, puct)


def test_a_sharded_puct_search_over_float32_observations_is_the_whole_search():
    import torch

    _search_case(2, True, 4, True, obs_dtype=torch.float32)


# ---- 2. moves -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("puct", [False, True])
@pytest.mark.parametrize("K", PATHS)
@pytest.mark.parametrize("kind,dyn", KINDS)
def test_sharded_moves_are_the_whole_moves(kind, dyn, K, puct):
    import torch

    whole, shards = _run(kind, dyn, K, puct, (20, 28))
    t = 3
    picks = {}
    for greedy in (False, True):
        wa, wpi, wv = whole.pick_moves(greedy=greedy, t=t)
        picks[greedy] = wa.cpu().numpy()
        assert np.array_equal(picks[greedy], _sampled(whole, t) if not greedy else whole.best_actions().cpu().numpy())
        for off, s in shards:
            n = s.trees
            a, pi, v = s.pick_moves(greedy=greedy, t=t)
            assert torch.equal(a, wa[off:off + n]), (greedy, off)
            assert _raw(pi) == _raw(wpi[off:off + n]) and _raw(v) == _raw(wv[off:off + n]), (greedy, off)
            if not greedy:
                assert np.array_equal(a.cpu().numpy(), _sampled(s, t)), off
    assert (picks[False] != picks[True]).any()                       # the inputs: the counter words decide some move
    wr, wd = whole.advance(torch.as_tensor(picks[False], device=whole.env.device))
    whole.run(16)
    for off, s in shards:
        n = s.trees
        r, d = s.advance(torch.as_tensor(picks[False][off:off + n], device=s.env.device))
        s.run(16)
        assert _raw(r) == _raw(wr[off:off + n]) and torch.equal(d, wd[off:off + n]), off
        _same_trees(s, whole, off, live_only=True)
    assert whole.iterations == 64 and bool(wd.any()) and not bool(wd.all())     # moves that end an episode and moves that do not


# ---- 3. self-play -------------------------------------------------------------------------------------------------------------------------
RING = ("obs", "pi", "value", "action", "reward", "done", "move", "z")


def _play_case(kind, dyn, K, puct, **kw):
    import torch

    from snac_amd import SelfPlay

    its = 12
    whole, shards = _envs(kind, dyn, few_bricks=True, total_step=6, time_gt=True, **kw)
    plays = []
    for env in [whole] + [e for _, e in shards]:
        play = SelfPlay(_search(env, K, puct, (env.total_step + 1) * its), capacity_moves=8, sample_moves=3)
        play.play(11, iterations=its)
        play.targets()
        plays.append(play)
    torch.cuda.synchronize()
    ref = plays[0]
    assert ref.moves == 11 and ref.head == 3 and ref.valid_moves() == 8          # the ring wrapped
    done = ref.done.cpu().numpy() != 0
    assert done.any(1).sum() > 1                                     # episodes ended at more than one move
    assert (whole._episode.cpu().numpy() >= 1).all()                 # every tree restarted (episode 0 comes from the first reset())
    assert ref.z.any() and (ref.action.cpu().numpy() != 0).any()
    for (off, env), play in zip(shards, plays[1:]):
        n = env.num_envs
        for name in RING:
            assert _raw(getattr(play, name)) == _raw(getattr(ref, name)[:, off:off + n]), (name, off)
        _same_env_rows(env, whole, off)
        _same_trees(play.search, ref.search, off, live_only=True)


@pytest.mark.parametrize("puct", [False, True])
@pytest.mark.parametrize("K", PATHS)
def test_sharded_self_play_is_the_whole_self_play(K, puct):
    _play_case(2, True, K, puct)


def test_sharded_self_play_in_1d_static():
    _play_case(1, False, 4, False)


def test_sharded_puct_self_play_over_float32_observations():
    import torch

    _play_case(2, True, 4, True, obs_dtype=torch.float32)
