"""Batched UCT tree search on the device over node pools (snac_uct_node, snac_uct_select / snac_uct_backup / snac_uct_advance and
snac_uct_select_paths / snac_uct_backup_paths, snac_uct_select_puct / snac_uct_set_priors, snac_uct_pick_moves / snac_uct_restart,
snac_uct_select_paths_norm / snac_uct_select_puct_norm / snac_uct_backup_paths_norm / snac_uct_bounds, snac_uct_select_gumbel /
snac_uct_gumbel_candidates, snac_uct_set_priors_value / snac_uct_select_gumbel_interior / snac_uct_improved_policy, snac_uct_load_roots:
include/snac_hip.h; snac_amd/csrc/k_uct.hip, k_uct_play.hip, k_uct_reanalyse.hip).

B independent trees, one path per tree per iteration (paths=1) or K of them (paths=K, below).  An iteration is enqueued on the env's
stream with no host synchronisation: selection (k_uct_select), the B tree edges (snac_transition_nodes*: edge b belongs to tree b),
each leaf's first reward (the new edge's or the stored one: two small torch ops), the default-policy evaluation of the B leaves
(snac_evaluate_nodes*, script/MCTS/utils/mcts.py:100-110) and the backup (k_uct_backup).

    env = BatchedDMPEnv(2, True, 4096, seed=1); env.reset()
    search = UCTSearch(env, nodes_per_tree=256, horizon=600, gamma=0.99)
    search.reset()                       # root b <- env row b
    search.run(200)
    a = search.best_actions()            # [B] the most-visited root action

Playing an episode: advance() plays one action per tree and keeps the played child's subtree (its visits, values and nodes) as the
new tree, compacted on the device with no host synchronisation:

    search.reset()
    for move in range(moves):
        search.run(50)
        r, d = search.advance(search.best_actions())   # reward / done of the move, per tree
    search.store_roots()                 # env row b <- root b: observe(), iou() of the played states

Root parallelism over one state: give G states `copies` trees each (reset(rows=...) with each row repeated); the copies draw different
counter-RNG words because their slots differ, and their root statistics add up:

    search = UCTSearch(env, 128, 600, 0.99, trees=G * copies)
    search.reset(rows=torch.arange(G, device=env.device).repeat_interleave(copies))
    search.run(100)
    visits = search.root_visits().view(G, copies, -1).sum(1)      # [G, A]

Tree parallelism for a few trees: paths=K sends K paths through EACH tree per iteration, kept apart by virtual loss (a path counts as
a visit, and as a return of -virtual_loss, on every node under it until the backup), so that an iteration hands B * K edges and B * K
leaves to the transition and evaluation kernels.  One tree keeps the whole budget and advance() keeps its subtree, which root
parallelism cannot do.  Root visits after n iterations are n * K; virtual_loss of the order of a step reward spreads the K paths
wider than the default 0.0 (virtual visits only) at some cost in search quality:

    env = BatchedDMPEnv(2, True, 64, seed=1); env.reset()
    search = UCTSearch(env, nodes_per_tree=8192, horizon=100, gamma=0.99, max_iterations=256, paths=16)
    search.reset()
    search.run(256)                      # 4096 leaf evaluations per tree
    r, d = search.advance(search.best_actions())

A policy / value network in place of the rollout: evaluator=fn makes the search PUCT ("PUCT" in include/snac_hip.h).  Once per iteration
fn gets the observation rows of the B * K leaves, in slot order, on the env's device with the env's stream current, and returns
(priors [S, A] probabilities, value [S]); the priors are stored in the expanded nodes as float32 as given (softmax and masking are the
caller's; root noise is add_dirichlet_noise(), or the caller's own through root_priors() / set_root_priors(p)), and first reward +
value (0 at a terminal leaf) is backed up in place of a rollout estimate.  c is then the PUCT constant, first_play_value the q of an untried action; horizon only spaces the counter words (0 is allowed).
reset() and advance() call fn on the B roots for the priors of the new roots.

    net = torch.nn.Sequential(torch.nn.Linear(env.obs_dim, 128), torch.nn.ReLU(), torch.nn.Linear(128, env.num_actions + 1)).to(env.device)

    @torch.no_grad()
    def fn(obs):
        y = net(obs.to(torch.float32))
        return torch.softmax(y[:, :-1], 1), torch.tanh(y[:, -1])

    search = UCTSearch(env, nodes_per_tree=512, horizon=0, gamma=0.99, c=1.25, paths=16, evaluator=fn)
    search.reset()
    search.run(32)
    r, d = search.advance(search.best_actions())

The network on the device: evaluator=DeviceMLP(net, env) (snac_amd/mlp.py; a Sequential of Linear and ReLU whose last output is the value
as it is, no tanh) runs the network, its softmax / value head, the terminal mask and est += value as ONE launch per iteration
(snac_mlp_uct_value_leaves; "Policy / value network on the device" in include/snac_hip.h) in place of fn's launches and the torch
operations behind them, with float64 sums in a stated order: the same bytes on every run, and the bytes of
evaluator=lambda o: mlp.policy_value(o), the generic path.  The parameters are read in place at every launch.

Self-play: pick_moves() draws a move per tree from the root's visit counts (argmax, or in proportion to them: counter-RNG stream 3) and
gives the visit distribution and the root value, the training targets of the network above; restart(mask) starts a new episode in the
finished trees and leaves the others alone.  Neither synchronises with the host.  snac_amd/selfplay.py (SelfPlay) is the loop with a
ring of targets around them:

    r, d = search.advance(search.pick_moves(greedy=False, t=move)[0], check=False)
    env.reset(mask=d, want_obs=False)    # the finished trees' env rows: the next episode's start state (and plan)
    search.restart(d)                    # tree b <- env row b where d[b]; every other tree keeps its subtree

    play = SelfPlay(search, capacity_moves=256, sample_moves=10)
    play.play(64, iterations=32); play.targets(); batch = play.sample(512)      # obs, pi, z, ...

Rewards of any scale: q_normalise=True keeps, per tree, the smallest and the largest mean value W / N of its nodes below the root
(q_bounds, [B, 2] float64: lo, hi; empty: +inf, -inf) and compares (q - lo) / (hi - lo) in place of a tried child's q ("Normalised q" in
include/snac_hip.h), in the rollout search and in PUCT, for every paths >= 1.  This environment pays 5 or 10 per brick and -100 for a
boxed-in 3D episode, so raw returns run from tens to hundreds and drown an exploration term of order 1; normalised, c keeps its textbook
meaning at every move of an episode.  first_play_value is then in normalised units: 0.0 rates an untried action like the worst child
seen so far, 1.0 like the best.  Until a tree has seen two different means its q is left as it is.  The backup folds the new means into
the bounds; advance() and restart() recompute them from the tree they leave (a kept subtree: the bounds of its own nodes, since the
return still to collect shrinks along an episode; a one-node tree: empty), all on the env's stream with no host synchronisation.

    search = UCTSearch(env, nodes_per_tree=512, horizon=0, gamma=0.99, c=1.25, paths=16, evaluator=fn, q_normalise=True)

Small budgets: gumbel=m (with an evaluator and q_normalise=True) adds the Gumbel root search of Gumbel AlphaZero / MuZero (Danihelka et
al. 2022; "Gumbel root" in include/snac_hip.h).  At a few dozen iterations per move PUCT's visit counts are a poor policy target and an
unvisited action gets target 0; instead m root actions are sampled without replacement by Gumbel-top-k, the budget is spent on them by
sequential halving, the survivor is played and the target is an improved policy built from completed q-values.  Below the root the
search is the normalised PUCT search.  `cand` (int32 [B], a bit per root action) holds the candidates; reset(), advance() and restart()
zero it, and with cand all zero run(n) is the PUCT search.

    search = UCTSearch(env, 512, 0, 0.99, c=1.25, paths=4, evaluator=fn, q_normalise=True, gumbel=4)
    search.reset()
    search.gumbel_begin(search.gumbel_scores())          # log-priors + Gumbel noise -> the 4 candidates of every tree
    search.gumbel_run(32)                                # gumbel_schedule(32, 4): two phases of 16 iterations, a halving between them
    a, pi = search.gumbel_actions(), search.improved_policy()
    r, d = search.advance(a)

gumbel_interior=True finishes the method ("Gumbel interior" in include/snac_hip.h): every node keeps the value the evaluator gave for
its state (net_values), and every node that is not a root taking a candidate's turn -- every level below the root, and the root in
run(n) -- selects, deterministically, the action with the largest pi'(a) - N(a) / (1 + sum N), where pi' is the node's improved policy:
softmax(log prior + sigma(completed q)), an unvisited action's q completed by v_mix, the mix of the node's network value and the
prior-weighted mean of its visited children's q.  c, virtual_loss and first_play_value then play no part in selection (first_play_value
still rates an unvisited candidate in the halvings and the final move), and improved_policy() is computed on the device by the function
that selects, with the paper's v_mix.

    search = UCTSearch(env, 512, 0, 0.99, paths=4, evaluator=fn, q_normalise=True, gumbel=4, gumbel_interior=True)

Stored positions: load_roots(records, index) is reset() from node records instead of env rows ("Reanalyse" in include/snac_hip.h).  A
record is a complete state -- header with the plan row, episode counter, grid; the plan table stays in the env -- so a position can be
searched again long after its env row has moved on: tree b starts over from records[index[b]] (one launch, no host synchronisation).
SelfPlay(keep_states=True) keeps each move's root record in its ring and reanalyse() re-searches them with a second search over the same
env, typically one with the latest network as its evaluator:

    again = UCTSearch(env, 512, 0, 0.99, c=1.25, paths=4, evaluator=latest, trees=256, max_iterations=32)
    again.load_roots(play.state.view(-1, play.state.shape[-1]), index)       # index: [256] flat ring entries
    again.run(32)

Counter words: iteration `it` (counted from reset()) steps its edges with t = it * (H + 1) and rolls its leaves out from
t0 = it * (H + 1) + 1, so no two iterations share a word.  Path k of tree b draws both with the key (env_id_base + b) * K + k, its slot
in the search over ALL envs, so no two paths share a word either and a shard of the trees (env_id_base = E: dist.py) searches exactly as
the same trees do in one search over the whole batch; the transition and evaluation kernels key edge / leaf s of a call by the
descriptor's base + s, so the per-iteration launches get a copy of the env's descriptor with env_id_base * K.  What is per tree keeps
the env's own base: the move's edge of advance() (env_id_base + b, it * (H + 1)), pick_moves() (stream 3, env_id_base + b), restart()
and env.reset() (stream 1).  A
captured graph freezes these arguments: a graph of run(n), replayed after reset(), repeats run(n) exactly; a graph of one iteration
replayed n times would draw iteration 0's words every time.
"""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import ptr as _ptr
from .mlp import DeviceMLP
from .nodes import NodePool


_NODE = _lib.STRUCTS["snac_uct_node"]
WORDS = C.sizeof(_NODE) // 4                                         # int32 words per snac_uct_node (256 bytes)


def _words(field):
    """The int32 words of a snac_uct_node field within a row of `stats`, as a slice."""
    f = getattr(_NODE, field)
    return slice(f.offset // 4, (f.offset + f.size) // 4)


_CHILD, _CHILD_VISITS, _CHILD_VALUE, _VALUE_SUM, _REWARD = (_words(f) for f in ("child", "child_visits", "child_value", "value_sum", "reward"))
_PARENT, _ACTION, _TERMINAL, _VISITS = (_words(f).start for f in ("parent", "action", "terminal", "visits"))
_PRIOR, _NET_VALUE = _lib.UCT_PRIOR_WORD, _lib.UCT_NET_VALUE_WORD    # first words of prior[0 .. 7] (float32) and net_value (float64)


def uct_tables(n):
    """(log_table, rsqrt_table) of length n as python floats: [sqrt(log(i))], [1.0 / sqrt(i)]; entry 0 is 0.0 (never read: a node with
    children has been visited)."""
    lt = [0.0] + [math.sqrt(math.log(i)) for i in range(1, n)]
    rt = [0.0] + [1.0 / math.sqrt(i) for i in range(1, n)]
    return lt, rt


def gumbel_schedule(n, m):
    """The sequential-halving plan of n iterations over m candidates: max(1, ceil(log2 m)) phases of n // phases iterations each, the
    last phase taking the remainder.  Returns [(halve, i)] per iteration: halve -- the candidates are halved before it (the first
    iteration of every phase but the first); i -- its index inside its phase.  The candidates then run m -> ceil(m / 2) -> ... -> 2."""
    n, m = int(n), int(m)
    if m < 1:
        raise ValueError("m must be >= 1")
    phases = max(1, (m - 1).bit_length())
    if n < phases:
        raise ValueError("%d iterations cannot cover the %d halving phases of %d candidates" % (n, phases, m))
    L = n // phases
    plan = []
    for p in range(phases):
        length = L if p < phases - 1 else n - L * (phases - 1)
        plan += [(p > 0 and i == 0, i) for i in range(length)]
    return plan


class UCTSearch:
    """UCT over `trees` independent trees of `nodes_per_tree` nodes each on one NodePool of env's kind (include/snac_hip.h, "UCT tree
    search", has the exact selection and backup rules).  paths=K > 1: K paths per tree and iteration with `virtual_loss` per in-flight
    path ("K paths per tree and iteration" there).  Everything is allocated here; run() only enqueues work."""

    def __init__(self, env, nodes_per_tree, horizon, gamma, c=math.sqrt(2), max_iterations=1024, trees=None, paths=1, virtual_loss=0.0,
                 evaluator=None, first_play_value=None, q_normalise=False, gumbel=None, gumbel_c_visit=50.0, gumbel_c_scale=1.0,
                 gumbel_interior=False):
        """evaluator: None (the rollout search) or a callable obs [S, obs_dim] -> (priors [S, A], value [S]) that guides a PUCT search
        (the module docstring); first_play_value (PUCT only, default 0.0): the q of an untried action.  q_normalise (a bool): compare
        q normalised by the tree's min-max bounds (the module docstring); q_bounds is then a [B, 2] float64 tensor, else None.
        gumbel (None or m >= 1; needs an evaluator and q_normalise=True): the Gumbel root search over m sampled root actions (the module
        docstring, "Gumbel root"), with sigma(q) = (gumbel_c_visit + max_a N_a) * gumbel_c_scale * q.  gumbel_interior (a bool; True
        needs gumbel): the Gumbel rule below the root too, the network values kept in the nodes, improved_policy() with the full v_mix."""
        if not isinstance(gumbel_interior, bool):
            raise ValueError("gumbel_interior must be a bool")
        if gumbel_interior and gumbel is None:
            raise ValueError("gumbel_interior=True extends the Gumbel root search: give gumbel=m")
        if not isinstance(q_normalise, bool):
            raise ValueError("q_normalise must be a bool")
        if gumbel is not None:
            if isinstance(gumbel, bool) or not isinstance(gumbel, int) or gumbel < 1:
                raise ValueError("gumbel must be an integer >= 1")
            if evaluator is None or not q_normalise:
                raise ValueError("the Gumbel root search needs an evaluator and q_normalise=True")
            if not (math.isfinite(float(gumbel_c_visit)) and math.isfinite(float(gumbel_c_scale))):
                raise ValueError("gumbel_c_visit and gumbel_c_scale must be finite")
        self.gumbel, self.gumbel_c_visit, self.gumbel_c_scale = gumbel, float(gumbel_c_visit), float(gumbel_c_scale)
        self.gumbel_interior = gumbel_interior
        if evaluator is not None and not callable(evaluator):
            raise ValueError("evaluator must be callable: obs [S, obs_dim] -> (priors [S, A], value [S])")
        if first_play_value is not None and evaluator is None:
            raise ValueError("first_play_value belongs to the PUCT search: give an evaluator")
        fpv = 0.0 if first_play_value is None else float(first_play_value)
        if not math.isfinite(fpv):
            raise ValueError("first_play_value must be finite")
        self.evaluator, self.first_play_value, self.q_normalise = evaluator, fpv, q_normalise
        self.env = env
        self.trees = int(env.num_envs if trees is None else trees)
        self.nodes_per_tree, self.horizon, self.gamma, self.c = int(nodes_per_tree), int(horizon), float(gamma), float(c)
        self.max_iterations = int(max_iterations)
        self.paths, self.virtual_loss = int(paths), float(virtual_loss)
        B, cap, K = self.trees, self.nodes_per_tree, self.paths
        if B < 1 or cap < 1:
            raise ValueError("trees and nodes_per_tree must be >= 1")
        if self.horizon < 0 or self.max_iterations < 1:
            raise ValueError("horizon must be >= 0 and max_iterations >= 1")
        if K < 1 or K != paths:
            raise ValueError("paths must be an integer >= 1")
        if not math.isfinite(self.virtual_loss):
            raise ValueError("virtual_loss must be finite")
        if B * (cap + K) > 0x7FFFFFFF:
            raise ValueError("trees * (nodes_per_tree + %s) rows exceed int32" % ("1" if K == 1 else "paths"))
        if self.max_iterations * K + 1 > 0x7FFFFFFF:
            raise ValueError("max_iterations * paths visits exceed int32")
        if K > 1 and not -(1 << 63) <= env.env_id_base * K <= (env.env_id_base + B) * K - 1 < 1 << 63:
            raise ValueError("the slot keys (env_id_base + b) * paths + k exceed int64")
        self.num_actions = env.num_actions
        self.rows = B * (cap + K)                                    # the trees' rows, then a scratch row per slot b * K + k
        S = B * K
        dev = env.device
        self.pool = NodePool(env, self.rows)
        self.stats = torch.zeros((self.rows, WORDS), dtype=torch.int32, device=dev)
        assert self.stats.data_ptr() % 128 == 0
        lt, rt = uct_tables(self.max_iterations * K + 1)                 # the root's N + P reaches max_iterations * K
        self.log_table = torch.tensor(lt, dtype=torch.float64, device=dev)
        self.rsqrt_table = torch.tensor(rt, dtype=torch.float64, device=dev)
        self._gpow = torch.tensor([self.gamma ** t for t in range(max(1, self.horizon))], dtype=torch.float64, device=dev)

        def slot(dtype):
            return torch.zeros(S, dtype=dtype, device=dev)

        self._used = torch.zeros(B, dtype=torch.int32, device=dev)
        self._src, self._dst, self._leaf = slot(torch.int32), slot(torch.int32), slot(torch.int32)
        self._action, self._expanded = slot(torch.int8), slot(torch.uint8)
        self._r_leaf, self._reward, self._first = slot(torch.float32), slot(torch.float32), slot(torch.float32)
        self._done, self._est = slot(torch.uint8), slot(torch.float64)
        self._iteration = 0
        self._roots = torch.arange(B, device=dev) * cap
        self._lib = env._lib
        P = self.pool
        self._select_args = (self.num_actions, _ptr(self.stats), self.rows, B, cap, self.c, _ptr(self.log_table), _ptr(self.rsqrt_table),
                             int(self.log_table.numel()), _ptr(self._used), _ptr(self._src), _ptr(self._dst), _ptr(self._action),
                             _ptr(self._leaf), _ptr(self._expanded), _ptr(self._r_leaf))
        self._backup_args = (self.num_actions, _ptr(self.stats), self.rows, B, cap, self.gamma, _ptr(self._src), _ptr(self._action),
                             _ptr(self._leaf), _ptr(self._expanded), _ptr(self._reward), _ptr(self._done), _ptr(self._est))
        self._transition = getattr(self._lib, P.TRANSITION)
        self._evaluate_fn = getattr(self._lib, P.EVALUATE)
        # the rollout search with paths=1 keeps the one-path entry points, unless it normalises q: there is no one-path _norm form
        self._multi = K > 1 or evaluator is not None or q_normalise
        self._slot_desc = None if K == 1 else type(env._desc)()      # the per-iteration launches' descriptor (_slots())
        if self._multi:
            self._first_slot, self._first_idx = slot(torch.int32), slot(torch.int32)
            self._first_new, self._first_has = slot(torch.float32), slot(torch.bool)
            self._select_args = (self.num_actions, _ptr(self.stats), self.rows, B, cap, K, self.c, self.virtual_loss, _ptr(self.log_table),
                                 _ptr(self.rsqrt_table), int(self.log_table.numel()), _ptr(self._used), _ptr(self._src), _ptr(self._dst),
                                 _ptr(self._action), _ptr(self._leaf), _ptr(self._expanded), _ptr(self._r_leaf), _ptr(self._first_slot))
            self._backup_args = (self.num_actions, _ptr(self.stats), self.rows, B, cap, K, self.gamma, _ptr(self._src), _ptr(self._action),
                                 _ptr(self._leaf), _ptr(self._expanded), _ptr(self._reward), _ptr(self._done), _ptr(self._est))
        if evaluator is not None:                                    # PUCT: priors in the nodes, the evaluator's value in place of a rollout
            A, n = self.num_actions, self.max_iterations * K + 1
            self.sqrt_table = torch.tensor([math.sqrt(max(i, 1)) for i in range(n)], dtype=torch.float64, device=dev)
            self.inv_table = torch.tensor([1.0 / (1 + i) for i in range(n)], dtype=torch.float64, device=dev)
            self._select_args = (A, _ptr(self.stats), self.rows, B, cap, K, self.c, self.virtual_loss, self.first_play_value,
                                 _ptr(self.sqrt_table), _ptr(self.inv_table), n, _ptr(self._used), _ptr(self._src), _ptr(self._dst),
                                 _ptr(self._action), _ptr(self._leaf), _ptr(self._expanded), _ptr(self._r_leaf), _ptr(self._first_slot))
            self._obs = torch.zeros((S, env.obs_dim), dtype=env.obs_dtype, device=dev)
            self._root_obs = torch.zeros((B, env.obs_dim), dtype=env.obs_dtype, device=dev)
            self._priors = torch.zeros((S, A), dtype=torch.float32, device=dev)
            self._root_priors = torch.zeros((B, A), dtype=torch.float32, device=dev)
            self._prior_rows, self._none = slot(torch.int32), torch.full((S,), -1, dtype=torch.int32, device=dev)
            self._term_new, self._term_old, self._term = slot(torch.uint8), slot(torch.int32), slot(torch.bool)
            self._value, self._zero = slot(torch.float64), slot(torch.float64)
            self._root_rows = self._roots.to(torch.int32)
            self._observe = getattr(self._lib, P.OBSERVE)
            self._obs_ptrs = (_ptr(P.records), P.rows, S, _ptr(self._leaf), _ptr(self._obs))
            self._root_obs_ptrs = (_ptr(P.records), P.rows, B, _ptr(self._root_rows), _ptr(self._root_obs))
            self._prior_args = (A, _ptr(self.stats), self.rows, S, _ptr(self._prior_rows), _ptr(self._priors), 0)
            self.noise_bad_rows = torch.zeros(1, dtype=torch.int32, device=dev)     # add_dirichlet_noise(): roots whose priors it refused
            self._mlp = evaluator if isinstance(evaluator, DeviceMLP) else None
            if self._mlp is not None:                                # the network on the device: _value_leaves() is one fused launch
                mlp = self._mlp
                if mlp.device != dev or mlp.num_actions != A or mlp.dims[0] != env.obs_dim:
                    raise ValueError("the DeviceMLP must be on %s with %d inputs and num_actions = %d" % (dev, env.obs_dim, A))
                self._leaves_args = (A, _ptr(self._obs), int(env.obs_dtype == torch.float64), S, _ptr(self._first_has), _ptr(self._first_idx),
                                     _ptr(self._done), _ptr(self.stats), self.rows, _ptr(self._leaf), _ptr(self._priors), _ptr(self._value),
                                     _ptr(self._est))
        self.q_bounds = None
        if q_normalise:                                              # the _norm entry points: the same arguments, then the bounds
            self.q_bounds = torch.empty((B, 2), dtype=torch.float64, device=dev)
            assert self.q_bounds.data_ptr() % 16 == 0
            self._no_bounds = torch.tensor([math.inf, -math.inf], dtype=torch.float64, device=dev)
            self.q_bounds.copy_(self._no_bounds.expand(B, 2))
            self._select_args += (_ptr(self.q_bounds),)
            self._backup_args += (_ptr(self.q_bounds),)
            self._bounds_args = (_ptr(self.stats), self.rows, B, cap, _ptr(self._used))
        self.cand = None
        if gumbel is not None:                                       # snac_uct_select_gumbel: the _norm arguments, then cand and the offset
            self.cand = torch.zeros(B, dtype=torch.int32, device=dev)
            self._gumbel_begun = False
            self._gscores = torch.zeros((B, self.num_actions), dtype=torch.float32, device=dev)
            self._select_args += (_ptr(self.cand),)
            self._cand_args = (self.num_actions, _ptr(self.stats), self.rows, B, cap)
            self._cand_tail = (_ptr(self._gscores), self.gumbel_c_visit, self.gumbel_c_scale, self.first_play_value, _ptr(self.q_bounds),
                               _ptr(self.cand))
            if gumbel_interior:                                      # the network value of every node; the roots' improved policies
                self._root_value, self._root_term = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
                self._root_zero = torch.zeros(B, dtype=torch.float64, device=dev)
                self._policy_args = (self.num_actions, _ptr(self.stats), self.rows, B, cap, B, _ptr(self._root_rows), self.gumbel_c_visit,
                                     self.gumbel_c_scale, _ptr(self.q_bounds))
        self._edge_ptrs = (_ptr(P.records), P.rows, S, _ptr(self._src), _ptr(self._dst))
        self._step_ptrs = (_ptr(self._action), None, None, _ptr(self._reward), _ptr(self._done))
        self._eval_ptrs = (_ptr(P.records), P.rows, S, _ptr(self._leaf), self.horizon)
        self._est_ptrs = (_ptr(self._gpow), _ptr(self._est), None)
        # advance(): the B root edges into the scratch records, then the re-rooting (work: an old -> new and a new -> old map per tree)
        self._adv_action = torch.zeros(B, dtype=torch.int8, device=dev)
        self._adv_reward, self._adv_done = torch.zeros(B, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
        self._adv_src = self._roots.to(torch.int32)
        self._adv_dst = (B * cap + torch.arange(B, device=dev)).to(torch.int32)
        self._work = torch.empty(2 * B * cap, dtype=torch.int32, device=dev)
        self._adv_edge_ptrs = (_ptr(P.records), P.rows, B, _ptr(self._adv_src), _ptr(self._adv_dst))
        self._adv_step_ptrs = (_ptr(self._adv_action), None, None, _ptr(self._adv_reward), _ptr(self._adv_done))
        self._advance_args = (self.num_actions, _ptr(self.stats), self.rows, B, cap, _ptr(P.records), P.WORDS * 4, P.rows, _ptr(self._adv_action),
                              _ptr(self._adv_reward), _ptr(self._adv_done), _ptr(self._used), _ptr(self._work))
        # pick_moves() / restart(): the roots' statistics; the B env rows into the scratch records, then the masked trees' new roots
        self._pick_args = (C.byref(env._desc), self.num_actions, _ptr(self.stats), self.rows, B, cap)
        self._sample_all = torch.zeros(B, dtype=torch.uint8, device=dev)     # greedy=False
        self._rs_mask, self._rs_term = torch.zeros(B, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
        self._rs_flags = torch.zeros(B, dtype=torch.int32, device=dev)
        self._rs_hdr = P.records[B * cap:B * cap + B, 0]             # word 0 of the scratch records: position and flags
        self._pack = getattr(self._lib, P.PACK)
        self._restart_args = (self.num_actions, _ptr(self.stats), self.rows, B, cap, _ptr(P.records), P.WORDS * 4, P.rows, _ptr(self._rs_mask),
                              _ptr(self._rs_term), _ptr(self._used))
        self._load_args = self._restart_args[:8]                     # load_roots(): then src, src_rows, index, used

    # ---- the search ---------------------------------------------------------------------------------------------------
    def reset(self, rows=None):
        """Root b <- env row rows[b] (None: row b), also copied into the tree's scratch record; the statistics and the iteration
        count start over.  A root whose row has NEED_RESET is terminal."""
        env, B, cap = self.env, self.trees, self.nodes_per_tree
        if rows is None:
            if B > env.num_envs:
                raise ValueError("%d trees, %d env rows: give rows" % (B, env.num_envs))
            rows = torch.arange(B, device=env.device)
        rows = torch.as_tensor(rows, device=env.device).reshape(-1)
        if int(rows.numel()) != B:
            raise ValueError("rows must have %d entries" % B)
        roots = self._roots
        self.pool.load(rows=rows, node_rows=roots)
        self.pool.load(rows=rows, node_rows=B * cap + torch.arange(B, device=env.device))
        self.stats.zero_()
        self.stats[:, _CHILD] = -1
        self.stats[:, _PARENT:_ACTION + 1] = -1                      # parent, action: neighbours
        self.stats[roots, _TERMINAL] = self.pool.need_reset[roots].to(torch.int32)
        self._used.fill_(1)
        self._iteration = 0
        if self.q_normalise:
            self.q_bounds.copy_(self._no_bounds.expand(B, 2))
        self._no_candidates()
        if self.evaluator is not None:
            with torch.cuda.device(env.device):
                self._prime_roots()

    def load_roots(self, records, index=None):
        """reset() from stored node records instead of env rows (snac_uct_load_roots; include/snac_hip.h, "Reanalyse"): root b <-
        records[index[b]] (None: records[b]), also copied into the tree's scratch record; fresh root statistics, terminal where the
        record's header carries NEED_RESET; the iteration count, the q bounds and the candidates start over and a PUCT search primes the
        new roots.  records: a contiguous uint8 [n, record_bytes] tensor of the pool's kind on the env's device, 128-byte aligned and
        apart from the pool's own records (SelfPlay.state, NodePool.records viewed as bytes); index: an integer tensor [trees], clamped
        into [0, n) on the device.  One launch on the env's stream, no host synchronisation.  Unlike reset(), only the roots'
        statistics rows are written: the other rows are outside every tree (tree_sizes() == 1), as after restart()."""
        B, rb = self.trees, self.pool.WORDS * 4
        if not torch.is_tensor(records) or records.dtype != torch.uint8 or records.dim() != 2 or int(records.shape[1]) != rb:
            raise ValueError("records must be a uint8 [n, %d] tensor: the node records of a %dD pool" % (rb, self.pool.KIND))
        n = int(records.shape[0])
        if n < 1 or (index is None and n < B):
            raise ValueError("%d records for %d trees: give an index" % (n, B) if n else "records is empty")
        if index is not None:
            if not torch.is_tensor(index) or int(index.numel()) != B:
                raise ValueError("index must be a tensor of %d entries" % B)
            if index.is_floating_point() or index.is_complex() or index.dtype == torch.bool:
                raise ValueError("index must be integers")
        env = self.env
        if records.device != env.device or (index is not None and index.device != env.device):
            raise ValueError("records and index must be on %s" % env.device)
        if not records.is_contiguous() or records.data_ptr() % 128 != 0:
            raise ValueError("records must be contiguous and 128-byte aligned")
        if index is not None:
            index = index.reshape(-1).to(torch.int32).contiguous()
        with torch.cuda.device(env.device):
            _lib.check(self._lib.snac_uct_load_roots(*self._load_args, _ptr(records), n, None if index is None else _ptr(index),
                                                     _ptr(self._used), env._stream()))
            self._iteration = 0
            if self.q_normalise:
                self.q_bounds.copy_(self._no_bounds.expand(B, 2))
            self._no_candidates()
            if self.evaluator is not None:
                self._prime_roots()

    def run(self, iterations):
        """Enqueue `iterations` iterations (select, transition, evaluate, backup; `paths` paths per tree each) on the env's stream; no host
        synchronisation."""
        n = int(iterations)
        if n < 0:
            raise ValueError("iterations must be >= 0")
        if self._iteration + n > self.max_iterations:
            raise ValueError("%d iterations after %d exceed max_iterations = %d" % (n, self._iteration, self.max_iterations))
        self._run(n)

    def _run(self, n):
        """run() without the budget check, for a caller that bounds the visit counts itself (SelfPlay: per episode)."""
        with torch.cuda.device(self.env.device):
            for _ in range(n):
                self._select()
                self._edges()
                self._evaluate()
                self._backup()
                if self.evaluator is not None:
                    self._set_priors()

    def advance(self, actions, check=True):
        """Play actions[b] in tree b and re-root it (include/snac_hip.h, "Re-rooting after a move"): a tried action keeps its child's
        subtree, compacted to the tree's first rows; an untried one leaves a single node, the root's transition by that action; a
        terminal root stays as it is.  Enqueues the B root edges (into the scratch records, with this iteration's counter words) and
        the re-rooting on the env's stream.  check=True rejects actions of the wrong length or outside [0, A) (a host read);
        check=False does no host synchronisation (out-of-range actions are clamped on the device).
        The iteration count is not reset: later iterations keep drawing fresh counter words, and max_iterations keeps bounding the
        iterations since reset(), which also keeps every visit count inside the U tables.
        Returns (reward float32 [B], done bool [B]): the move's reward and done (a terminal root: 0, True)."""
        env, B = self.env, self.trees
        a = actions.to(env.device) if torch.is_tensor(actions) else torch.as_tensor(actions, device=env.device)
        a = a.reshape(-1)
        if int(a.numel()) != B:
            raise ValueError("actions must have %d entries" % B)
        if a.is_floating_point() or a.is_complex() or a.dtype == torch.bool:
            raise ValueError("actions must be integers")
        if check and (int(a.min()) < 0 or int(a.max()) >= self.num_actions):
            raise ValueError("actions must be in [0, %d)" % self.num_actions)
        reward = torch.empty(B, dtype=torch.float32, device=env.device)
        done = torch.empty(B, dtype=torch.uint8, device=env.device)
        self._advance_into(a, reward, done)
        return reward, done.view(torch.bool)

    def _advance_into(self, a, reward, done, prime=True):
        """advance(check=False) of the B integer actions `a` on the device into the caller's reward float32 [B] / done uint8 [B];
        prime=False leaves the priors of the new roots to a priming that follows (restart())."""
        with torch.cuda.device(self.env.device):
            self._adv_action.copy_(a.clamp(0, self.num_actions - 1))
            self._no_candidates()
            self._root_edges()
            self._reroot(reward, done)
            if self.q_normalise:                                     # every tree: the bounds of the subtree it kept
                self._rebound(None)
            if prime and self.evaluator is not None:                 # the roots made from an untried action are unvisited: they get priors
                self._prime_roots()

    # ---- self-play: a move from the visit counts, a new episode in some trees ---------------------------------------------------
    def pick_moves(self, greedy=None, t=0, out=None, temperature=None):
        """One move per tree from its root's visit counts (snac_uct_pick_moves; include/snac_hip.h, "Self-play").  greedy: None or True
        -- the most-visited action, ties to the lowest (best_actions()); False -- drawn in proportion to the visits with the counter
        RNG's stream 3, keyed by (env_id_base + b, t); a [B] tensor -- per tree (non-zero: greedy).  t: the caller's move counter.  A
        root without child visits (a terminal root; before any iteration) gives action 0 and pi 0.  out: (action int8 [B], pi float32
        [B, A], value float32 [B]) contiguous on the env's device to write into.  Enqueued on the env's stream, no host synchronisation.
        temperature: None, or the T of the trees that are not greedy (snac_explore_pick_moves_temp; "Exploration noise" there): a number
        >= 0 or a float32 [B] tensor, per tree.  Such a tree draws in proportion to N_a ** (1 / T) from the same stream-3 word: T = 1 is
        the draw without a temperature bit for bit, T = 0 (or a NaN in the tensor) the most-visited action, T = inf uniform over the
        visited actions.  pi and value do not depend on it.
        Returns (action, pi: the visit distribution N_a / sum N, value: the root's W / N)."""
        B, A = self.trees, self.num_actions
        T = None
        if torch.is_tensor(temperature):
            if tuple(temperature.shape) != (B,) or temperature.dtype != torch.float32:
                raise ValueError("temperature must be a number or a float32 [%d] tensor" % B)
            T = temperature
        elif temperature is not None:
            if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not temperature >= 0:
                raise ValueError("temperature must be a number >= 0 or a float32 [%d] tensor" % B)
            T = float(temperature)
        g = None
        if torch.is_tensor(greedy) or isinstance(greedy, (list, tuple)):
            g = greedy if torch.is_tensor(greedy) else torch.as_tensor(greedy)
            if int(g.numel()) != B:
                raise ValueError("greedy must have %d entries" % B)
        elif greedy is not None and not isinstance(greedy, (bool, int)):
            raise ValueError("greedy must be None, a bool or a [%d] tensor" % B)
        if out is not None:
            if len(out) != 3:
                raise ValueError("out must be (action, pi, value)")
            for x, shape, dt in zip(out, ((B,), (B, A), (B,)), (torch.int8, torch.float32, torch.float32)):
                if not torch.is_tensor(x) or tuple(x.shape) != shape or x.dtype != dt or not x.is_contiguous():
                    raise ValueError("out must be contiguous action int8 [%d], pi float32 [%d, %d], value float32 [%d]" % (B, B, A, B))
        dev = self.env.device
        if out is None:
            out = (torch.empty(B, dtype=torch.int8, device=dev), torch.empty((B, A), dtype=torch.float32, device=dev),
                   torch.empty(B, dtype=torch.float32, device=dev))
        elif any(x.device != dev for x in out):
            raise ValueError("out must be on %s" % dev)
        if g is not None:
            g = g.to(dev).reshape(-1)
            if g.dtype != torch.uint8 or not g.is_contiguous():
                g = (g != 0).to(torch.uint8)
        elif greedy is not None and not greedy:
            g = self._sample_all
        if torch.is_tensor(T):
            T = T.to(dev).contiguous()
        self._pick(g, t, *out, temperature=T)
        return out

    def _pick(self, greedy, t, action, pi, value, temperature=None):
        """snac_uct_pick_moves on the env's stream; greedy uint8 [B] on the device or None, each output a tensor or None.  temperature
        (a float, or a contiguous float32 [B] tensor on the device): snac_explore_pick_moves_temp instead."""
        env = self.env
        with torch.cuda.device(env.device):
            if temperature is not None:
                per_tree = torch.is_tensor(temperature)
                _lib.check(self._lib.snac_explore_pick_moves_temp(*self._pick_args, None if greedy is None else _ptr(greedy), int(t) & 0xFFFFFFFF,
                                                                  _ptr(temperature) if per_tree else None, 1.0 if per_tree else temperature,
                                                                  *(None if x is None else _ptr(x) for x in (action, pi, value)), env._stream()))
                return
            _lib.check(self._lib.snac_uct_pick_moves(*self._pick_args, None if greedy is None else _ptr(greedy), int(t) & 0xFFFFFFFF,
                                                     *(None if x is None else _ptr(x) for x in (action, pi, value)), env._stream()))

    def restart(self, mask, rows=None):
        """A new episode in the trees with mask[b] != 0: env row rows[b] (None: row b) becomes their root exactly as reset() would make
        it (fresh statistics, one node; a PUCT search primes the new roots with the evaluator's priors); every other tree keeps its
        statistics, records and size bit for bit (a kept root that has been visited keeps its priors).  All B rows are loaded into the
        trees' scratch records, then snac_uct_restart moves the masked ones: no host synchronisation, no data-dependent shape (row
        indices are clamped on the device).  The iteration count is not reset, for advance()'s reasons."""
        env, B = self.env, self.trees
        m = mask if torch.is_tensor(mask) else torch.as_tensor(mask)
        if int(m.numel()) != B:
            raise ValueError("mask must have %d entries" % B)
        if rows is None:
            if B > env.num_envs:
                raise ValueError("%d trees, %d env rows: give rows" % (B, env.num_envs))
        else:
            rows = rows if torch.is_tensor(rows) else torch.as_tensor(rows)
            if int(rows.numel()) != B:
                raise ValueError("rows must have %d entries" % B)
            if rows.is_floating_point() or rows.is_complex() or rows.dtype == torch.bool:
                raise ValueError("rows must be integers")
            rows = rows.to(env.device).reshape(-1).to(torch.int32).contiguous()
        P = self.pool
        with torch.cuda.device(env.device):
            torch.ne(m.to(env.device).reshape(-1), 0, out=self._rs_mask.view(torch.bool))
            self._no_candidates()
            _lib.check(self._pack(C.byref(env._desc), C.byref(env._state), None if rows is None else _ptr(rows), B, _ptr(P.records), P.rows,
                                  _ptr(self._adv_dst), env._stream()))
            torch.bitwise_right_shift(self._rs_hdr, 16, out=self._rs_flags)          # the loaded records' NEED_RESET
            self._rs_flags.bitwise_and_(_lib.FLAG_NEED_RESET)
            self._rs_term.copy_(self._rs_flags)
            _lib.check(self._lib.snac_uct_restart(*self._restart_args, env._stream()))
            if self.q_normalise:                                     # the restarted trees have one node: empty bounds; the others keep theirs
                self._rebound(self._rs_mask)
            if self.evaluator is not None:
                self._prime_roots()

    # the two phases of advance() (tools/uct_advance_time.py times them one by one); the caller holds the env's device
    def _root_edges(self):
        env = self.env
        _lib.check(self._transition(C.byref(env._desc), C.byref(env._state), *self._adv_edge_ptrs, self._t(), *self._adv_step_ptrs, env._stream()))

    def _reroot(self, reward, done):
        _lib.check(self._lib.snac_uct_advance(*self._advance_args, _ptr(reward), _ptr(done), self.env._stream()))

    def _rebound(self, mask):
        """q_bounds of the trees with mask[b] != 0 (uint8 [B] on the device; None: all) <- the bounds of their nodes as they stand."""
        _lib.check(self._lib.snac_uct_bounds(*self._bounds_args, None if mask is None else _ptr(mask), _ptr(self.q_bounds), self.env._stream()))

    def store_roots(self, rows=None):
        """Env row rows[b] <- the record of root b (None: row b), so that observe() / iou() read the played states."""
        self.pool.store(node_rows=self._roots, rows=rows)

    # the four phases of an iteration (tools/uct_time.py times them one by one); the caller holds the env's device
    def _t(self):
        return (self._iteration * (self.horizon + 1)) & 0xFFFFFFFF

    def _select(self, offset=0):
        L = self._lib
        if self.gumbel is not None and self.gumbel_interior:         # the improved policy's rule wherever no candidate has its turn
            _lib.check(L.snac_uct_select_gumbel_interior(*self._select_args, offset, self.gumbel_c_visit, self.gumbel_c_scale,
                                                         self.env._stream()))
            return
        if self.gumbel is not None:                                  # cand all zero: snac_uct_select_puct_norm's search
            _lib.check(L.snac_uct_select_gumbel(*self._select_args, offset, self.env._stream()))
            return
        if self.evaluator is not None:
            fn = L.snac_uct_select_puct_norm if self.q_normalise else L.snac_uct_select_puct
        elif self.q_normalise:
            fn = L.snac_uct_select_paths_norm
        else:
            fn = L.snac_uct_select if self.paths == 1 else L.snac_uct_select_paths
        _lib.check(fn(*self._select_args, self.env._stream()))

    def _slots(self):
        """The descriptor of the launches over the B * K slots: the env's as it is now (set_action_probs() may have changed it), with
        env_id_base * K for K > 1, so that base + s is (env_id_base + b) * K + k (the module docstring, "Counter words")."""
        env, d = self.env, self._slot_desc
        if d is None:
            return env._desc
        C.memmove(C.byref(d), C.byref(env._desc), C.sizeof(d))
        d.env_id_base = env.env_id_base * self.paths
        return d

    def _edges(self):
        env = self.env
        _lib.check(self._transition(C.byref(self._slots()), C.byref(env._state), *self._edge_ptrs, self._t(), *self._step_ptrs, env._stream()))

    def _first_reward(self):
        if not self._multi:
            torch.where(self._expanded.view(torch.bool), self._reward, self._r_leaf, out=self._first)   # the new edge's reward or the stored one
        else:                                                        # the expander's edge reward (a fresh leaf: another slot's) or the stored
            torch.clamp(self._first_slot, min=0, out=self._first_idx)
            torch.index_select(self._reward, 0, self._first_idx, out=self._first_new)
            torch.ge(self._first_slot, 0, out=self._first_has)
            torch.where(self._first_has, self._first_new, self._r_leaf, out=self._first)
        self._est.copy_(self._first)

    def _evaluate(self):
        env = self.env
        self._first_reward()
        if self.evaluator is not None:
            self._evaluate_leaves()
            return
        _lib.check(self._evaluate_fn(C.byref(self._slots()), C.byref(env._state), *self._eval_ptrs, (self._t() + 1) & 0xFFFFFFFF, *self._est_ptrs,
                                     env._stream()))

    def _backup(self):
        L = self._lib
        fn = L.snac_uct_backup_paths_norm if self.q_normalise else L.snac_uct_backup_paths if self._multi else L.snac_uct_backup
        _lib.check(fn(*self._backup_args, self.env._stream()))
        self._iteration += 1

    # the PUCT phases (tools/uct_puct_time.py times them one by one); the caller holds the env's device
    def _call(self, obs, rows):
        """The evaluator on `rows` observation rows: (priors float32 [rows, A] as given, value float64 [rows])."""
        priors, value = self.evaluator(obs)
        if tuple(priors.shape) != (rows, self.num_actions) or int(value.numel()) != rows:
            raise ValueError("the evaluator must return priors [%d, %d] and value [%d]" % (rows, self.num_actions, rows))
        return priors.to(torch.float32), value.reshape(-1).to(torch.float64)

    def _observe_leaves(self):
        env = self.env
        _lib.check(self._observe(C.byref(env._desc), C.byref(env._state), *self._obs_ptrs, env._stream()))

    def _evaluate_leaves(self):
        """est = first reward + (the leaf terminal ? 0 : the evaluator's value); the leaf's priors wait for the backup."""
        self._observe_leaves()
        self._value_leaves()

    def _value_leaves(self):
        if self._mlp is not None:                                    # snac_mlp_uct_value_leaves: the network, its head and the lines below
            mlp = self._mlp
            _lib.check(self._lib.snac_mlp_uct_value_leaves(mlp._descriptor(), *self._leaves_args, _ptr(mlp.bad_rows), self.env._stream()))
            return
        priors, value = self._call(self._obs, self.trees * self.paths)
        self._priors.copy_(priors)
        torch.index_select(self._done, 0, self._first_idx, out=self._term_new)       # the expander's done (a fresh leaf: another slot's)
        torch.index_select(self.stats[:, _TERMINAL], 0, self._leaf, out=self._term_old)     # else the stored node's terminal
        torch.where(self._first_has, self._term_new != 0, self._term_old != 0, out=self._term)
        torch.where(self._term, self._zero, value, out=self._value)
        self._est.add_(self._value)

    def _set_priors(self):
        torch.where(self._expanded.view(torch.bool), self._leaf, self._none, out=self._prior_rows)
        if self.gumbel_interior:                                     # and the leaves' values: 0 where terminal (_value_leaves())
            _lib.check(self._lib.snac_uct_set_priors_value(*self._prior_args[:-1], _ptr(self._value), 0, self.env._stream()))
            return
        _lib.check(self._lib.snac_uct_set_priors(*self._prior_args, self.env._stream()))

    def _prime_roots(self):
        """Observe the B roots, call the evaluator, give the unvisited roots their priors (the value of this call is unused, except by a
        gumbel_interior search: the unvisited roots keep it as their network value, 0 where the root is terminal)."""
        env = self.env
        _lib.check(self._observe(C.byref(env._desc), C.byref(env._state), *self._root_obs_ptrs, env._stream()))
        priors, value = self._call(self._root_obs, self.trees)
        self._root_priors.copy_(priors)
        if self.gumbel_interior:
            torch.index_select(self.stats[:, _TERMINAL], 0, self._roots, out=self._root_term)
            torch.where(self._root_term != 0, self._root_zero, value, out=self._root_value)
            _lib.check(self._lib.snac_uct_set_priors_value(self.num_actions, _ptr(self.stats), self.rows, self.trees, _ptr(self._root_rows),
                                                           _ptr(self._root_priors), _ptr(self._root_value), 1, env._stream()))
            return
        _lib.check(self._lib.snac_uct_set_priors(self.num_actions, _ptr(self.stats), self.rows, self.trees, _ptr(self._root_rows),
                                                 _ptr(self._root_priors), 1, env._stream()))

    def set_root_priors(self, priors):
        """Root b's priors <- priors[b] ([B, A], stored as float32), whether the root has been visited or not: where a caller mixes
        exploration noise into the evaluator's root priors (root_priors())."""
        if self.evaluator is None:
            raise ValueError("priors belong to the PUCT search: give an evaluator")
        p = torch.as_tensor(priors, device=self.env.device)
        if tuple(p.shape) != (self.trees, self.num_actions):
            raise ValueError("priors must be [%d, %d]" % (self.trees, self.num_actions))
        with torch.cuda.device(self.env.device):
            self._root_priors.copy_(p.to(torch.float32))
            _lib.check(self._lib.snac_uct_set_priors(self.num_actions, _ptr(self.stats), self.rows, self.trees, _ptr(self._root_rows),
                                                     _ptr(self._root_priors), 0, self.env._stream()))

    @property
    def iterations(self):
        """Iterations enqueued since reset()."""
        return self._iteration

    # ---- the Gumbel root search (include/snac_hip.h, "Gumbel root") ---------------------------------------------------------------
    def _no_candidates(self):
        """A new root: no candidate set steers it (one torch op, no host synchronisation)."""
        if self.gumbel is not None:
            self.cand.zero_()
            self._gumbel_begun = False

    def _need_gumbel(self):
        if self.gumbel is None:
            raise ValueError("not a Gumbel search: give UCTSearch gumbel=m")

    def _candidates(self, mode, action=None):
        _lib.check(self._lib.snac_uct_gumbel_candidates(*self._cand_args, mode, self.gumbel, *self._cand_tail,
                                                        None if action is None else _ptr(action), self.env._stream()))

    def gumbel_scores(self, noise=True, generator=None, t=None):
        """[B, A] float32: log(root_priors()), plus a Gumbel(0, 1) sample -log(-log(U)) per entry with noise=True, U from torch.rand on the
        env's device (generator: a torch.Generator of that device).  A prior of 0 gives -inf: the action is never a candidate before
        one with a positive prior.  t (the caller's move counter): the scores in one launch instead, the noise from the counter RNG's
        stream 7 keyed by (env_id_base + b, a, t), so that they do not depend on the sharding or on a generator's state
        (snac_explore_gumbel_scores; include/snac_hip.h, "Exploration noise"); noise may then also be a [B] tensor (non-zero: that tree gets
        noise) and generator must be None.  No host synchronisation."""
        self._need_gumbel()
        if t is not None:
            return self._counter_scores(noise, generator, t)
        logits = torch.log(self.root_priors())
        if not noise:
            return logits
        u = torch.rand(logits.shape, dtype=torch.float32, device=self.env.device, generator=generator)
        return logits - torch.log(-torch.log(u))

    def _mask8(self, m):
        """A [B] mask tensor as contiguous uint8 on the env's device (non-zero: set); a bool or uint8 tensor there is taken as it is."""
        m = m.to(self.env.device).reshape(-1)
        if m.dtype == torch.bool:
            m = m.view(torch.uint8)
        elif m.dtype != torch.uint8:
            m = (m != 0).view(torch.uint8)
        return m.contiguous()

    def _counter_scores(self, noise, generator, t, out=None):
        """gumbel_scores(t=): snac_explore_gumbel_scores into `out` (None: a new [B, A] tensor)."""
        B = self.trees
        if generator is not None:
            raise ValueError("generator does not go with t: the counter RNG draws the noise")
        if isinstance(t, bool) or not isinstance(t, int):
            raise ValueError("t must be an integer: the caller's move counter")
        if torch.is_tensor(noise):
            if int(noise.numel()) != B:
                raise ValueError("noise must be a bool or a [%d] tensor" % B)
        elif not isinstance(noise, (bool, int)):
            raise ValueError("noise must be a bool or a [%d] tensor" % B)
        env, dev = self.env, self.env.device
        with torch.cuda.device(dev):
            if torch.is_tensor(noise):
                m = self._mask8(noise)
            else:
                m = None if noise else self._sample_all              # zeros: no tree gets noise
            if out is None:
                out = torch.empty((B, self.num_actions), dtype=torch.float32, device=dev)
            _lib.check(self._lib.snac_explore_gumbel_scores(*self._pick_args, _ptr(m), t & 0xFFFFFFFF, _ptr(out), env._stream()))
        return out

    def add_dirichlet_noise(self, alpha, eps=0.25, t=0, mask=None, attempts=16):
        """AlphaZero's root noise, in place: the priors of root b <- (1 - eps) * priors + eps * eta_b, eta_b ~ Dirichlet(alpha) over the
        actions with a positive prior, drawn from the counter RNG's stream 6 keyed by (env_id_base + b, a, t) -- t: the caller's move
        counter -- so that a shard of the trees draws what they draw in the whole batch (snac_explore_root_dirichlet; include/snac_hip.h,
        "Exploration noise").  PUCT only.  mask: None or a [B] tensor (non-zero: that tree gets noise); attempts: the bound of the Gamma
        draws' rejection loop, 1 .. 32.  A root whose priors hold a NaN, an infinity, a negative or no positive entry is left as it is
        and counted in noise_bad_rows (int32 [1] on the device).  One launch on the env's stream, no host synchronisation."""
        if self.evaluator is None:
            raise ValueError("priors belong to the PUCT search: give an evaluator")
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 2.0 ** -10 <= alpha <= 2.0 ** 10:
            raise ValueError("alpha must be a number in [2^-10, 2^10]")
        if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 <= eps <= 1.0:
            raise ValueError("eps must be a number in [0, 1]")
        if isinstance(attempts, bool) or not isinstance(attempts, int) or not 1 <= attempts <= 32:
            raise ValueError("attempts must be an integer in [1, 32]")
        if isinstance(t, bool) or not isinstance(t, int):
            raise ValueError("t must be an integer: the caller's move counter")
        if mask is not None and (not torch.is_tensor(mask) or int(mask.numel()) != self.trees):
            raise ValueError("mask must be None or a [%d] tensor" % self.trees)
        env = self.env
        with torch.cuda.device(env.device):
            m = None if mask is None else self._mask8(mask)
            _lib.check(self._lib.snac_explore_root_dirichlet(*self._pick_args, _ptr(m), t & 0xFFFFFFFF, float(alpha), float(eps), attempts,
                                                             _ptr(self.noise_bad_rows), env._stream()))

    def gumbel_begin(self, scores):
        """Candidate sets for this move: cand[b] <- the min(m, A) root actions of tree b with the largest scores[b] ([B, A], stored as
        float32: g(a) + logit(a), gumbel_scores(); ties to the lowest a, NaN as -inf), none at a terminal root (snac_uct_gumbel_candidates,
        BEGIN).  The scores stay with the search for the halvings and the final move."""
        self._need_gumbel()
        s = torch.as_tensor(scores, device=self.env.device)
        if tuple(s.shape) != (self.trees, self.num_actions):
            raise ValueError("scores must be [%d, %d]" % (self.trees, self.num_actions))
        with torch.cuda.device(self.env.device):
            self._gscores.copy_(s)
            self._candidates(0)
        self._gumbel_begun = True

    def gumbel_run(self, iterations):
        """Enqueue `iterations` iterations split by gumbel_schedule(iterations, min(m, A)) into sequential-halving phases: the phase's
        candidates are visited in turn (iteration i of a phase sends its K paths to candidates i * K, i * K + 1, ... modulo their
        number), and before every phase but the first the candidates are halved by g + logit + sigma(q) (snac_uct_gumbel_candidates,
        HALVE).  Needs gumbel_begin() since the last reset() / advance() / restart().  No host synchronisation."""
        n = int(iterations)
        if self._iteration + n > self.max_iterations:
            raise ValueError("%d iterations after %d exceed max_iterations = %d" % (n, self._iteration, self.max_iterations))
        self._gumbel_run(n)

    def _gumbel_run(self, n):
        """gumbel_run() without the budget check (SelfPlay bounds the visit counts per episode)."""
        self._need_gumbel()
        if not self._gumbel_begun:
            raise ValueError("gumbel_run() needs gumbel_begin() since the last reset(), advance() or restart()")
        plan = gumbel_schedule(n, min(self.gumbel, self.num_actions))
        K = self.paths
        with torch.cuda.device(self.env.device):
            for halve, i in plan:
                if halve:
                    self._candidates(1)
                self._select(i * K)
                self._edges()
                self._evaluate()
                self._backup()
                self._set_priors()

    def gumbel_actions(self, out=None):
        """[B] int8: the move of the Gumbel search, the remaining candidate with the largest g + logit + sigma(q) (ties to the lowest; a
        tree without candidates: the most-visited action as best_actions(), 0 without visits): snac_uct_gumbel_candidates, PICK.
        out: a contiguous int8 [B] tensor on the env's device to write into."""
        self._need_gumbel()
        dev = self.env.device
        if out is None:
            out = torch.empty(self.trees, dtype=torch.int8, device=dev)
        elif (not torch.is_tensor(out) or tuple(out.shape) != (self.trees,) or out.dtype != torch.int8 or not out.is_contiguous()
              or out.device != dev):
            raise ValueError("out must be a contiguous int8 [%d] tensor on %s" % (self.trees, dev))
        with torch.cuda.device(dev):
            self._candidates(2, out)
        return out

    def improved_policy(self):
        """[B, A] float32: the policy target of the Gumbel search, softmax(logits + sigma(completed q)) in float64 torch ops.  logits =
        log(root priors); q of a visited root child (N_a > 0) is its normalised W_a / N_a, q of every other action the normalised
        sum W_visited / sum N_visited; sigma(q) = (c_visit + max_a N_a) * c_scale * q.  A root without a visited child gives its
        normalised priors.  The value given to unvisited actions simplifies the paper's v_mix (Danihelka et al. 2022, eq. 33), which
        also mixes in the root's network value weighted by the priors: that value is not stored in the tree, so the visit-weighted
        mean of the visited children's q stands in for it.  A gumbel_interior search keeps that value, and returns instead the
        improved policy of snac_uct_improved_policy for the roots, the one its selection uses, with the paper's v_mix ("Gumbel
        interior" in include/snac_hip.h; a terminal root: zeros).  No host synchronisation."""
        self._need_gumbel()
        A = self.num_actions
        if self.gumbel_interior:
            pi = torch.empty((self.trees, A), dtype=torch.float32, device=self.env.device)
            with torch.cuda.device(self.env.device):
                _lib.check(self._lib.snac_uct_improved_policy(*self._policy_args, _ptr(pi), self.env._stream()))
            return pi
        r = self.stats[self._roots]
        child, N = r[:, _CHILD][:, :A], r[:, _CHILD_VISITS][:, :A]
        W = r[:, _CHILD_VALUE].contiguous().view(torch.float64)[:, :A]
        visited = (child >= 0) & (N > 0)
        zero = torch.zeros_like(W)
        n = torch.where(visited, N.to(torch.float64), zero)
        w = torch.where(visited, W, zero)
        sum_n = n.sum(1, keepdim=True)
        any_visit = sum_n > 0
        one = torch.ones_like(sum_n)
        mixed = w.sum(1, keepdim=True) / torch.where(any_visit, sum_n, one)      # every unvisited action's q
        q = torch.where(visited, w / torch.where(visited, n, one), mixed)
        lo, hi = self.q_bounds[:, 0:1], self.q_bounds[:, 1:2]
        on = hi > lo
        q = torch.where(on, (q - lo) / torch.where(on, hi - lo, one), q)
        sig = (self.gumbel_c_visit + n.max(1, keepdim=True).values) * self.gumbel_c_scale * q
        sig = torch.where(any_visit, sig, zero)
        logits = torch.log(self.root_priors().to(torch.float64))
        return torch.softmax(logits + sig, 1).to(torch.float32)

    # ---- readers ----------------------------------------------------------------------------------------------------------
    def root_visits(self):
        """[B, A] int32: the visits of each root child (0 where untried)."""
        return self.stats[self._roots][:, _CHILD_VISITS][:, :self.num_actions].clone()

    def root_q(self):
        """[B, A] float64: W / N of each root child, NaN where untried."""
        r = self.stats[self._roots]
        w = r[:, _CHILD_VALUE].contiguous().view(torch.float64)[:, :self.num_actions]
        q = w / r[:, _CHILD_VISITS][:, :self.num_actions].to(torch.float64)
        return torch.where(r[:, _CHILD][:, :self.num_actions] >= 0, q, torch.full_like(q, float("nan")))

    def root_priors(self):
        """[B, A] float32: the priors of each root (zero in a rollout search)."""
        return self.stats[self._roots][:, _PRIOR:_PRIOR + self.num_actions].contiguous().view(torch.float32)

    def best_actions(self):
        """[B] int64: the most-visited root action, ties to the lowest."""
        return torch.argmax(self.root_visits(), dim=1)

    def q_bounds_of_trees(self):
        """[B, 2] float64: (lo, hi) of each tree's mean values below the root, (+inf, -inf) while there is none (q_normalise=True only)."""
        if not self.q_normalise:
            raise ValueError("bounds belong to a search with q_normalise=True")
        return self.q_bounds.clone()

    def tree_sizes(self):
        """[B] int32: nodes used by each tree (the root counts)."""
        return self._used.clone()

    # views over all node rows (scratch rows included), decoded from snac_uct_node
    @property
    def children(self):
        return self.stats[:, _CHILD][:, :self.num_actions]

    @property
    def parent(self):
        return self.stats[:, _PARENT]

    @property
    def action(self):
        return self.stats[:, _ACTION]

    @property
    def terminal(self):
        return self.stats[:, _TERMINAL] != 0

    @property
    def visits(self):
        return self.stats[:, _VISITS]

    @property
    def value_sum(self):
        return self.stats[:, _VALUE_SUM].view(torch.float64)[:, 0]

    @property
    def reward(self):
        return self.stats[:, _REWARD].view(torch.float32)[:, 0]

    @property
    def prior(self):
        """[rows, A] float32: the PUCT priors (zero in a rollout search)."""
        return self.stats[:, _PRIOR:_PRIOR + self.num_actions].view(torch.float32)

    @property
    def net_values(self):
        """[rows] float64: the value the evaluator gave for each node's state, 0 at a terminal node (a gumbel_interior search; zero in
        every other)."""
        return self.stats[:, _NET_VALUE:_NET_VALUE + 2].view(torch.float64)[:, 0]
