"""Self-play on the device with a ring of training targets: the search side's counterpart of ReplayRing (snac_uct_pick_moves /
snac_uct_restart / snac_uct_returns: include/snac_hip.h, "Self-play"; snac_amd/csrc/k_uct_play.hip; snac_uct_save_roots /
snac_uct_store_targets / snac_uct_returns_nstep: "Reanalyse"; snac_amd/csrc/k_uct_reanalyse.hip).

Tree b of a UCTSearch plays env row b.  play(moves, iterations) enqueues, per move and for all B trees at once: the search, the roots'
observation rows, a move drawn from the root's visit counts (in proportion to them for the first `sample_moves` moves of an episode,
the most-visited one after that), the re-rooting, and -- for the trees whose episode ended -- a reset of their env rows and a new
root.  Everything lands in ring slot `head`; nothing crosses the bus and the host never waits:

    env = BatchedDMPEnv(2, True, 64, seed=1); env.reset()
    search = UCTSearch(env, 2048, 0, 0.99, c=1.25, paths=16, evaluator=fn, max_iterations=(env.total_step + 1) * 32)
    search.reset()
    play = SelfPlay(search, capacity_moves=512, sample_moves=10)
    for step in range(steps):
        play.play(16, iterations=32)
        play.targets()                               # z: discounted returns to the end of each episode, bootstrapped at the ring's end
        batch = play.sample(1024)                    # obs float32, pi, z, value, action, reward, done
        loss = cross_entropy(policy(batch["obs"]), batch["pi"]) + mse(value(batch["obs"]), batch["z"]); ...

A search built with q_normalise=True plays the same way: advance() and restart() keep its q bounds (snac_amd/uct.py), nothing here
knows them.

SelfPlay(search, ..., gumbel=True) on a UCTSearch(gumbel=m) plays by the Gumbel root search ("Gumbel root" in include/snac_hip.h) in place
of PUCT at the root and the visit counts: per move gumbel_begin() on log-priors with Gumbel noise (for the first `sample_moves` moves
of an episode; without noise after that), gumbel_run(iterations), action = gumbel_actions(), pi = improved_policy(); value, reward, done
and the re-rooting are as above.  Exploration comes from the Gumbel noise: there is no root_noise hook in this mode.

Exploration from the counter RNG ("Exploration noise" in include/snac_hip.h): dirichlet=(alpha, eps) mixes AlphaZero's Dirichlet noise
into the roots' priors before every move's search, temperature=T draws the sampled moves in proportion to N ** (1 / T), and
counter_noise=True (with gumbel=True) takes the Gumbel noise from it too.  Each is one launch keyed by (env_id_base + b, the move
counter), so a sharded run plays exactly the whole batch's moves; without them play() enqueues what it always did.

Reanalyse: a position's pi and value come from a search guided by the network as it was when the move was played, and at a few dozen
iterations per move they age quickly, while replaying costs far more than searching again.  SelfPlay(..., keep_states=True) also keeps
each move's root record, a complete state (`state`: 128 bytes per ring entry for 1D and 2D, 896 for 3D), and reanalyse(search, iterations)
searches R stored positions again with a second UCTSearch over the same env -- any trees = R, its own evaluator: the latest network --
and overwrites their pi and value (`refreshed` counts how often).  targets(td_steps=n) then builds MuZero's n-step value target
z_t = sum_{k<n} gamma^k r_{t+k} + gamma^n v_{t+n} from the ring's values, so that fresh root values reach z:

    play = SelfPlay(search, capacity_moves=512, sample_moves=10, keep_states=True)
    again = UCTSearch(env, 512, 0, 0.99, c=1.25, paths=4, evaluator=latest, trees=256, max_iterations=32)
    for step in range(steps):
        play.play(16, iterations=32)
        play.reanalyse(again, 32)                    # 256 entries drawn without replacement on the device; no host synchronisation
        play.targets(td_steps=5)

The ring, over moves (slot = move % capacity_moves), every tensor on the env's device:
    obs [cap, B, D] env.obs_dtype   pi [cap, B, A] float32   value [cap, B] float32   action [cap, B] int8
    reward [cap, B] float32   done [cap, B] uint8   move [cap, B] int32 (the move's index inside its episode)   z [cap, B] float32
    keep_states=True:   state [cap, B, record_bytes] uint8 (the root's record when the move was chosen)   refreshed [cap, B] int32

Prioritised replay: SelfPlay(..., prioritized=True) keeps a PriorityTree (snac_amd/priority.py; include/snac_hip.h, "Prioritised
replay") over the capacity_moves * trees entries, flat = slot * trees + b.  Every move written gets the largest priority seen so far
(one more small entry point per move); sample(batch, prioritized=True, beta=...) draws in proportion to the priorities and returns
`index`, `prob` and the importance weights `weight`; update_priorities(index, priority) stores new ones, e.g. MuZero's
(value - z).abs() ** alpha; reanalyse(..., prioritized=True) draws its entries from the same distribution.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import ptr as _ptr


class SelfPlay:
    def __init__(self, search, capacity_moves, sample_moves=0, gamma=None, root_noise=None, gumbel=False, generator=None, keep_states=False,
                 prioritized=False, priority_scale_log2=16, dirichlet=None, temperature=None, counter_noise=False):
        """search: a UCTSearch with one tree per env row (reset() by the caller); capacity_moves: ring slots; sample_moves: the moves of
        an episode drawn in proportion to the visits (the rest: argmax); gamma: of the value targets (default: the search's);
        root_noise: PUCT only, priors [B, A] -> priors [B, A], applied to the roots before every move's search (exploration noise is the
        caller's).  gumbel=True (a UCTSearch(gumbel=m), root_noise None): the moves and policy targets of the Gumbel root search, with
        Gumbel noise in the first sample_moves moves of an episode drawn from `generator` (a torch.Generator of the env's device; None:
        the default one).  keep_states=True: the ring also keeps every move's root record (`state`: 128 bytes per entry for 1D and 2D,
        896 for 3D, capacity_moves * trees entries) and a count of its reanalyses (`refreshed`), which reanalyse() needs; one more
        launch per move.  prioritized=True: a PriorityTree over the capacity_moves * trees entries (flat = slot * trees + b), seeded from
        the env's seed, with priority_scale_log2 as its scale_log2; every move played gets the largest priority seen so far.
        Exploration from the counter RNG (include/snac_hip.h, "Exploration noise"; one launch each, independent of the sharding):
        dirichlet=(alpha, eps) (PUCT; not with root_noise or gumbel=True): UCTSearch.add_dirichlet_noise(alpha, eps, t=moves) before
        every move's search; temperature=T (a number >= 0; not with gumbel=True): the first sample_moves moves of an episode are drawn
        in proportion to N ** (1 / T) in place of N; counter_noise=True (gumbel=True, generator None): the Gumbel noise comes from
        UCTSearch.gumbel_scores(noise=mask, t=moves), one launch in place of two score tensors and a torch.where."""
        if not isinstance(counter_noise, bool):
            raise ValueError("counter_noise must be a bool")
        if dirichlet is not None:
            if callable(root_noise) or gumbel is True:
                raise ValueError("dirichlet does not go with a root_noise callable or with gumbel=True")
            if (not isinstance(dirichlet, (tuple, list)) or len(dirichlet) != 2
                    or any(isinstance(x, bool) or not isinstance(x, (int, float)) for x in dirichlet)
                    or not 2.0 ** -10 <= dirichlet[0] <= 2.0 ** 10 or not 0.0 <= dirichlet[1] <= 1.0):
                raise ValueError("dirichlet must be (alpha in [2^-10, 2^10], eps in [0, 1])")
            if search.evaluator is None:
                raise ValueError("dirichlet noise belongs to the PUCT search: give the search an evaluator")
            dirichlet = (float(dirichlet[0]), float(dirichlet[1]))
        if temperature is not None:
            if gumbel is True:
                raise ValueError("temperature does not go with gumbel=True: the Gumbel search plays its survivor")
            if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not temperature >= 0:
                raise ValueError("temperature must be a number >= 0")
            temperature = float(temperature)
        if counter_noise and (gumbel is not True or generator is not None):
            raise ValueError("counter_noise=True belongs to gumbel=True with generator=None")
        self.dirichlet, self.temperature, self.counter_noise = dirichlet, temperature, counter_noise
        if not isinstance(keep_states, bool):
            raise ValueError("keep_states must be a bool")
        if not isinstance(prioritized, bool):
            raise ValueError("prioritized must be a bool")
        if isinstance(priority_scale_log2, bool) or not isinstance(priority_scale_log2, int) or not 0 <= priority_scale_log2 <= 31:
            raise ValueError("priority_scale_log2 must be an integer in [0, 31]")
        self.keep_states = keep_states
        if not isinstance(gumbel, bool):
            raise ValueError("gumbel must be a bool")
        if gumbel and getattr(search, "gumbel", None) is None:
            raise ValueError("gumbel=True needs a Gumbel search: UCTSearch(gumbel=m)")
        if gumbel and root_noise is not None:
            raise ValueError("root_noise does not go with gumbel=True: the Gumbel noise explores")
        if generator is not None and not gumbel:
            raise ValueError("generator belongs to gumbel=True")
        self.gumbel, self.generator = gumbel, generator
        self.cap, self.sample_moves = int(capacity_moves), int(sample_moves)
        if self.cap < 1 or self.cap != capacity_moves:
            raise ValueError("capacity_moves must be an integer >= 1")
        if self.sample_moves < 0 or self.sample_moves != sample_moves:
            raise ValueError("sample_moves must be an integer >= 0")
        if root_noise is not None and not callable(root_noise):
            raise ValueError("root_noise must be callable: priors [B, A] -> priors [B, A]")
        if root_noise is not None and search.evaluator is None:
            raise ValueError("root_noise belongs to the PUCT search: give the search an evaluator")
        self.gamma = float(search.gamma if gamma is None else gamma)
        if self.gamma != self.gamma or self.gamma in (float("inf"), float("-inf")):
            raise ValueError("gamma must be finite")
        env = search.env
        if search.trees != env.num_envs:
            raise ValueError("%d trees, %d env rows: self-play ties tree b to env row b" % (search.trees, env.num_envs))
        self.search, self.env, self.root_noise = search, env, root_noise
        B, A, dev = search.trees, search.num_actions, env.device
        if B * self.cap > 0x7FFFFFFF:
            raise ValueError("trees * capacity_moves entries exceed int32")
        cap = self.cap
        self.obs = torch.zeros((cap, B, env.obs_dim), dtype=env.obs_dtype, device=dev)
        self.pi = torch.zeros((cap, B, A), dtype=torch.float32, device=dev)
        self.value, self.reward, self.z = (torch.zeros((cap, B), dtype=torch.float32, device=dev) for _ in range(3))
        self.action = torch.zeros((cap, B), dtype=torch.int8, device=dev)
        self.done = torch.zeros((cap, B), dtype=torch.uint8, device=dev)
        self.move = torch.zeros((cap, B), dtype=torch.int32, device=dev)
        self.head, self.moves = 0, 0                                 # the next slot; moves played since construction
        self._move = torch.zeros(B, dtype=torch.int32, device=dev)   # each tree's move inside its episode
        self._next = torch.zeros(B, dtype=torch.int32, device=dev)
        self._zero = torch.zeros(B, dtype=torch.int32, device=dev)
        self._greedy = torch.zeros(B, dtype=torch.uint8, device=dev)
        self._noisy = torch.zeros((B, 1), dtype=torch.bool, device=dev)
        self._boot = torch.zeros(B, dtype=torch.float32, device=dev)
        self._observe = getattr(search._lib, search.pool.OBSERVE)
        self._root_rows = search._adv_src                            # int32 [B]: row b * cap
        self.state = self.refreshed = None
        if keep_states:
            P = search.pool
            self.state = torch.zeros((cap, B, P.WORDS * 4), dtype=torch.uint8, device=dev)
            self.refreshed = torch.zeros((cap, B), dtype=torch.int32, device=dev)
            assert self.state.data_ptr() % 128 == 0
            self._save_args = (B, search.nodes_per_tree, _ptr(P.records), P.WORDS * 4, P.rows)
        self.tree = None
        if prioritized:
            from .priority import MAX_ENTRIES, PriorityTree

            if B * cap > MAX_ENTRIES:
                raise ValueError("trees * capacity_moves entries exceed what a PriorityTree holds (2^31 - 64)")
            self.tree = PriorityTree(B * cap, dev, scale_log2=priority_scale_log2, seed=env.seed, sampler_id=env.env_id_base * cap)

    def _check_budget(self, iterations):
        s = self.search
        need = (self.env.total_step + 1) * iterations
        if s.max_iterations < need:
            raise ValueError("max_iterations = %d is below (total_step + 1) * iterations = %d: a tree is restarted after at most "
                             "total_step + 1 moves, and its visit counts must stay inside the search's tables" % (s.max_iterations, need))

    def play(self, moves, iterations):
        """Enqueue `moves` moves of every tree with `iterations` search iterations before each, into the ring; no host synchronisation."""
        moves, n = int(moves), int(iterations)
        if moves < 0 or n < 0:
            raise ValueError("moves and iterations must be >= 0")
        self._check_budget(n)
        s, env, P = self.search, self.env, self.search.pool
        B = s.trees
        with torch.cuda.device(env.device):
            for _ in range(moves):
                h = self.head
                if self.gumbel:
                    self._gumbel_search(n)
                else:
                    if self.root_noise is not None:
                        s.set_root_priors(self.root_noise(s.root_priors()))
                    if self.dirichlet is not None:
                        s.add_dirichlet_noise(*self.dirichlet, t=self.moves)
                    s._run(n)
                _lib.check(self._observe(C.byref(env._desc), C.byref(env._state), _ptr(P.records), P.rows, B, _ptr(self._root_rows),
                                         _ptr(self.obs[h]), env._stream()))
                if self.keep_states:                                 # the roots' records, before the advance moves them on
                    _lib.check(s._lib.snac_uct_save_roots(*self._save_args, _ptr(self.state[h]), env._stream()))
                    self.refreshed[h].zero_()
                if self.gumbel:
                    s.gumbel_actions(out=self.action[h])
                    self.pi[h].copy_(s.improved_policy())
                    s._pick(None, 0, None, None, self.value[h])      # the root's W / N
                else:
                    torch.ge(self._move, self.sample_moves, out=self._greedy.view(torch.bool))
                    s._pick(self._greedy, self.moves, self.action[h], self.pi[h], self.value[h], temperature=self.temperature)
                s._advance_into(self.action[h], self.reward[h], self.done[h], prime=False)   # restart() primes every unvisited root
                self.move[h].copy_(self._move)
                env.reset(mask=self.done[h], want_obs=False)         # the finished trees' env rows: the next episode (and its plan)
                s.restart(self.done[h])
                torch.add(self._move, 1, out=self._next)
                torch.where(self.done[h].view(torch.bool), self._zero, self._next, out=self._move)
                if self.tree is not None:                            # the slot's new positions: the largest priority seen so far
                    self.tree.fill(h * B, B)
                self.head = (h + 1) % self.cap
                self.moves += 1

    def _gumbel_search(self, n):
        """A move's Gumbel root search: candidates from noisy scores in the first sample_moves moves of a tree's episode, from the
        log-priors alone after that (one torch.where of the two), then the sequential-halving iterations."""
        s = self.search
        torch.lt(self._move.view(-1, 1), self.sample_moves, out=self._noisy)
        if self.counter_noise:                                       # the same scores in one launch, the noise from the counter RNG
            s._counter_scores(self._noisy, None, self.moves, out=s._gscores)
            s._candidates(0)
            s._gumbel_begun = True
        else:
            s.gumbel_begin(torch.where(self._noisy, s.gumbel_scores(True, self.generator), s.gumbel_scores(False)))
        s._gumbel_run(n)

    # ---- the ring ---------------------------------------------------------------------------------------------------------
    def valid_moves(self):
        """Slots that hold a move."""
        return min(self.moves, self.cap)

    def __len__(self):
        """Number of addressable samples (move, tree)."""
        return self.valid_moves() * self.search.trees

    def slots(self):
        """Ring slots that hold a move, oldest first (int64 tensor on the device)."""
        v = self.valid_moves()
        return (torch.arange(v, device=self.env.device) + (self.head - v) % self.cap) % self.cap

    def targets(self, bootstrap=True, td_steps=None):
        """Fill z for the valid slots (snac_uct_returns): per tree, from the newest move back, g = reward + (done ? 0 : gamma * g) in
        float64, z = float32(g).  g starts as the value of the tree's current root (pick_moves' value: W / N, 0 before any iteration)
        with bootstrap=True -- the episode goes on beyond the ring -- and as 0 with bootstrap=False.  td_steps=n >= 1: the n-step target
        instead (snac_uct_returns_nstep): the same recurrence over the n moves from each slot on, started from the ring's `value` n
        moves later (what reanalyse() refreshes), or from the bootstrap where the ring ends first; n >= valid_moves() is the default's
        z bit for bit.  No host synchronisation."""
        if td_steps is not None and (isinstance(td_steps, bool) or td_steps != int(td_steps) or int(td_steps) < 1):
            raise ValueError("td_steps must be None or an integer >= 1")
        s, env = self.search, self.env
        v = self.valid_moves()
        boot = None
        if bootstrap and v:
            s._pick(None, 0, None, None, self._boot)
            boot = self._boot
        ring = (s.trees, self.cap, (self.head - v) % self.cap, v)
        with torch.cuda.device(env.device):
            if td_steps is None:
                _lib.check(s._lib.snac_uct_returns(*ring, self.gamma, _ptr(self.reward), _ptr(self.done), _ptr(boot), _ptr(self.z), env._stream()))
            else:
                _lib.check(s._lib.snac_uct_returns_nstep(*ring, min(int(td_steps), 0x7FFFFFFF), self.gamma, _ptr(self.reward), _ptr(self.done),
                                                         _ptr(self.value), _ptr(boot), _ptr(self.z), env._stream()))
        return self.z

    def reanalyse(self, search, iterations, index=None, generator=None, check=True, prioritized=False):
        """Search R = search.trees stored positions again and overwrite their targets (include/snac_hip.h, "Reanalyse").  search: a second
        UCTSearch over the same env with an evaluator -- the latest network -- and the same actions; any trees = R <= len(self),
        nodes_per_tree and paths; iterations <= its max_iterations.  index: R distinct flat entries slot * trees + b in valid slots
        (an integer tensor; check=True validates it with a host read), or None: drawn without replacement on the device from
        `generator` (a torch.Generator of the env's device; None: the default one).  Enqueues search.load_roots() of the entries'
        stored records, the search (a gumbel=m search: gumbel_begin() on the log-priors without noise and the halving schedule; any
        other: the PUCT iterations) and snac_uct_store_targets: pi <- the improved policy or the visit distribution, value <- the
        root's W / N, refreshed += 1, at the indexed entries only.  With check=False or index=None there is no host synchronisation.
        prioritized=True (a SelfPlay(prioritized=True), index None): the R entries are drawn from the priority tree instead, MuZero's
        Reanalyse distribution.  The tree draws with replacement and snac_uct_store_targets needs distinct entries, so the draws are
        sorted on the device and every repeat is marked -1: its tree searches entry 0 and stores nothing, and fewer than R entries
        are refreshed.  An empty tree (every priority 0) refreshes nothing.
        Returns the index (int64 [R], on the device; -1 at a marked repeat)."""
        if not isinstance(prioritized, bool):
            raise ValueError("prioritized must be a bool")
        if prioritized and self.tree is None:
            raise ValueError("prioritized=True needs the priority tree: SelfPlay(..., prioritized=True)")
        if prioritized and index is not None:
            raise ValueError("prioritized=True draws the entries itself: index must be None")
        if not self.keep_states:
            raise ValueError("reanalyse() needs the stored root records: SelfPlay(..., keep_states=True)")
        if search is self.search:
            raise ValueError("reanalyse() needs a second UCTSearch over the same env: the playing search keeps its trees")
        if search.env is not self.env:
            raise ValueError("the reanalysing search must be built on the env of the playing search (its plan table and rules)")
        if search.evaluator is None:
            raise ValueError("the reanalysing search needs an evaluator")
        if search.num_actions != self.search.num_actions:
            raise ValueError("the reanalysing search must have %d actions" % self.search.num_actions)
        R, n = search.trees, int(iterations)
        if R > len(self):
            raise ValueError("%d trees to reanalyse, %d entries in the ring" % (R, len(self)))
        if n < 0 or n != iterations or n > search.max_iterations:
            raise ValueError("iterations must be an integer in [0, max_iterations = %d]" % search.max_iterations)
        B, cap, dev = self.search.trees, self.cap, self.env.device
        v = self.valid_moves()
        first = (self.head - v) % cap
        if prioritized:
            flat = torch.sort(self.tree.sample(R)[0]).values
            flat[1:].masked_fill_(flat[1:] == flat[:-1], -1)
        elif index is None:                                          # the R largest of v * B uniform draws: distinct entries
            i = torch.topk(torch.rand(v * B, device=dev, generator=generator), R).indices
            flat = ((first + i // B) % cap) * B + i % B
        else:
            if not torch.is_tensor(index) or int(index.numel()) != R:
                raise ValueError("index must be a tensor of %d entries" % R)
            if index.is_floating_point() or index.is_complex() or index.dtype == torch.bool:
                raise ValueError("index must be integers")
            flat = index.to(dev).reshape(-1).to(torch.int64)
            if check:
                if int(flat.min()) < 0 or int(flat.max()) >= cap * B or int(((flat // B - first) % cap).max()) >= v:
                    raise ValueError("index must name entries slot * %d + b of valid slots" % B)
                if int(torch.unique(flat).numel()) != R:
                    raise ValueError("index must name distinct entries")
        idx = flat.to(torch.int32)
        search.load_roots(self.state.view(cap * B, -1), idx)
        policy = None
        if search.gumbel is not None:
            search.gumbel_begin(search.gumbel_scores(False))
            search._gumbel_run(n)
            policy = search.improved_policy()
        else:
            search._run(n)
        with torch.cuda.device(dev):
            _lib.check(search._lib.snac_uct_store_targets(search.num_actions, _ptr(search.stats), search.rows, R, search.nodes_per_tree, _ptr(idx),
                                                          cap * B, _ptr(policy), _ptr(self.pi), _ptr(self.value), _ptr(self.refreshed),
                                                          self.env._stream()))
        return flat

    def sample(self, batch, generator=None, prioritized=False, beta=0.4, stratified=True):
        """Uniform minibatch over the valid (move, tree) pairs -> dict on the device: obs float32 [n, D], pi [n, A], z, value, reward
        float32 [n], action int64 [n], done bool [n]; with keep_states=True also refreshed int32 [n].  One flat index and 1-D gathers
        (ReplayRing.gather has the measurement).  prioritized=True (a SelfPlay(prioritized=True); generator None): the entries are
        drawn from the priority tree, with replacement, stratified over the total unless stratified=False, and three keys are added:
        index int64 [n] (flat = slot * trees + b, what update_priorities() takes), prob float32 [n] and the importance weights
        weight = (len(self) * prob) ** -beta / their largest over the batch (beta = 0: all ones)."""
        v = self.valid_moves()
        if v == 0:
            raise ValueError("the ring is empty")
        if not isinstance(prioritized, bool):
            raise ValueError("prioritized must be a bool")
        B = self.search.trees
        if prioritized:
            if self.tree is None:
                raise ValueError("prioritized=True needs the priority tree: SelfPlay(..., prioritized=True)")
            if generator is not None:
                raise ValueError("generator does not go with prioritized=True: the tree draws with the counter RNG")
            beta = float(beta)
            if beta != beta or beta < 0 or beta == float("inf"):
                raise ValueError("beta must be a finite number >= 0")
            flat, prob = self.tree.sample(int(batch), stratified)
        else:
            i = torch.randint(0, v * B, (int(batch),), device=self.env.device, generator=generator)
            flat = (((self.head - v) % self.cap + i // B) % self.cap) * B + i % B
        out = dict(obs=self.obs.view(self.cap * B, -1)[flat].to(torch.float32), pi=self.pi.view(self.cap * B, -1)[flat],
                   z=self.z.view(-1)[flat], value=self.value.view(-1)[flat], action=self.action.view(-1)[flat].long(),
                   reward=self.reward.view(-1)[flat], done=self.done.view(-1)[flat].bool())
        if self.keep_states:
            out["refreshed"] = self.refreshed.view(-1)[flat]
        if prioritized:
            w = (prob * float(len(self))) ** -beta
            out["index"], out["prob"], out["weight"] = flat, prob, w / w.max()
        return out

    def update_priorities(self, index, priority):
        """New priorities for sampled entries (PriorityTree.update): index [n], the `index` of sample(prioritized=True); priority [n],
        floats >= 0 -- the caller applies alpha, e.g. (value - z).abs() ** alpha.  Where an index repeats, the largest priority wins.
        An entry that play() overwrote between sample() and update_priorities() receives the stale priority: the usual behaviour of
        prioritised replay, harmless because the next update of that entry corrects it.  No host synchronisation."""
        if self.tree is None:
            raise ValueError("update_priorities() needs the priority tree: SelfPlay(..., prioritized=True)")
        self.tree.update(index, priority)
