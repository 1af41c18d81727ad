"""ReplayRing: the replay memory of the reference's DQN / DRQN scripts, kept on the GPU.

The reference appends one python tuple (s, a, r, s', env_plan) per env-step to a deque and rebuilds float32 minibatches
on the host (script/DQN/2d/DQN_2d_dynamic.py:122-124 store_memory, :184-199 prefill loop, :145-166 minibatch assembly).
Here the fused rollout writes its outputs straight into a ring over ticks,

    obs[cap, N, D]   reward[cap, N]   done[cap, N]   action[cap, N]   step_size[cap, N]   plan_idx[cap, N]   first[cap, N]

and a transition is addressed by (slot, env): s' = obs[slot, env]; s = obs[slot - 1, env], or the reset observation
when first[slot, env] (the reference takes prev_state from env.reset() there); plan = the plan row in effect.  Nothing
is stored twice and nothing crosses PCIe; sample() gathers float32 minibatches with snac_replay_gather.

Prioritised replay (the reference's script/Rainbow keeps a segment tree on the host): ReplayRing(..., prioritized=True) keeps a
PriorityTree (snac_amd/priority.py; include/snac_hip.h, "Prioritised replay") over the cap * N entries, flat = slot * N + env.
collect() gives every transition it writes the largest priority seen so far; sample(batch, prioritized=True, beta=...) draws in
proportion to the priorities and adds slot, env, index, prob and the importance weights `weight`; update_priorities(index, |td|)
stores new ones.

Walks along an env's column (include/snac_hip.h, "n-step transitions and episode windows"): gather_nstep() / sample(n_step=, gamma=)
give Rainbow's multi-step transition (s, the discounted sum of up to n rewards, the row to bootstrap from and its discount), cut at the
episode's end and at the newest slot; gather_windows() / sample_windows() give DRQN's windows of up to L consecutive tuples of one
episode that END at the drawn transition, valid steps first, with a mask.  One launch each, no torch index kernel, no host
synchronisation.
"""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import ptr as _ptr


def _walk_steps(name, v):
    """n of an n-step transition / L of a window: an integer in [1, 64] (a wave's lanes hold the steps of a walk)"""
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 64:
        raise ValueError("%s must be an integer in [1, 64]" % name)
    return v


def _walk_gamma(gamma):
    if gamma is None or isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not math.isfinite(gamma):
        raise ValueError("n_step needs gamma: a finite number")
    return float(gamma)


def _pairs(env, slot, env_index):
    """(slot, env) pairs as the gather entry points take them: two contiguous int32 tensors on the env's device, and their count B"""
    slot = torch.as_tensor(slot, device=env.device).to(torch.int32).contiguous()
    env_index = torch.as_tensor(env_index, device=env.device).to(torch.int32).contiguous()
    return slot, env_index, int(slot.numel())


def _outputs(empty, env):
    """new(*shape, dtype=float32): an output of a gather call on the env's device, allocated by `empty`, the calling module's torch.empty"""
    return lambda *shape, dtype=torch.float32: empty(shape, dtype=dtype, device=env.device)


def _with_plan(env, out, plan):
    """The dict of a gather with the plan in its shape, [B, 20, 20] (1D: [B, 30]), where one was asked for"""
    if plan is not None:
        out["plan"] = plan if env.kind == 1 else plan.view(plan.shape[0], 20, 20)
    return out


class ReplayRing:
    def __init__(self, env, capacity_ticks, layout="ticks", place_candidates=0, memory="malloc", prioritized=False, priority_scale_log2=16):
        """env: BatchedDMPEnv (already reset); capacity_ticks: ring length in vector steps (>= 2).
        layout "ticks": obs[cap, N, D]; "tiled": obs[ceil(N / 64), cap, 64, D] -- a tile of 64 envs streams through its own
        contiguous region of the ring (SNAC_OBS_TILED: the faster layout to collect into); row(slot, env) and
        obs_at(slot) read either.  memory: where the observation ring lives -- "vmm": a snac_traj_alloc block (one virtual range
        over chunks from two 32 GiB slices of physical memory: MI355X writes it 15-20 % faster; building it
        holds up to half of the free device memory for about a second and freeing it waits for the device, so it is opt-in),
        "malloc" (default): torch.empty, "auto": "vmm" from 1 GiB up.  place_candidates > 1: the ring is placed by env.alloc_trajectory (that many
        candidate blocks timed with the rollout itself, the fastest kept: where the driver puts a block's runs still matters).
        prioritized=True: a PriorityTree over the cap * N entries (flat = slot * N + env), seeded from the env's seed, with
        priority_scale_log2 as its scale_log2."""
        if not isinstance(prioritized, bool):
            raise ValueError("prioritized must be a bool")
        if isinstance(priority_scale_log2, bool) or not isinstance(priority_scale_log2, int) or not 0 <= priority_scale_log2 <= 31:
            raise ValueError("priority_scale_log2 must be an integer in [0, 31]")
        if capacity_ticks < 2:
            raise ValueError("capacity_ticks must be >= 2")
        if layout not in ("ticks", "tiled"):
            raise ValueError("layout must be 'ticks' or 'tiled'")
        self.env = env
        self.cap = int(capacity_ticks)
        self.tiled = layout == "tiled"
        N, D, dev = env.num_envs, env.obs_dim, env.device
        self.placement = None
        if memory not in ("auto", "vmm", "malloc"):
            raise ValueError("memory must be 'auto', 'vmm' or 'malloc'")
        shape = ((N + 63) // 64, self.cap, 64, D) if self.tiled else (self.cap, N, D)
        nbytes = shape[0] * shape[1] * shape[2] * (shape[3] if self.tiled else 1) * torch.empty((), dtype=env.obs_dtype).element_size()
        if memory == "auto":
            memory = "vmm" if nbytes >= (1 << 30) else "malloc"
        if place_candidates and place_candidates > 1:
            self.obs, self.placement = env.alloc_trajectory(self.cap, candidates=int(place_candidates), layout=layout, memory=memory)
        elif memory == "vmm":
            from . import trajmem

            self.obs = trajmem.traj_empty(shape, env.obs_dtype, dev)
        else:
            self.obs = torch.empty(shape, dtype=env.obs_dtype, device=dev)
        self.memory = memory
        self.reward = torch.zeros((self.cap, N), dtype=torch.float32, device=dev)
        self.done = torch.zeros((self.cap, N), dtype=torch.uint8, device=dev)
        self.action = torch.zeros((self.cap, N), dtype=torch.int8, device=dev)
        self.step_size = torch.zeros((self.cap, N), dtype=torch.int8, device=dev)
        self.plan_idx = torch.zeros((self.cap, N), dtype=torch.int16, device=dev)
        self.first = torch.zeros((self.cap, N), dtype=torch.uint8, device=dev)
        self.head = 0          # next slot to write
        self.ticks = 0         # ticks collected so far
        self.plan_cells = 30 if env.kind == 1 else 400
        # the predecessor of slot 0 is slot cap - 1: seed it with the envs' CURRENT observation, so that the very first
        # transitions have their `s` also when the ring is attached to envs in mid-episode (first[0, i] == 0)
        self._put(self.cap - 1, env.observe())
        self._env_t = env.t    # the env may only advance through the ring: s' / s are paired by slot
        self.tree = None
        if prioritized:
            from .priority import MAX_ENTRIES, PriorityTree

            if self.cap * N > MAX_ENTRIES:
                raise ValueError("capacity_ticks * num_envs entries exceed what a PriorityTree holds (2^31 - 64)")
            self.tree = PriorityTree(self.cap * N, dev, scale_log2=priority_scale_log2, seed=env.seed, sampler_id=env.env_id_base * self.cap)

    def _put(self, slot, rows):
        """rows [N, D] -> the ring's slot (either layout)"""
        if not self.tiled:
            self.obs[slot].copy_(rows)
            return
        N, D = rows.shape
        G = self.obs.shape[0]
        if N != G * 64:                                            # ragged last tile: pad (the padding rows are never read)
            rows = torch.cat([rows, rows.new_zeros((G * 64 - N, D))])
        self.obs[:, slot].copy_(rows.view(G, 64, D))

    def obs_at(self, slot):
        """The observations of one ring slot as [N, D] (a view for layout "ticks", a copy for "tiled")."""
        if not self.tiled:
            return self.obs[slot]
        G, _, E, D = self.obs.shape
        return self.obs[:, slot].reshape(G * E, D)[:self.env.num_envs]

    def row(self, slot, env_index):
        """obs rows of (slot, env) pairs -> [B, D] in the ring's dtype (either layout)."""
        slot = torch.as_tensor(slot, device=self.env.device).long()
        env_index = torch.as_tensor(env_index, device=self.env.device).long()
        if not self.tiled:
            return self.obs[slot, env_index]
        return self.obs[env_index >> 6, slot, env_index & 63]

    def __len__(self):
        """Number of addressable transitions."""
        return self.valid_ticks() * self.env.num_envs

    def valid_ticks(self):
        """Slots whose predecessor is still in the ring (the oldest slot is kept only as a predecessor once wrapped)."""
        return self.ticks if self.ticks < self.cap else self.cap - 1

    def collect(self, T, actions=None, step_size=None):
        """Run T vector steps (auto-reset) and append them: at most two launches (ring wrap).  actions / step_size as in
        BatchedDMPEnv.rollout ([T, N] or None for the counter RNG)."""
        T = int(T)
        if T > self.cap:
            raise ValueError("T exceeds the ring capacity")
        if self.env.t != self._env_t:
            raise _lib.SnacError("the envs were stepped outside the ring since the last collect(): the predecessor rows no longer "
                                 "match (attach a new ReplayRing)")
        done_ticks = 0
        while done_ticks < T:
            n = min(T - done_ticks, self.cap - self.head)
            sl = slice(self.head, self.head + n)
            a = None if actions is None else actions[done_ticks:done_ticks + n]
            k = None if step_size is None else step_size[done_ticks:done_ticks + n]
            rec = dict(actions=self.action[sl], step_size=self.step_size[sl], plan_idx=self.plan_idx[sl], first=self.first[sl])
            if self.tiled:
                self.env.rollout(n, actions=a, step_size=k, obs="tiled", out=self.obs, ring=(self.cap, self.head),
                                 reward_out=self.reward[sl], done_out=self.done[sl], record=rec)
            else:
                self.env.rollout(n, actions=a, step_size=k, obs="all", out=self.obs[sl], reward_out=self.reward[sl],
                                 done_out=self.done[sl], record=rec)
            if self.tree is not None:                                # the span just written: the largest priority seen so far
                self.tree.fill(self.head * self.env.num_envs, n * self.env.num_envs)
            self.head = (self.head + n) % self.cap
            self.ticks += n
            done_ticks += n
        if self.tree is not None and T and self.ticks >= self.cap:   # wrapped: slot `head` survives only as a predecessor
            self.tree.fill(self.head * self.env.num_envs, self.env.num_envs, 0.0)
        self._env_t = self.env.t

    def collect_policy(self, net, T, mode="eps_greedy", epsilon=0.0, extra=None):
        """collect() with the actions from the DeviceMLP `net` (BatchedDMPEnv.rollout_policy: observe -> network -> draw -> step per tick,
        inside the launch): T vector steps appended in at most two launches (ring wrap), priorities filled as collect() does.  mode,
        epsilon: rollout_policy's.  extra: {"value" | "logp" | "entropy": a float32 [cap, N] tensor} whose rows of the written slots
        receive that output (RolloutBuffer.collect_policy).  layout "tiled" is not a layout of the fused launch: ValueError."""
        if self.tiled:
            raise ValueError("collect_policy needs layout='ticks': the fused launch writes [T, N, D] rows")
        if isinstance(T, bool) or not isinstance(T, int) or T < 1:
            raise ValueError("T must be an integer >= 1")
        if T > self.cap:
            raise ValueError("T exceeds the ring capacity")
        if self.env.t != self._env_t:
            raise _lib.SnacError("the envs were stepped outside the ring since the last collect(): the predecessor rows no longer "
                                 "match (attach a new ReplayRing)")
        done_ticks = 0
        while done_ticks < T:
            n = min(T - done_ticks, self.cap - self.head)
            sl = slice(self.head, self.head + n)
            out = dict(obs=self.obs[sl], reward=self.reward[sl], done=self.done[sl], actions=self.action[sl], step_size=self.step_size[sl],
                       plan_idx=self.plan_idx[sl], first=self.first[sl])
            out.update({name: t[sl] for name, t in (extra or {}).items()})
            self.env.rollout_policy(net, n, mode=mode, epsilon=epsilon, obs="all", want_value=False, want_logp=False, out=out)
            if self.tree is not None:                                # the span just written: the largest priority seen so far
                self.tree.fill(self.head * self.env.num_envs, n * self.env.num_envs)
            self.head = (self.head + n) % self.cap
            self.ticks += n
            done_ticks += n
        if self.tree is not None and self.ticks >= self.cap:         # wrapped: slot `head` survives only as a predecessor
            self.tree.fill(self.head * self.env.num_envs, self.env.num_envs, 0.0)
        self._env_t = self.env.t

    def append(self, actions, step_size=None):
        """One vector step with the caller's actions ([N], e.g. an epsilon-greedy policy's), appended to the ring."""
        actions = torch.as_tensor(actions, device=self.env.device)
        self.collect(1, actions=actions.reshape(1, -1), step_size=None if step_size is None else torch.as_tensor(step_size).reshape(1, -1))

    def slots(self):
        """Ring slots that hold addressable transitions, oldest first (int64 tensor on the device)."""
        v = self.valid_ticks()
        start = (self.head - v) % self.cap
        return (torch.arange(v, device=self.env.device) + start) % self.cap

    def gather(self, slot, env_index, with_plan=True):
        """Minibatch for explicit (slot, env) pairs -> dict of float32 / int tensors on the device:
        s [B, D], s_next [B, D], action [B], reward [B], done [B] (bool), plan [B, 20, 20] (1D: [B, 30])."""
        e = self.env
        slot, env_index, B = _pairs(e, slot, env_index)
        new = _outputs(torch.empty, e)
        s, s_next, plan = new(B, e.obs_dim), new(B, e.obs_dim), new(B, self.plan_cells) if with_plan else None
        self._gather_call(e._lib.snac_replay_gather_tiled if self.tiled else e._lib.snac_replay_gather, (self.obs, self.first, self.plan_idx),
                          slot, env_index, (), (s, s_next, plan), layout_arg=False)
        # action / reward / done of the samples: ONE flat index and three 1-D gathers (two-index advanced indexing was five index
        # kernels that took as long as the gather kernel itself, tools/gather_time.py)
        flat = slot.long() * e.num_envs + env_index.long()
        return _with_plan(e, dict(s=s, s_next=s_next, action=self.action.view(-1)[flat].long(), reward=self.reward.view(-1)[flat],
                                  done=self.done.view(-1)[flat].bool()), plan)

    def _gather_call(self, fn, rings, slot, env_index, extra, outs, layout_arg=True):
        """The one place that builds a gather call: desc, state, cap, the layout flag (the plain gather has an entry point per layout
        instead), the ring arrays (an integer among them, the walks' end, passes as it is), the pairs and their count, `extra`, the
        outputs and the stream; on the env's device, checked."""
        e = self.env
        head = [C.byref(e._desc), C.byref(e._state), self.cap] + ([int(self.tiled)] if layout_arg else [])
        rings = [a if isinstance(a, int) else _ptr(a) for a in rings]
        with torch.cuda.device(e.device):
            _lib.check(fn(*head, *rings, _ptr(slot), _ptr(env_index), int(slot.numel()), *extra, *[_ptr(o) for o in outs], e._stream()))

    def gather_nstep(self, slot, env_index, n, gamma, with_plan=True):
        """n-step transitions from explicit (slot, env) pairs (Rainbow's multi-step memory): the walk starts at the pair's step and ends
        after n steps, at a done, at an episode's end without one, or at the newest slot, whichever comes first.  -> the gather() dict
        with `return` float32 [B] in the place of `reward` (the discounted sum of the rewards taken, in float64), and discount float32
        [B] (gamma ** steps, 0 where done), steps int32 [B]; s and action are step 0's, s_next and done the last step's.  The target is
        out["return"] + out["discount"] * max_a Q(out["s_next"]).  One launch; n = 1 is gather()."""
        n, gamma = _walk_steps("n", n), _walk_gamma(gamma)
        e = self.env
        slot, env_index, B = _pairs(e, slot, env_index)
        new = _outputs(torch.empty, e)
        s, s_next, plan = new(B, e.obs_dim), new(B, e.obs_dim), new(B, self.plan_cells) if with_plan else None
        action, ret, discount = new(B, dtype=torch.int64), new(B), new(B)
        done, steps = new(B, dtype=torch.bool), new(B, dtype=torch.int32)
        rings = (self.obs, self.first, self.done, self.reward, self.action, self.plan_idx, (self.head - 1) % self.cap)
        self._gather_call(e._lib.snac_replay_gather_nstep, rings, slot, env_index, (n, gamma), (s, s_next, plan, action, ret, discount, done, steps))
        out = dict(s=s, s_next=s_next, action=action, done=done, discount=discount, steps=steps)
        out["return"] = ret
        return _with_plan(e, out, plan)

    def gather_windows(self, slot, env_index, length, with_plan=True):
        """Windows of up to `length` consecutive transitions of one env inside ONE episode that END at the explicit (slot, env) pairs
        (DRQN's Memory.get_batch): a window reaches back until it has `length` steps, or meets the episode's first step or the oldest
        addressable slot.  -> s / s_next float32 [B, L, D], action int64 / reward float32 / done bool / mask bool [B, L], length int32
        [B], plan [B, 20, 20] (1D: [B, 30]; the plan at the window's last step).  The valid steps come first (position j holds step
        slot - length[b] + 1 + j) and everything past them is zero, so a recurrent net starts from its zero state at the window's real
        start.  One launch that reads the length + 1 distinct rows of a window once each; length = 1 is gather()."""
        L = _walk_steps("length", length)
        e = self.env
        slot, env_index, B = _pairs(e, slot, env_index)
        new = _outputs(torch.empty, e)
        s, s_next, plan = new(B, L, e.obs_dim), new(B, L, e.obs_dim), new(B, self.plan_cells) if with_plan else None
        action, reward = new(B, L, dtype=torch.int64), new(B, L)
        done, mask, length = new(B, L, dtype=torch.bool), new(B, L, dtype=torch.bool), new(B, dtype=torch.int32)
        rings = (self.obs, self.first, self.done, self.reward, self.action, self.plan_idx, (self.head - self.valid_ticks()) % self.cap)
        self._gather_call(e._lib.snac_replay_gather_windows, rings, slot, env_index, (L,), (s, s_next, plan, action, reward, done, mask, length))
        return _with_plan(e, dict(s=s, s_next=s_next, action=action, reward=reward, done=done, mask=mask, length=length), plan)

    def _draw(self, batch, generator, prioritized, beta, stratified):
        """The transitions of a minibatch -> slot, env, and for prioritized=True what sample() adds (index, prob, weight), else None."""
        if not isinstance(prioritized, bool):
            raise ValueError("prioritized must be a bool")
        if prioritized and self.tree is None:
            raise ValueError("prioritized=True needs the priority tree: ReplayRing(..., prioritized=True)")
        if prioritized and generator is not None:
            raise ValueError("generator does not go with prioritized=True: the tree draws with the counter RNG")
        if prioritized:
            beta = float(beta)
            if beta != beta or beta < 0 or beta == float("inf"):
                raise ValueError("beta must be a finite number >= 0")
        v = self.valid_ticks()
        if v == 0:
            raise ValueError("the ring is empty")
        dev = self.env.device
        if prioritized:
            N = self.env.num_envs
            flat, prob = self.tree.sample(int(batch), stratified)
            w = (prob * float(len(self))) ** -beta
            return flat // N, flat % N, dict(index=flat, prob=prob, weight=w / w.max())
        age = torch.randint(0, v, (batch,), device=dev, generator=generator)
        slot = (self.head - 1 - age) % self.cap
        env_index = torch.randint(0, self.env.num_envs, (batch,), device=dev, generator=generator)
        return slot, env_index, None

    def sample(self, batch, generator=None, with_plan=True, prioritized=False, beta=0.4, stratified=True, n_step=None, gamma=None):
        """Uniform minibatch over the addressable transitions (random.sample in the reference, :144).  prioritized=True (a
        ReplayRing(prioritized=True); generator None): the transitions are drawn from the priority tree, with replacement, stratified
        over the total unless stratified=False, and the gather() dict gains slot, env and index = slot * N + env (int64 [n]; what
        update_priorities() takes), prob float32 [n] and the importance weights weight = (len(self) * prob) ** -beta / their largest
        over the batch (beta = 0: all ones).  n_step=n (an integer in [1, 64], with gamma): the same draw, gathered as n-step
        transitions -- the gather_nstep() dict, with slot and env."""
        if n_step is not None:
            n_step, gamma = _walk_steps("n_step", n_step), _walk_gamma(gamma)
        slot, env_index, extra = self._draw(batch, generator, prioritized, beta, stratified)
        if n_step is None:
            out = self.gather(slot, env_index, with_plan=with_plan)
        else:
            out = self.gather_nstep(slot, env_index, n_step, gamma, with_plan=with_plan)
        if extra is not None or n_step is not None:
            out.update(slot=slot, env=env_index, **(extra or {}))
        return out

    def sample_windows(self, batch, length, generator=None, with_plan=True, prioritized=False, beta=0.4, stratified=True):
        """DRQN-style minibatch without a host synchronisation: the window ENDS are drawn as sample() draws transitions (uniform, or
        prioritized=True with index, prob and weight of the end), and gather_windows() gives each its window -> the gather_windows()
        dict with slot and env (those of the window's end).  Where sample_sequences() rejects a window that crosses an episode's start
        and draws again, this returns it shorter, with its mask."""
        length = _walk_steps("length", length)
        slot, env_index, extra = self._draw(batch, generator, prioritized, beta, stratified)
        out = self.gather_windows(slot, env_index, length, with_plan=with_plan)
        out.update(slot=slot, env=env_index, **(extra or {}))
        return out

    def update_priorities(self, index, priority):
        """New priorities for sampled transitions (PriorityTree.update): index [n], the `index` of sample(prioritized=True);
        priority [n], floats >= 0, e.g. |td| (the caller applies alpha).  Where an index repeats, the largest priority wins.  A
        transition that collect() overwrote between sample() and update_priorities() receives the stale priority: the usual behaviour
        of prioritised replay; the next update of that entry corrects it.  Indices in the slot kept only as a predecessor are skipped,
        so that it stays undrawable.  No host synchronisation."""
        if self.tree is None:
            raise ValueError("update_priorities() needs the priority tree: ReplayRing(..., prioritized=True)")
        if not torch.is_tensor(index) or index.is_floating_point() or index.is_complex() or index.dtype == torch.bool:
            raise ValueError("index must be an integer tensor")
        if self.ticks >= self.cap:
            index = index.masked_fill(index // self.env.num_envs == self.head, -1)
        self.tree.update(index, priority)

    def sample_sequences(self, batch, time_step, generator=None, with_plan=True, oversample=4):
        """DRQN-style minibatch (Memory.get_batch of script/DRQN/2d/DRQN_2D_dynamic_training.py:131-143): `batch` windows of
        `time_step` consecutive transitions of one env that lie inside ONE episode -> dict of tensors
        s / s_next [B, L, D] float32, action / reward / done [B, L], plan [B, 20, 20] (1D: [B, 30]).
        Windows are drawn uniformly over all valid windows in the ring (the reference draws an episode first, then a
        window inside it, so it favours short episodes; neither is a parity surface -- the reference uses python's
        `random`).  Candidates are drawn `oversample` x batch at a time and filtered on the device, which waits for the device every round;
        sample_windows() draws window ends and masks instead, in one launch and without that wait."""
        L, B = int(time_step), int(batch)
        v = self.valid_ticks()
        if L < 1 or v < L:
            raise ValueError("time_step must be in [1, valid_ticks()]")
        dev, N = self.env.device, self.env.num_envs
        steps = torch.arange(L, device=dev)
        got_slot, got_env, have = [], [], 0
        for _ in range(64):
            n = max(B * oversample, 64)
            age = torch.randint(L - 1, v, (n,), device=dev, generator=generator)        # age of the window's FIRST transition
            env_index = torch.randint(0, N, (n,), device=dev, generator=generator)
            slots = (self.head - 1 - age[:, None] + steps[None, :]) % self.cap            # [n, L], oldest first
            inside = self.first[slots[:, 1:], env_index[:, None]].sum(dim=1) == 0 if L > 1 else torch.ones(n, dtype=torch.bool, device=dev)
            got_slot.append(slots[inside]); got_env.append(env_index[inside])
            have += int(inside.sum())
            if have >= B:
                break
        if have < B:
            raise ValueError("no episode in the ring holds %d consecutive steps" % L)
        slots, env_index = torch.cat(got_slot)[:B], torch.cat(got_env)[:B]
        flat = self.gather(slots.reshape(-1), env_index[:, None].expand(B, L).reshape(-1), with_plan=False)
        out = {k: t.view(B, L, *t.shape[1:]) for k, t in flat.items()}
        if with_plan:
            out["plan"] = self.gather(slots[:, 0], env_index, with_plan=True)["plan"]
        out["slot"], out["env"] = slots, env_index
        return out
