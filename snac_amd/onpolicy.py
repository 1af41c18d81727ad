"""RolloutBuffer: the on-policy side of the replay ring -- what the reference's script/PPO collects per update, kept on the GPU.

A composition over ReplayRing(env, horizon + 1): the ring's arrays hold the horizon's observations, actions, rewards and dones, and four
more [cap, N] float32 arrays hold what PPO adds -- `value` and `logp` of the action taken (written by act()), `adv` and `ret` (written by
finish()).  The extra slot is the predecessor row of the oldest step, so all `horizon` slots stay addressable after the ring wrapped.

    buf = RolloutBuffer(env, horizon, gamma, lam)
    for _ in range(horizon):
        obs = env.observe()                              # the observation to act on, as in examples/dqn_batched.py
        buf.act(actions, value, logp)                    # value / logp at the head slot, then ring.append(actions)
    buf.finish(value_of(env.observe()))                  # snac_gae over the newest `horizon` slots: one launch
    for mb in buf.minibatches(batch, epochs):            # snac_replay_gather_onpolicy: one launch per minibatch
        ...                                              # mb["s"], ["plan"], ["action"], ["value"], ["logp"], ["adv"], ["ret"]

include/snac_hip.h, "On-policy rollouts", has both rules.  Nothing here waits for the device."""
import math

import torch

from . import _lib
from ._lib import ptr as _ptr
from .replay import ReplayRing, _outputs, _pairs, _with_plan

GAE_CHUNK = _lib.GAE_CHUNK                                           # slots per chunk of snac_gae's kernel (SNAC_GAE_CHUNK)


def _count(name, v):
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError("%s must be an integer >= 1" % name)
    return v


def _finite(name, v):
    if v is None or isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError("%s must be a finite number" % name)
    return float(v)


class RolloutBuffer:
    def __init__(self, env, horizon, gamma, lam, layout="ticks"):
        """env: BatchedDMPEnv (already reset); horizon: vector steps per update (>= 1); gamma, lam: the discount and the lambda of
        generalised advantage estimation (finite numbers); layout: the ReplayRing's."""
        self.horizon, self.gamma, self.lam = _count("horizon", horizon), _finite("gamma", gamma), _finite("lam", lam)
        if layout not in ("ticks", "tiled"):
            raise ValueError("layout must be 'ticks' or 'tiled'")
        self.env = env
        self.ring = ReplayRing(env, self.horizon + 1, layout=layout)
        shape, dev = (self.ring.cap, env.num_envs), env.device
        self.value = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.logp = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.adv = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.ret = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.norm = torch.zeros((2,), dtype=torch.float32, device=dev)    # {mean, 1 / (std + 1e-8)} of adv over the span
        self._actions = torch.empty((env.num_envs,), dtype=torch.int8, device=dev)      # act_logits(): the actions of the tick, reused
        self.collected = 0                                           # ticks since the last finish()
        self.first = None                                            # the oldest slot of the span finish() filled

    def act(self, actions, value, logp):
        """One vector step: `value` [N] (the critic's value of env.observe()) and `logp` [N] (the log-probability of `actions` under the
        policy that drew them) go to the ring's head slot, then the envs step with `actions` [N] (ReplayRing.append, auto-reset)."""
        head = self.ring.head
        self.value[head].copy_(torch.as_tensor(value, device=self.env.device).reshape(-1))
        self.logp[head].copy_(torch.as_tensor(logp, device=self.env.device).reshape(-1))
        self.ring.append(actions)
        self.collected += 1

    def act_logits(self, logits, value):
        """act() with the draw on the device: one snac_policy_act launch (BatchedDMPEnv.sample_actions' rule, keyed by env.t) samples the
        actions from `logits` float32 [N, num_actions] into a reused int8 buffer and writes their log-probabilities straight into the head
        slot's row of `logp`; then `value` [N] goes to the head slot and the envs step, as in act().  Returns the actions (int8 [N], the
        buffer the next call overwrites)."""
        e, head = self.env, self.ring.head
        e.sample_actions(logits, out=(self._actions, self.logp[head], None))
        self.value[head].copy_(torch.as_tensor(value, device=e.device).reshape(-1))
        self.ring.append(self._actions)
        self.collected += 1
        return self._actions

    def collect_policy(self, net, T):
        """T act_logits() ticks with the DeviceMLP `net` as actor-critic, in at most two launches (ReplayRing.collect_policy, the
        categorical mode): the network takes the envs' observation rows (and their input_plan() cells, by its input width), its first
        num_actions outputs are the logits and its last one the value; `value` and `logp` go straight into the written slots' rows."""
        from .mlp import DeviceMLP

        if not isinstance(net, DeviceMLP) or net.dims[-1] != self.env.num_actions + 1:
            raise ValueError("collect_policy needs an actor-critic: a network with num_actions + 1 = %d outputs" % (self.env.num_actions + 1))
        self.ring.collect_policy(net, T, mode="categorical", extra=dict(value=self.value, logp=self.logp))
        self.collected += T

    def span(self):
        """(first, count): the newest `horizon` slots, oldest first, as snac_gae takes them."""
        return (self.ring.head - self.horizon) % self.ring.cap, self.horizon

    def finish(self, bootstrap_value=None):
        """Advantages and returns of the newest `horizon` slots (snac_gae, one launch).  bootstrap_value [N]: the critic's value of every
        env's current observation (None: zeros)."""
        if self.collected < self.horizon:
            raise ValueError("finish() needs %d ticks since the last finish(); %d were collected" % (self.horizon, self.collected))
        e = self.env
        boot = None
        if bootstrap_value is not None:
            boot = torch.as_tensor(bootstrap_value, device=e.device).detach().to(torch.float32).reshape(-1).contiguous()
            if boot.numel() != e.num_envs:
                raise ValueError("bootstrap_value must hold one value per env")
        first, count = self.span()
        with torch.cuda.device(e.device):
            _lib.check(e._lib.snac_gae(e.num_envs, self.ring.cap, first, count, self.gamma, self.lam, _ptr(self.ring.reward), _ptr(self.ring.done),
                                       _ptr(self.value), _ptr(boot), _ptr(self.adv), _ptr(self.ret), e._stream()))
        self.first, self.collected = first, 0

    def span_slots(self):
        """The slots finish() filled, oldest first (int64 tensor on the device)."""
        if self.first is None:
            raise ValueError("no span yet: call finish() first")
        return (torch.arange(self.horizon, device=self.env.device) + self.first) % self.ring.cap

    def update_norm(self):
        """mean and 1 / (std + 1e-8) of adv over the span -> self.norm, with torch on the device (the population std, as numpy's)."""
        a = self.adv.index_select(0, self.span_slots())
        torch.stack([a.mean(), 1.0 / (a.std(unbiased=False) + 1e-8)], out=self.norm)
        return self.norm

    def gather(self, slot, env_index, normalise=True, with_plan=True):
        """The PPO minibatch of explicit (slot, env) pairs (snac_replay_gather_onpolicy, one launch) -> dict of tensors on the device:
        s float32 [B, D] (the observation acted on), action int64 [B], value / logp / adv / ret float32 [B], plan [B, 20, 20] (1D:
        [B, 30]).  normalise=True: adv is (adv - norm[0]) * norm[1] with the pair update_norm() left in self.norm."""
        if not isinstance(normalise, bool):
            raise ValueError("normalise must be a bool")
        e, r = self.env, self.ring
        slot, env_index, B = _pairs(e, slot, env_index)
        new = _outputs(torch.empty, e)
        s, plan, action = new(B, e.obs_dim), new(B, r.plan_cells) if with_plan else None, new(B, dtype=torch.int64)
        value, logp, adv, ret = new(B), new(B), new(B), new(B)
        rings = (r.obs, r.first, r.plan_idx, r.action, self.value, self.logp, self.adv, self.ret, self.norm if normalise else None)
        r._gather_call(e._lib.snac_replay_gather_onpolicy, rings, slot, env_index, (), (s, plan, action, value, logp, adv, ret))
        return _with_plan(e, dict(s=s, action=action, value=value, logp=logp, adv=adv, ret=ret), plan)

    def minibatches(self, batch, epochs=1, normalise=True, generator=None):
        """`epochs` passes over the span finish() filled, each in a new random order: every (slot, env) of the span once per epoch, in
        minibatches of `batch` entries with a ragged last one -> the gather() dicts, with slot and env (int32 [B]).  The order is a
        device permutation (torch.randperm with `generator`) whose positions are mapped to (slot, env) on the device; the norm pair is
        computed once (normalise=True); one gather launch per minibatch."""
        batch, epochs = _count("batch", batch), _count("epochs", epochs)
        if not isinstance(normalise, bool):
            raise ValueError("normalise must be a bool")
        if self.first is None:
            raise ValueError("no span yet: call finish() first")
        return self._minibatches(batch, epochs, normalise, generator)

    def _minibatches(self, batch, epochs, normalise, generator):
        N, dev = self.env.num_envs, self.env.device
        total = self.horizon * N
        if normalise:
            self.update_norm()
        for _ in range(epochs):
            perm = torch.randperm(total, device=dev, generator=generator)
            slot = ((perm // N + self.first) % self.ring.cap).to(torch.int32)
            env_index = (perm % N).to(torch.int32)
            for b0 in range(0, total, batch):
                sl, en = slot[b0:b0 + batch], env_index[b0:b0 + batch]
                out = self.gather(sl, en, normalise=normalise)
                out.update(slot=sl, env=en)
                yield out
