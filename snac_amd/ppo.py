"""PPOLoss: PPO's update on the device (include/snac_hip.h, "PPO loss (the reference's script/PPO)"; snac_amd/csrc/k_ppo.hip).

What stands between the network and the optimiser in a PPO minibatch -- the log-probability of the taken action, the ratio, the clipped
surrogate, the (clipped) value loss, the entropy bonus, their mean, and the backward pass through all of it -- is one call of two
launches that never waits for the device: snac_ppo_loss gives the mean loss, its closed-form gradient with respect to the logits and the
value, and PPO2's diagnostics (approximate KL, clip fraction).  Float64 operations and float64 sums in a stated order: the same inputs
give the same bytes on every run.

    ppo = PPOLoss(env)                                                           # or PPOLoss(5, device="cuda:0")
    for mb in buf.minibatches(batch, epochs):
        logits, value = net(mb["s"], mb["plan"])
        loss = ppo.loss(logits, value, mb)                                       # 0-dim float32, carries the gradient
        opt.zero_grad(set_to_none=True); loss.backward(); opt.step()
    ppo.stats_dict()                                                             # of the last call; the only call that waits

The value function is clipped as PPO2 does by default (clip_vf=None: by `clip`); a negative clip_vf turns that off.
"""
import math

import torch

from ._lib import ptr as _ptr
from ._rule import Rule

STATS = ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "good", "clamped")      # the places of stats[0..8)


class _Loss(torch.autograd.Function):
    """The mean loss with d/dlogits and d/dvalue from the same call; everything else is a constant."""

    @staticmethod
    def forward(ctx, logits, value, ppo, consts, want_per_sample):
        B = int(logits.shape[0])
        dev = ppo.device
        grad_logits = torch.empty((B, ppo.num_actions), dtype=torch.float32, device=dev)
        grad_value = torch.empty((B,), dtype=torch.float32, device=dev)
        per_sample = torch.empty((B,), dtype=torch.float32, device=dev) if want_per_sample else None
        mean = torch.empty((), dtype=torch.float32, device=dev)
        ppo.stats = torch.empty((len(STATS),), dtype=torch.float64, device=dev)
        ppo._call(B, logits, value, consts, 1.0 / B, per_sample, grad_logits, grad_value, ppo.stats, mean)
        ctx.save_for_backward(grad_logits, grad_value)
        if not want_per_sample:
            return mean
        ctx.mark_non_differentiable(per_sample)
        return mean, per_sample

    @staticmethod
    def backward(ctx, grad_mean, *unused):
        grad_logits, grad_value = ctx.saved_tensors
        return grad_mean * grad_logits, grad_mean * grad_value, None, None, None


class PPOLoss(Rule):
    def __init__(self, num_actions, clip=0.2, clip_vf=None, vf_coef=0.5, ent_coef=0.01, device=None):
        """num_actions: 3, 5 or 8 (the envs' action counts), or a BatchedDMPEnv, whose num_actions, device and stream are then taken;
        clip: the surrogate's clip range, > 0; clip_vf: the value function's (None: `clip`, PPO2's default; negative: no clipping);
        vf_coef, ent_coef: the weights of the value loss and of the entropy bonus; device: a cuda device (not with an env)."""
        super().__init__(num_actions, device, "the logits and the minibatch live")

        def number(x, what):
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
                raise ValueError("%s must be a finite number" % what)
            return float(x)
        self.clip = number(clip, "clip")
        if not self.clip > 0:
            raise ValueError("clip must be > 0")
        self.clip_vf = self.clip if clip_vf is None else number(clip_vf, "clip_vf")
        self.vf_coef, self.ent_coef = number(vf_coef, "vf_coef"), number(ent_coef, "ent_coef")
        self.stats = None                                            # float64 [8] on the device: the last call's
        self._partials = None                                        # made on first use: the constructor does not touch the device

    bad_rows = property(Rule._bad_rows, doc="""int32 [1] on the device: the samples zeroed so far (a NaN or +inf logit, every logit
    -inf, an action outside [0, A) or without weight, a logp, adv, ret or value that is not finite).""")

    def _call(self, B, logits, value, consts, scale, loss, grad_logits, grad_value, stats, mean):
        """One snac_ppo_loss call on the current stream.  Only addresses are passed: a tensor that requires a gradient is read as data."""
        action, logp, adv, ret, value_old = consts
        rows = (B + 63) // 64
        if self._partials is None or self._partials.shape[0] < rows:
            self._partials = torch.empty((max(rows, 64), len(STATS)), dtype=torch.float64, device=self.device)
        self._launch(self._lib.snac_ppo_loss, B, self.num_actions, _ptr(logits), _ptr(action), _ptr(logp), _ptr(adv), _ptr(value), _ptr(value_old),
                     _ptr(ret), self.clip, self.clip_vf, self.vf_coef, self.ent_coef, scale, _ptr(loss), _ptr(grad_logits), _ptr(grad_value), _ptr(stats),
                     _ptr(mean), _ptr(self._partials), _ptr(self.bad_rows))

    def loss(self, logits, value, mb, want_per_sample=False):
        """0-dim float32: the mean over the minibatch of PPO2's loss -min(r adv, clamp(r) adv) + vf_coef * Lv - ent_coef * H, as a tensor
        that carries a gradient to `logits` (float32 [B, A]) and `value` (float32 [B]).  The forward pass is the one call, which also
        writes the gradient of the mean in closed form (the header's grad_logits and grad_value with scale 1 / B); the backward pass is
        one product each with the incoming gradient.  mb: the dict RolloutBuffer.minibatches() / gather() gives (its action int64 [B],
        logp, adv, ret and value -- the old value -- float32 [B] are read), or the tuple (action, logp, adv, ret, value_old); they are
        constants of the loss.  want_per_sample: also return the losses float32 [B] of the same call (no gradient).  self.stats holds
        the call's statistics afterwards.  Returns mean_loss, or (mean_loss, loss)."""
        logits = self._check(logits, (None, self.num_actions), "logits")
        B = int(logits.shape[0])
        value = self._check(value, (B,), "value")
        if isinstance(mb, dict):
            try:
                action, logp, adv, ret, value_old = (mb[k] for k in ("action", "logp", "adv", "ret", "value"))
            except KeyError as e:
                raise ValueError("mb must hold action, logp, adv, ret and value: %s is missing" % e) from None
        else:
            try:
                action, logp, adv, ret, value_old = mb
            except (TypeError, ValueError):
                raise ValueError("mb must be a minibatch dict or the tuple (action, logp, adv, ret, value_old)") from None
        action = self._check(action, (B,), "action", torch.int64)
        logp, adv, ret = self._check(logp, (B,), "logp"), self._check(adv, (B,), "adv"), self._check(ret, (B,), "ret")
        value_old = self._check(value_old, (B,), "value_old") if self.clip_vf >= 0 else None
        return _Loss.apply(logits, value, self, (action, logp, adv, ret, value_old), bool(want_per_sample))

    def stats_dict(self):
        """The statistics of the last loss() as Python floats: loss, policy_loss, value_loss, entropy, approx_kl, clip_fraction (means
        over the minibatch), good and clamped (counts).  Waits for the device: the only call here that does."""
        if self.stats is None:
            raise ValueError("no loss() has been called yet")
        return dict(zip(STATS, self.stats.tolist()))
