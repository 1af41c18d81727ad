"""SearchLoss: the self-play update on the device (include/snac_hip.h, "Search loss (AlphaZero / Gumbel self-play)";
snac_amd/csrc/k_search.hip).

What stands between the network and the optimiser in an AlphaZero minibatch -- the log-softmax of the policy head, its cross-entropy to
the search's distribution, the squared or Huber error of the value head to the return, the importance weights of prioritised replay, the
mean, and the backward pass through all of it -- is one call of two launches that never waits for the device: snac_search_loss gives the
mean loss, its closed-form gradient with respect to the logits and the value, the new priorities |value - z| and the batch statistics.
Float64 operations and float64 sums in a stated order: the same inputs give the same bytes on every run.

    sl = SearchLoss(env)                                                         # or SearchLoss(5, device="cuda:0"); huber=D: Huber's value error
    mb = play.sample(batch, prioritized=True, beta=0.4)
    y = net(mb["obs"])
    loss, _, priority = sl.loss(y[:, :A].contiguous(), y[:, A].contiguous(), mb, want_per_sample=True)
    opt.zero_grad(set_to_none=True); loss.backward(); opt.step()
    play.update_priorities(mb["index"], priority)                               # device to device: nothing waits
    sl.stats_dict()                                                              # of the last call; the only call that waits
"""
import math

import torch

from ._lib import ptr as _ptr
from ._rule import Rule

STATS = ("loss", "policy_loss", "value_loss", "entropy", "abs_error", "agreement", "good", "weight")      # the places of stats[0..8)


class _Loss(torch.autograd.Function):
    """The mean loss with d/dlogits and d/dvalue from the same call; everything else is a constant."""

    @staticmethod
    def forward(ctx, logits, value, sl, consts, want_per_sample):
        B = int(logits.shape[0])
        dev = sl.device
        grad_logits = torch.empty((B, sl.num_actions), dtype=torch.float32, device=dev)
        grad_value = torch.empty((B,), dtype=torch.float32, device=dev)
        loss = torch.empty((B,), dtype=torch.float32, device=dev) if want_per_sample else None
        priority = torch.empty((B,), dtype=torch.float32, device=dev) if want_per_sample else None
        mean = torch.empty((), dtype=torch.float32, device=dev)
        sl.stats = torch.empty((len(STATS),), dtype=torch.float64, device=dev)
        sl._call(B, logits, value, consts, 1.0 / B, loss, priority, grad_logits, grad_value, sl.stats, mean)
        ctx.save_for_backward(grad_logits, grad_value)
        if not want_per_sample:
            return mean
        ctx.mark_non_differentiable(loss, priority)
        return mean, loss, priority

    @staticmethod
    def backward(ctx, grad_mean, *unused):
        grad_logits, grad_value = ctx.saved_tensors
        return grad_mean * grad_logits, grad_mean * grad_value, None, None, None


class SearchLoss(Rule):
    def __init__(self, num_actions, vf_coef=1.0, huber=None, device=None):
        """num_actions: 3, 5 or 8 (the envs' action counts), or a BatchedDMPEnv, whose num_actions, device and stream are then taken;
        vf_coef: the weight of the value error, >= 0; huber: None for the squared error, or the delta > 0 of huber_loss; device: a cuda
        device (not with an env)."""
        super().__init__(num_actions, device, "the logits and the minibatch live")
        if isinstance(vf_coef, bool) or not isinstance(vf_coef, (int, float)) or not math.isfinite(vf_coef) or vf_coef < 0:
            raise ValueError("vf_coef must be a finite number >= 0")
        self.vf_coef = float(vf_coef)
        if huber is None:
            self.delta = 0.0
        else:
            if isinstance(huber, bool) or not isinstance(huber, (int, float)) or not math.isfinite(huber) or not huber > 0:
                raise ValueError("huber must be None (the squared error) or a finite delta > 0")
            self.delta = float(huber)
        self.stats = None                                            # float64 [8] on the device: the last call's
        self._partials = None                                        # made on first use: the constructor does not touch the device

    bad_rows = property(Rule._bad_rows, doc="""int32 [1] on the device: the samples zeroed so far (a NaN or +inf logit, every logit
    -inf, a pi that is not finite, negative or on a masked action, a value, z or weight that is not finite, a negative weight).""")

    def _call(self, B, logits, value, consts, scale, loss, priority, grad_logits, grad_value, stats, mean):
        """One snac_search_loss call on the current stream.  Only addresses are passed: a tensor that requires a gradient is read as data."""
        pi, z, weight = consts
        rows = (B + 63) // 64
        if self._partials is None or self._partials.shape[0] < rows:
            self._partials = torch.empty((max(rows, 64), len(STATS)), dtype=torch.float64, device=self.device)
        self._launch(self._lib.snac_search_loss, B, self.num_actions, _ptr(logits), _ptr(value), _ptr(pi), _ptr(z), _ptr(weight), self.vf_coef,
                     self.delta, scale, _ptr(loss), _ptr(priority), _ptr(grad_logits), _ptr(grad_value), _ptr(stats), _ptr(mean),
                     _ptr(self._partials), _ptr(self.bad_rows))

    def loss(self, logits, value, mb, want_per_sample=False):
        """0-dim float32: the mean over the minibatch of weight * (-(pi * log_softmax(logits)).sum(1) + vf_coef * error(value - z)), as a
        tensor that carries a gradient to `logits` (float32 [B, A]) and `value` (float32 [B]), both contiguous.  The forward pass is the
        one call, which also writes the gradient of the mean in closed form (the header's grad_logits and grad_value with scale 1 / B);
        the backward pass is one product each with the incoming gradient.  mb: the dict SelfPlay.sample() gives (its pi float32 [B, A],
        z float32 [B] and, if present, weight float32 [B] are read), or the tuple (pi, z[, weight]); they are constants of the loss.
        want_per_sample: also return the unweighted losses and the new priorities |value - z|, float32 [B] each, of the same call (no
        gradient).  self.stats holds the call's statistics afterwards.  Returns mean_loss, or (mean_loss, loss, priority)."""
        if isinstance(mb, dict):
            try:
                pi, z = mb["pi"], mb["z"]
            except KeyError as e:
                raise ValueError("mb must hold pi and z: %s is missing" % e) from None
            weight = mb.get("weight")
        else:
            try:
                pi, z, weight = mb if len(mb) == 3 else tuple(mb) + (None,)
            except (TypeError, ValueError):
                raise ValueError("mb must be a minibatch dict or the tuple (pi, z[, weight])") from None
        logits = self._check(logits, (None, self.num_actions), "logits")
        B = int(logits.shape[0])
        value = self._check(value, (B,), "value")
        pi, z = self._check(pi, (B, self.num_actions), "pi"), self._check(z, (B,), "z")
        if weight is not None:
            weight = self._check(weight, (B,), "weight")
        return _Loss.apply(logits, value, self, (pi, z, weight), bool(want_per_sample))

    def stats_dict(self):
        """The statistics of the last loss() as Python floats: loss (weighted), policy_loss, value_loss, entropy, abs_error, agreement,
        weight (means over the minibatch) and good (a count).  Waits for the device: the only call here that does."""
        if self.stats is None:
            raise ValueError("no loss() has been called yet")
        return dict(zip(STATS, self.stats.tolist()))
