"""TDLoss: the Q-learning update on the device (include/snac_hip.h, "Q-learning losses"; snac_amd/csrc/k_qloss.hip).

What stands between the network and the optimiser in a DQN minibatch -- the greedy or double-DQN choice of the next action, the target,
the taken action's Q-value, the squared or Huber error, the importance weights of prioritised replay, the mean, and the backward pass
through all of it -- is one call of two launches that never waits for the device: snac_td_loss gives the mean loss, its closed-form
gradient with respect to q, the new priorities |td| and the batch statistics.  Float64 operations and float64 sums in a stated order:
the same inputs give the same bytes on every run.

    td = TDLoss(env, huber=1.0)                                                  # or TDLoss(5, device="cuda:0"); huber=None: squared error
    mb = ring.sample_prioritized(batch, n_step=3, gamma=0.99)
    with torch.no_grad():
        q_next, q_select = target(mb["s_next"]), online(mb["s_next"])           # q_select: double DQN; leave it out for plain DQN
    loss, _, priority = td.loss(online(mb["s"]), mb["action"], q_next=q_next, ret=mb["return"], discount=mb["discount"],
                                q_select=q_select, weight=mb["weight"], want_per_sample=True)
    opt.zero_grad(set_to_none=True); loss.backward(); opt.step()
    ring.update_priorities(mb["index"], priority)                               # device to device: nothing waits
    td.stats_dict()                                                              # of the last call; the only call that waits

A target computed elsewhere goes in as y: SAC's critics take SoftValue.target's y, td.loss(q1(s), action, y).
"""
import math

import torch

from ._lib import ptr as _ptr
from ._rule import Rule

STATS = ("loss", "td_loss", "abs_td", "q_taken", "target", "linear_fraction", "good", "weight")      # the places of stats[0..8)


class _Loss(torch.autograd.Function):
    """The mean loss with d/dq from the same call; everything else is a constant."""

    @staticmethod
    def forward(ctx, q, td, consts, want_per_sample, want_y):
        B = int(q.shape[0])
        dev = td.device
        grad_q = torch.empty((B, td.num_actions), dtype=torch.float32, device=dev)
        loss = torch.empty((B,), dtype=torch.float32, device=dev) if want_per_sample else None
        priority = torch.empty((B,), dtype=torch.float32, device=dev) if want_per_sample else None
        y_out = torch.empty((B,), dtype=torch.float32, device=dev) if want_y else None
        mean = torch.empty((), dtype=torch.float32, device=dev)
        td.stats = torch.empty((len(STATS),), dtype=torch.float64, device=dev)
        td._call(B, q, consts, 1.0 / B, loss, priority, y_out, grad_q, td.stats, mean)
        ctx.save_for_backward(grad_q)
        extra = ((loss, priority) if want_per_sample else ()) + ((y_out,) if want_y else ())
        if not extra:
            return mean
        ctx.mark_non_differentiable(*extra)
        return (mean,) + extra

    @staticmethod
    def backward(ctx, grad_mean, *unused):
        grad_q, = ctx.saved_tensors
        return grad_mean * grad_q, None, None, None, None


class TDLoss(Rule):
    def __init__(self, num_actions, huber=None, device=None):
        """num_actions: 3, 5 or 8 (the envs' action counts), or a BatchedDMPEnv, whose num_actions, device and stream are then taken;
        huber: None for the squared error of mse_loss, or the delta > 0 of huber_loss; device: a cuda device (not with an env)."""
        super().__init__(num_actions, device, "the Q-values and the minibatch live")
        if huber is None:
            self.delta = 0.0
        else:
            if isinstance(huber, bool) or not isinstance(huber, (int, float)) or not math.isfinite(huber) or not huber > 0:
                raise ValueError("huber must be None (the squared error) or a finite delta > 0")
            self.delta = float(huber)
        self.stats = None                                            # float64 [8] on the device: the last call's
        self._partials = None                                        # made on first use: the constructor does not touch the device

    bad_rows = property(Rule._bad_rows, doc="""int32 [1] on the device: the samples zeroed so far (an action outside [0, A), a taken or
    chosen Q-value, ret, discount, y or weight that is not finite, a negative discount or weight).""")

    def _call(self, B, q, consts, scale, loss, priority, y_out, grad_q, stats, mean):
        """One snac_td_loss call on the current stream.  Only addresses are passed: a tensor that requires a gradient is read as data."""
        action, y, q_next, q_select, ret, discount, weight = consts
        rows = (B + 63) // 64
        if self._partials is None or self._partials.shape[0] < rows:
            self._partials = torch.empty((max(rows, 64), len(STATS)), dtype=torch.float64, device=self.device)
        self._launch(self._lib.snac_td_loss, B, self.num_actions, _ptr(q), _ptr(action), _ptr(y), _ptr(q_next), _ptr(q_select), _ptr(ret),
                     _ptr(discount), _ptr(weight), self.delta, scale, _ptr(loss), _ptr(priority), _ptr(y_out), _ptr(grad_q), _ptr(stats), _ptr(mean),
                     _ptr(self._partials), _ptr(self.bad_rows))

    def loss(self, q, action, y=None, *, q_next=None, ret=None, discount=None, q_select=None, weight=None, want_per_sample=False, want_y=False):
        """0-dim float32: the mean over the minibatch of weight * error(q[b, action[b]] - target[b]), as a tensor that carries a gradient
        to `q` (float32 [B, A]).  The forward pass is the one call, which also writes the gradient of the mean in closed form (the
        header's grad_q with scale 1 / B); the backward pass is one product with the incoming gradient.  action: int64 [B].  The target
        is exactly one of y, float32 [B], and ret + discount * q_next[b, a_star] with q_next float32 [B, A], ret and discount float32
        [B], where a_star is the largest of q_select[b] (float32 [B, A], double DQN) or, without it, of q_next[b].  weight: the
        importance weights float32 [B], or None.  All of them are constants of the loss.  want_per_sample: also return the unweighted
        errors and the new priorities |td|, float32 [B] each, of the same call (no gradient); want_y: also the targets float32 [B].
        self.stats holds the call's statistics afterwards.  Returns mean_loss, or (mean_loss[, loss, priority][, y])."""
        has_next = [t is not None for t in (q_next, ret, discount)]
        if y is not None and (any(has_next) or q_select is not None):
            raise ValueError("one target: y, or q_next, ret and discount, not both")
        if y is None and not all(has_next):
            raise ValueError("a target is needed: y, or q_next, ret and discount together")
        q = self._check(q, (None, self.num_actions), "q")
        B = int(q.shape[0])
        action = self._check(action, (B,), "action", torch.int64)
        if y is not None:
            y = self._check(y, (B,), "y")
        else:
            q_next = self._check(q_next, (B, self.num_actions), "q_next")
            ret, discount = self._check(ret, (B,), "ret"), self._check(discount, (B,), "discount")
            if q_select is not None:
                q_select = self._check(q_select, (B, self.num_actions), "q_select")
        if weight is not None:
            weight = self._check(weight, (B,), "weight")
        return _Loss.apply(q, self, (action, y, q_next, q_select, ret, discount, weight), bool(want_per_sample), bool(want_y))

    def stats_dict(self):
        """The statistics of the last loss() as Python floats: loss (weighted), td_loss, abs_td, q_taken, target, linear_fraction, weight
        (means over the minibatch) and good (a count).  Waits for the device: the only call here that does."""
        if self.stats is None:
            raise ValueError("no loss() has been called yet")
        return dict(zip(STATS, self.stats.tolist()))
