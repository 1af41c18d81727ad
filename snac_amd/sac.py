"""SoftValue: the data side of discrete SAC on the device (include/snac_hip.h, "Soft values (discrete SAC)"; snac_amd/csrc/k_soft.hip).

All three losses of discrete SAC are functions of one softmax of the policy's logits and one elementwise minimum of two critics over
A = 3, 5 or 8 actions per sample.  snac_soft_value gives them in one launch that never waits for the device: the soft state value
V = sum_a pi_a (min(q1, q2)_a - alpha * log pi_a), the TD target ret + discount * V, the entropy (the bytes of env.sample_actions'), and
the closed-form gradient of the actor loss -V with respect to the logits, so that no backward pass runs through softmax / log-softmax.
Float64 operations in a stated order: the same inputs give the same bytes on every run.

    soft = SoftValue(env)                                                        # or SoftValue(5, device="cuda:0")
    alpha = log_alpha.detach().exp()                                             # one float32 on the device; a Python float will do
    y = soft.target(actor(s_next), q1_target(s_next), q2_target(s_next), alpha, ret, discount)
    critic_loss = mse(q1(s)[range(B), action], y) + mse(q2(s)[range(B), action], y)
    loss, entropy = soft.policy_loss(actor(s), q1(s).detach(), q2(s).detach(), alpha, want_entropy=True)
    loss.mean().backward()                                                       # d/dlogits from the forward launch
    alpha_loss = log_alpha * (entropy - target_entropy).mean()

A logit of -inf (or more than 45 below the row's largest) masks its action: its q-value is never read into a sum.
"""
import math

import torch

from ._lib import ptr as _ptr
from ._rule import Rule


class _PolicyLoss(torch.autograd.Function):
    """-V per sample with d(-V)/dlogits from the same launch; q1, q2 and alpha are constants."""

    @staticmethod
    def forward(ctx, logits, soft, q1, q2, alpha, want_entropy):
        B = int(logits.shape[0])
        v = torch.empty((B,), dtype=torch.float32, device=soft.device)
        grad = torch.empty((B, soft.num_actions), dtype=torch.float32, device=soft.device)
        entropy = torch.empty((B,), dtype=torch.float32, device=soft.device) if want_entropy else None
        soft._call(B, logits, q1, q2, alpha, None, None, 1.0, v, None, entropy, grad)
        ctx.save_for_backward(grad)
        if not want_entropy:
            return v.neg_()
        ctx.mark_non_differentiable(entropy)
        return v.neg_(), entropy

    @staticmethod
    def backward(ctx, grad_loss, *unused):
        grad, = ctx.saved_tensors
        return grad_loss[:, None] * grad, None, None, None, None, None


class SoftValue(Rule):
    def __init__(self, num_actions, device=None):
        """num_actions: 3, 5 or 8 (the envs' action counts), or a BatchedDMPEnv, whose num_actions, device and stream are then taken;
        device: a cuda device (not with an env)."""
        super().__init__(num_actions, device, "the logits and q-values live")
        self._alpha = None                                           # made on first use: the constructor does not touch the device

    bad_rows = property(Rule._bad_rows, doc="""int32 [1] on the device: the samples zeroed so far (a NaN or +inf logit, every logit
    -inf, ret or discount not finite or a negative discount in target(), alpha not finite or negative: then every sample of the call).""")

    def _alpha_of(self, alpha):
        """The temperature as the kernel reads it: a one-element float32 tensor on the device.  A number is copied into a kept tensor."""
        if torch.is_tensor(alpha):
            if alpha.dtype != torch.float32 or alpha.numel() != 1 or not alpha.is_contiguous():
                raise ValueError("alpha must be a one-element torch.float32 tensor on %s, or a number" % self.device)
            if alpha.device != self.device:
                raise ValueError("alpha must be on %s" % self.device)
            return alpha
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha) or alpha < 0:
            raise ValueError("alpha must be a one-element torch.float32 tensor on %s, or a finite number >= 0" % self.device)
        if self._alpha is None:
            self._alpha = torch.empty((1,), dtype=torch.float32, device=self.device)
        return self._alpha.fill_(float(alpha))                       # on the current stream: ordered before the launch, nothing waits

    def _inputs(self, logits, q1, q2, alpha):
        A = self.num_actions
        logits = self._check(logits, (None, A), "logits")
        B = int(logits.shape[0])
        q1 = self._check(q1, (B, A), "q1")
        if q2 is not None:
            q2 = self._check(q2, (B, A), "q2")
        return B, logits, q1, q2, self._alpha_of(alpha)

    def _call(self, B, logits, q1, q2, alpha, ret, discount, scale, v, y, entropy, grad):
        """One snac_soft_value launch on the current stream.  Only addresses are passed: a tensor that requires a gradient is read as data."""
        self._launch(self._lib.snac_soft_value, B, self.num_actions, _ptr(logits), _ptr(q1), _ptr(q2), _ptr(alpha), _ptr(ret), _ptr(discount), scale,
                     _ptr(v), _ptr(y), _ptr(entropy), _ptr(grad), _ptr(self.bad_rows))

    def value(self, logits, q1, q2=None, alpha=0.0, out=None):
        """float32 [B]: the soft state value V = sum_a pi_a (min(q1, q2)_a - alpha * log pi_a) of every sample (one launch).  logits, q1,
        q2: float32 [B, A]; q2 None: one critic.  alpha: a one-element float32 tensor on the device (log_alpha.detach().exp()) or a number.
        out: an optional preallocated float32 [B]."""
        B, logits, q1, q2, alpha = self._inputs(logits, q1, q2, alpha)
        v = torch.empty((B,), dtype=torch.float32, device=self.device) if out is None else self._check(out, (B,), "out")
        self._call(B, logits, q1, q2, alpha, None, None, 1.0, v, None, None, None)
        return v

    def target(self, logits_next, q1_next, q2_next, alpha, ret, discount, out=None):
        """float32 [B]: the TD target y = ret + discount * V(s_next) of both critics (one launch).  logits_next: the actor's logits of
        s_next; q1_next, q2_next: the target critics' values there (q2_next None: one critic); ret, discount: float32 [B] (mb["return"],
        mb["discount"] of an n-step sample, or reward and gamma * (1 - done)).  A sample whose ret or discount is not finite, or whose
        discount is negative, gets 0 and is counted in bad_rows.  out: an optional preallocated float32 [B]."""
        B, logits, q1, q2, alpha = self._inputs(logits_next, q1_next, q2_next, alpha)
        ret = self._check(ret, (B,), "ret")
        discount = self._check(discount, (B,), "discount")
        y = torch.empty((B,), dtype=torch.float32, device=self.device) if out is None else self._check(out, (B,), "out")
        self._call(B, logits, q1, q2, alpha, ret, discount, 1.0, None, y, None, None)
        return y

    def entropy(self, logits, out=None):
        """float32 [B]: the entropy of softmax(logits), the bytes env.sample_actions(logits, want_entropy=True) gives (one launch; no
        gradient).  out: an optional preallocated float32 [B]."""
        logits = self._check(logits, (None, self.num_actions), "logits")
        B = int(logits.shape[0])
        h = torch.empty((B,), dtype=torch.float32, device=self.device) if out is None else self._check(out, (B,), "out")
        self._call(B, logits, None, None, None, None, None, 1.0, None, None, h, None)
        return h

    def policy_loss(self, logits, q1, q2, alpha, want_entropy=False):
        """float32 [B]: the actor loss per sample, -V = sum_a pi_a (alpha * log pi_a - min(q1, q2)_a), as a tensor that carries a gradient
        to `logits`.  The forward pass is one launch that also writes d(-V)/dlogits in closed form (pi_a (V - d_a), the header's grad with
        scale 1); the backward pass is one product with the incoming gradient and runs through no softmax.  q1, q2 and alpha are constants
        of this loss, as SAC detaches them: they get no gradient, whatever they require.  want_entropy: also return the entropy [B] of the
        same launch (no gradient), for the temperature's loss.  Returns loss, or (loss, entropy)."""
        B, logits, q1, q2, alpha = self._inputs(logits, q1, q2, alpha)
        return _PolicyLoss.apply(logits, self, q1, q2, alpha, bool(want_entropy))
