"""CategoricalSupport: categorical (C51) value distributions on the device (include/snac_hip.h, "Distributional targets";
snac_amd/csrc/k_dist.hip).

A support of `atoms` values z_i = vmin + i * dz behind calls that never wait for the device: the expected values of a batch of
distributions (what an agent acts on), Rainbow's target -- the greedy or double-DQN choice of the next action and the projection of
return + discount * z onto the support -- and its loss, the cross-entropy of that target and the online distribution of the action taken
(include/snac_hip.h, "Q-learning losses"; k_qloss.hip).  All follow a rule of float64 operations in a stated order, so the same inputs
give the same bytes on every run; the textbook composition in torch ends in index_add_, whose float atomics land in any order.

    support = CategoricalSupport(env, atoms=51, vmin=-10.0, vmax=10.0)           # or CategoricalSupport(5, ..., device="cuda:0")
    q = support.expected(online(s).view(-1, A, 51).softmax(-1))                  # float32 [B, A]
    action = env.epsilon_greedy(q, eps)
    m, a_star, _ = support.project(target_p(s_next), ret, discount, p_select=online_p(s_next))      # m: float32 [B, 51]
    loss, ce = support.loss(online(s).view(-1, A, 51), action, m, weight=mb["weight"], want_per_sample=True)   # the raw logits, no softmax
    loss.backward()                                                              # one product: the gradient came with the forward call
    ring.update_priorities(mb["index"], ce)

The loss is the mean over the minibatch; its gradient with respect to the logits is written in closed form by the same call.
"""
import math

import torch

from ._lib import ptr as _ptr
from ._rule import Rule

MAX_ATOMS = 64
LOSS_STATS = ("loss", "cross_entropy", "entropy", "target_mass", "unused4", "unused5", "good", "weight")      # the places of stats[0..8) of loss()


class _Loss(torch.autograd.Function):
    """The mean cross-entropy with d/dlogits from the same call; everything else is a constant."""

    @staticmethod
    def forward(ctx, logits, support, action, m, weight, want_per_sample):
        B = int(logits.shape[0])
        dev = support.device
        grad = torch.empty_like(logits)
        per_sample = torch.empty((B,), dtype=torch.float32, device=dev) if want_per_sample else None
        mean = torch.empty((), dtype=torch.float32, device=dev)
        support.stats = torch.empty((len(LOSS_STATS),), dtype=torch.float64, device=dev)
        rows = (B + 63) // 64
        if support._partials is None or support._partials.shape[0] < rows:
            support._partials = torch.empty((max(rows, 64), len(LOSS_STATS)), dtype=torch.float64, device=dev)
        support._launch(support._lib.snac_c51_loss, B, support.num_actions, support.atoms, _ptr(logits), _ptr(action), _ptr(m), _ptr(weight), 1.0 / B,
                        _ptr(per_sample), _ptr(grad), _ptr(support.stats), _ptr(mean), _ptr(support._partials), _ptr(support.bad_rows))
        ctx.save_for_backward(grad)
        if not want_per_sample:
            return mean
        ctx.mark_non_differentiable(per_sample)
        return mean, per_sample

    @staticmethod
    def backward(ctx, grad_mean, *unused):
        grad, = ctx.saved_tensors
        return grad_mean * grad, None, None, None, None, None


class CategoricalSupport(Rule):
    def __init__(self, num_actions, atoms=51, vmin=-10.0, vmax=10.0, device=None):
        """num_actions: 3, 5 or 8 (the envs' action counts), or a BatchedDMPEnv, whose num_actions, device and stream are then taken;
        atoms: 2 .. 64; vmin < vmax, both finite; device: a cuda device (not with an env)."""
        super().__init__(num_actions, device, "the distributions live")
        if isinstance(atoms, bool) or not isinstance(atoms, int) or not 2 <= atoms <= MAX_ATOMS:
            raise ValueError("atoms must be an integer in [2, %d]" % MAX_ATOMS)
        for name, v in (("vmin", vmin), ("vmax", vmax)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError("%s must be a finite number" % name)
        if not vmin < vmax:
            raise ValueError("vmin must be below vmax")
        self.atoms, self.vmin, self.vmax = atoms, float(vmin), float(vmax)
        self.dz = (self.vmax - self.vmin) / float(atoms - 1)          # the header's dz: one float64 quotient
        self._z = None                                               # made on first use: the constructor does not touch the device
        self.stats = None                                            # float64 [8] on the device: the last loss()'s
        self._partials = None

    @property
    def z(self):
        """float32 [atoms] on the device: the support, rounded from the rule's float64 z_i (for the caller's own losses)."""
        if self._z is None:
            self._z = torch.tensor([self.vmin + float(i) * self.dz for i in range(self.atoms)], dtype=torch.float64).to(torch.float32).to(self.device)
        return self._z

    bad_rows = property(Rule._bad_rows, doc="""int32 [1] on the device: the samples project() (ret or discount not finite, or discount < 0)
    and loss() (an action outside [0, A), a logit of the taken action or an entry of m that is not finite, a weight that is not finite
    or negative) have zeroed so far.""")

    def _call(self, fn, B, *args):
        self._launch(fn, B, self.num_actions, self.atoms, self.vmin, self.vmax, *args)

    def expected(self, p, out=None):
        """float32 [B, A]: the expected value of every distribution of p, float32 [B, A, atoms] (snac_c51_expect, one launch).  It feeds
        env.epsilon_greedy(q, eps) when acting.  out: an optional preallocated float32 [B, A]."""
        A, K = self.num_actions, self.atoms
        p = self._check(p, (None, A, K), "p")
        B = int(p.shape[0])
        q = torch.empty((B, A), dtype=torch.float32, device=self.device) if out is None else self._check(out, (B, A), "out")
        self._call(self._lib.snac_c51_expect, B, _ptr(p), _ptr(q))
        return q

    def project(self, p_next, ret, discount, p_select=None, out=None, want_action=True, want_q=False):
        """The distributional target of a minibatch (snac_c51_project, one launch): per sample the action a_star with the largest expected
        value under p_select (None: p_next itself; double DQN gives the online network's distributions of s_next), lowest index on ties,
        and the distribution of ret + discount * z under p_next[b, a_star], clamped to [vmin, vmax] and shared between the two nearest
        atoms.  p_next, p_select: float32 [B, A, atoms]; ret, discount: float32 [B] (mb["return"], mb["discount"] of an n-step sample, or
        reward and gamma * (1 - done)).  A sample whose ret or discount is not finite, or whose discount is negative, gets a zero row,
        action 0 and value 0, and is counted in bad_rows.  out: optional preallocated (m float32 [B, atoms], a_star int8 [B] or None,
        q_star float32 [B] or None).  Returns (m, a_star or None, q_star or None); q_star is the expected value of p_next[b, a_star]."""
        A, K = self.num_actions, self.atoms
        p_next = self._check(p_next, (None, A, K), "p_next")
        B = int(p_next.shape[0])
        if p_select is not None:
            p_select = self._check(p_select, (B, A, K), "p_select")
        ret = self._check(ret, (B,), "ret")
        discount = self._check(discount, (B,), "discount")
        m, a_star, q_star = out if out is not None else (None, None, None)
        m = torch.empty((B, K), dtype=torch.float32, device=self.device) if m is None else self._check(m, (B, K), "out[0]")
        if not want_action:
            a_star = None
        elif a_star is None:
            a_star = torch.empty((B,), dtype=torch.int8, device=self.device)
        else:
            a_star = self._check(a_star, (B,), "out[1]", torch.int8)
        if not want_q:
            q_star = None
        elif q_star is None:
            q_star = torch.empty((B,), dtype=torch.float32, device=self.device)
        else:
            q_star = self._check(q_star, (B,), "out[2]")
        self._call(self._lib.snac_c51_project, B, _ptr(p_next), _ptr(p_select), _ptr(ret), _ptr(discount), _ptr(m), _ptr(a_star), _ptr(q_star),
                   _ptr(self.bad_rows))
        return m, a_star, q_star

    def loss(self, logits, action, m, weight=None, want_per_sample=False):
        """0-dim float32: the mean over the minibatch of weight * cross-entropy(m[b], softmax(logits[b, action[b]])), as a tensor that
        carries a gradient to `logits` (snac_c51_loss, two launches).  logits: float32 [B, A, atoms], contiguous: the .view(-1, A, atoms)
        of the network's output, no softmax; action: int64 [B]; m: float32 [B, atoms], what project() gives; weight: the importance
        weights float32 [B], or None.  The forward pass also writes the gradient of the mean in closed form (weight * (mass(m) * p - m) / B
        in the taken action's row, zeros elsewhere); the backward pass is one product.  want_per_sample: also return the unweighted
        cross-entropies float32 [B] of the same call (no gradient): the new priorities of prioritised replay.  self.stats holds the
        call's statistics afterwards.  Returns mean_loss, or (mean_loss, cross_entropy)."""
        A, K = self.num_actions, self.atoms
        logits = self._check(logits, (None, A, K), "logits")
        B = int(logits.shape[0])
        action = self._check(action, (B,), "action", torch.int64)
        m = self._check(m, (B, K), "m")
        if weight is not None:
            weight = self._check(weight, (B,), "weight")
        return _Loss.apply(logits, self, action, m, weight, bool(want_per_sample))

    def stats_dict(self):
        """The statistics of the last loss() as Python floats: loss (weighted), cross_entropy, entropy (of the online distribution of the
        action taken), target_mass, weight (means over the minibatch) and good (a count).  Waits for the device."""
        if self.stats is None:
            raise ValueError("no loss() has been called yet")
        return {k: v for k, v in zip(LOSS_STATS, self.stats.tolist()) if not k.startswith("unused")}
