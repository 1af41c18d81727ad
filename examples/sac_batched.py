"""A vectorised discrete SAC loop on the batched API -- everything stays on the GPU: N envs step per tick, the actions are drawn from
the actor's logits on the device (BatchedDMPEnv.sample_actions), transitions land in the device replay ring, and the three losses of
discrete SAC come from SoftValue: the TD target of both critics in one launch (target()), and the actor loss with its closed-form
gradient and the entropy that drives the temperature in one more (policy_loss()).  The setting is examples/dqn_batched.py's, 2D dynamic
(observation 51 + plan 400 -> 5 actions), with the pieces of script/SAC's algorithm: an actor MLP, twin Q networks with slowly moving
target copies, a learned log_alpha.  This file is an illustration of the API, not part of the parity surface.

    python examples/sac_batched.py --envs 4096 --ticks 200 [--prioritized] [--n-step N] [--composition] [--device-loss]

--prioritized / --n-step N: as in examples/dqn_batched.py (prioritised replay by |td| of the first critic; multi-step returns).

--composition: the target, the actor loss and the entropy are computed by their torch forms instead (log_softmax, exp, minimum, products,
sums, and autograd through them), for timing (tools/sac_time.py) and as a cross-check of the gradient.  Acting and the replay stay as
they are.

--device-loss: both critic losses come from TDLoss on the target y (one call each in place of the gather, the difference, the square, the
weighting, the mean and their backward passes); with --prioritized the first critic's |td| of the same call are the new priorities.
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from snac_amd import BatchedDMPEnv, ReplayRing, SoftValue, TDLoss  # noqa: E402


class Net(nn.Module):
    """The actor (logits) and the critics (one Q value per action): the same body."""

    def __init__(self, obs_dim, plan_cells, actions, hidden=256):
        super().__init__()
        self.body = nn.Sequential(nn.Linear(obs_dim + plan_cells, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(),
                                  nn.Linear(hidden, actions))

    def forward(self, obs, plan):
        return self.body(torch.cat([obs, plan.flatten(1)], dim=1))


def torch_soft_value(logits, q1, q2, alpha):
    """(V [B], entropy [B]) by the composition: what SoftValue computes in one launch, in float32 torch."""
    logp = torch.log_softmax(logits, dim=1)
    pi = logp.exp()
    return (pi * (torch.minimum(q1, q2) - alpha * logp)).sum(dim=1), -(pi * logp).sum(dim=1)


def torch_target(logits_next, q1_next, q2_next, alpha, ret, discount):
    return ret + discount * torch_soft_value(logits_next, q1_next, q2_next, alpha)[0]


def torch_policy_loss(logits, q1, q2, alpha):
    """(loss [B] with a gradient to logits through autograd, entropy [B] detached)."""
    v, entropy = torch_soft_value(logits, q1, q2, alpha)
    return -v, entropy.detach()


def run(envs=4096, ticks=200, batch=2048, gamma=0.95, lr=3e-4, tau=0.005, prefill=64, seed=1, log=print, prioritized=False, beta=0.4,
        n_step=None, composition=False, report=50, info=None, device_loss=False):
    """-> (losses: per tick (critic, actor, temperature), returns: the mean episodic return at every report).  info: an optional dict
    that receives the run's device counters ("bad_rows": the samples SoftValue zeroed; with device_loss "td_bad_rows": those TDLoss
    zeroed) and the last temperature ("alpha").  device_loss: the critic losses from TDLoss (the module's docstring)."""
    torch.manual_seed(seed)
    env = BatchedDMPEnv(2, True, envs, seed=seed, obs_dtype=torch.float32)
    dev, A = env.device, env.num_actions
    env.reset()
    ring = ReplayRing(env, capacity_ticks=max(2 * prefill, 128), **(dict(prioritized=True) if prioritized else {}))
    ring.collect(prefill)                                          # random policy, one fused launch
    obs = env.observe()
    plan = env.input_plan().float()
    soft = SoftValue(env)
    td_loss = TDLoss(env) if device_loss else None
    actor = Net(env.obs_dim, 400, A).to(dev)
    critics = [Net(env.obs_dim, 400, A).to(dev) for _ in range(2)]
    targets = [Net(env.obs_dim, 400, A).to(dev) for _ in range(2)]
    for c, t in zip(critics, targets):
        t.load_state_dict(c.state_dict())
    log_alpha = torch.zeros((1,), device=dev, requires_grad=True)
    target_entropy = 0.98 * math.log(A)                            # discrete SAC's usual choice: a little below the uniform policy's
    opt = torch.optim.Adam([dict(params=actor.parameters()), dict(params=[p for c in critics for p in c.parameters()]), dict(params=[log_alpha])], lr=lr)
    online = [p for c in critics for p in c.parameters()]
    slow = [p for t in targets for p in t.parameters()]
    every = torch.arange(batch, device=dev)
    t0, losses, returns = time.time(), [], []
    for tick in range(ticks):
        with torch.no_grad():
            actions = env.sample_actions(actor(obs.float(), plan), want_logp=False)[0]
        ring.append(actions)                                       # one env tick, recorded in the ring (auto-reset)
        obs = env.observe()
        plan = env.input_plan().float()                            # resets change plans
        how = dict(prioritized=True, beta=beta) if prioritized else {}
        if n_step is not None:
            how.update(n_step=n_step, gamma=gamma)
        mb = ring.sample(batch, **how)
        alpha = log_alpha.detach().exp()                           # one float32 on the device: nothing waits for it
        with torch.no_grad():                                      # the plan does not change inside an episode: step 0's serves s_next
            ret = (mb["reward"] if n_step is None else mb["return"]).float().contiguous()
            disc = (gamma * (~mb["done"]).float() if n_step is None else mb["discount"].float()).contiguous()
            nxt = [actor(mb["s_next"], mb["plan"])] + [t(mb["s_next"], mb["plan"]) for t in targets]
            y = (torch_target if composition else soft.target)(*nxt, alpha, ret, disc)
        q = [c(mb["s"], mb["plan"]) for c in critics]
        if device_loss:
            w = mb["weight"] if prioritized else None
            first = td_loss.loss(q[0], mb["action"], y, weight=w, want_per_sample=prioritized)
            critic_loss = (first[0] if prioritized else first) + td_loss.loss(q[1], mb["action"], y, weight=w)
            if prioritized:
                ring.update_priorities(mb["index"], first[2])     # |td| of the first critic, device to device
        elif prioritized:
            td = [qa[every, mb["action"]] - y for qa in q]
            critic_loss = sum((mb["weight"] * d ** 2).mean() for d in td)
            ring.update_priorities(mb["index"], td[0].detach().abs())
        else:
            td = [qa[every, mb["action"]] - y for qa in q]
            critic_loss = sum((d ** 2).mean() for d in td)
        logits = actor(mb["s"], mb["plan"])
        if composition:
            pi_loss, entropy = torch_policy_loss(logits, q[0].detach(), q[1].detach(), alpha)
        else:                                                      # q and alpha are constants of this loss; the gradient comes with the forward launch
            pi_loss, entropy = soft.policy_loss(logits, q[0].detach(), q[1].detach(), alpha, want_entropy=True)
        actor_loss = pi_loss.mean()
        alpha_loss = (log_alpha * (entropy - target_entropy).mean()).sum()      # the entropy is the actor-loss launch's
        opt.zero_grad(set_to_none=True)
        (critic_loss + actor_loss + alpha_loss).backward()         # three losses over disjoint parameters
        opt.step()
        with torch.no_grad():
            torch._foreach_lerp_(slow, online, tau)                # the target critics follow slowly
        losses.append(torch.stack([critic_loss.detach(), actor_loss.detach(), alpha_loss.detach()]).tolist())
        if (tick + 1) % report == 0:
            st = env.episodic_stats()
            returns.append(st["return_sum"] / max(st["episodes"], 1))
            log("tick %4d  critic %.4f  actor %.4f  alpha %.4f  episodes %d  mean return %.2f  mean IoU %.4f  (%.0f env-steps/s incl. learning)" % (
                tick + 1, losses[-1][0], losses[-1][1], float(alpha), st["episodes"], returns[-1],
                st["iou_fx_sum"] / 2.0**40 / max(st["episodes"], 1), envs * (tick + 1) / (time.time() - t0)))
    if info is not None:
        info["bad_rows"] = int(soft.bad_rows.cpu()[0]) + int(env.policy_bad_rows.cpu()[0])
        info["alpha"] = float(log_alpha.detach().exp())
        if device_loss:
            info["td_bad_rows"] = int(td_loss.bad_rows.cpu()[0])
    return losses, returns


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--prioritized", action="store_true", help="prioritised replay: sample in proportion to |td| of the first critic")
    ap.add_argument("--n-step", type=int, default=None, help="multi-step targets: the discounted sum of up to N rewards, bootstrapped N steps on")
    ap.add_argument("--composition", action="store_true", help="the torch forms of the target, the actor loss and the entropy instead of SoftValue")
    ap.add_argument("--device-loss", action="store_true", help="both critic losses, their gradients and the new priorities from TDLoss")
    a = ap.parse_args()
    run(a.envs, a.ticks, a.batch, prioritized=a.prioritized, n_step=a.n_step, composition=a.composition, device_loss=a.device_loss)
