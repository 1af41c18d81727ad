"""A vectorised DQN loop on the batched API -- everything stays on the GPU: N envs step per tick (snac_step), transitions land
in the device replay ring (snac_rollout_rec via ReplayRing.collect is the random-policy prefill; the epsilon-greedy ticks
are appended with ReplayRing.append), minibatches come from snac_replay_gather.  The network and the update rule follow the
reference's 2D dynamic DQN (script/DQN/2d/DQN_2d_dynamic.py: observation 51 + plan 400 -> 5 Q values, target network,
replace every `replace` steps); this file is an illustration of the API, not part of the parity surface.

    python examples/dqn_batched.py --envs 4096 --ticks 200 [--prioritized] [--n-step N] [--distributional [--atoms K --vmin V --vmax V]]
                                   [--device-loss [--huber D] [--double]]

--prioritized: prioritised replay as in the reference's script/Rainbow, with the sum tree on the device (ReplayRing(prioritized=True)):
minibatches are drawn in proportion to |td|, the loss is weighted by the importance weights, and the sampled transitions get their new
priorities after every step.

--n-step N: Rainbow's multi-step target (ReplayRing.sample(n_step=N, gamma=gamma), one gather launch): the minibatch carries the discounted
sum of up to N rewards, the row N steps on (or where the episode or the ring ended) and the discount that goes with it, and the target is
return + discount * max Q(s_next).  It works together with --prioritized.

--distributional: Rainbow's categorical (C51) value head with CategoricalSupport.  The network ends in A * K logits, a softmax per action;
the agent acts on the expected values (expected(), one launch), and the target is the projection of return + discount * z under the target
network's distribution of the action the online network prefers in s_next (project(), one launch, the same bytes on every run; double DQN
as in the reference's Rainbow).  The loss is the cross-entropy between that target and the online distribution of the action taken; with
--prioritized it is weighted by the importance weights and its per-sample values are the new priorities.  The support: a 2D step pays 0
or 5 and never less, so a return lies in [0, 5 / (1 - gamma)] = [0, 100] at gamma = 0.95; these are the defaults of --vmin / --vmax.  The
projection clamps what falls outside, so a narrower choice is safe too, only coarser at its ends.

--device-loss: the DQN loss comes from TDLoss, one call of two launches in place of max, the target arithmetic, gather, the error, the
weighting, the mean and their backward passes: the target network's Q-values of s_next, the return and the discount go in as they are, the
mean comes back carrying its closed-form gradient, and with --prioritized the new priorities |td| of the same call go to the ring without
a host synchronisation.  --huber D: huber_loss(delta=D) instead of the squared error; --double: double DQN, the next action chosen by the
online network.  With --distributional the cross-entropy comes from CategoricalSupport.loss on the raw logits (no log_softmax, no
advanced index, no product and sum, and no backward pass through them), and its per-sample values are the new priorities.

--device-rollout K: K epsilon-greedy ticks per update, collected by one fused launch (ReplayRing.collect_policy: a DeviceMLP over the
Q-network's parameters acts inside the env launch) instead of one observe, forward, draw and append per tick.

--device-backward: the online network's pass of the update and the gradients of its weights come from the device (DeviceMLP.train_forward:
one forward launch, three for the backward pass, float64 chains in a stated order) instead of torch's modules and autograd's pass back
through them; the optimiser stays torch's.  Not with --distributional.

--device-optimizer (needs --device-backward): the Adam step is the device's too.  The online pass is DeviceMLP.forward with no autograd node
behind it, loss.backward() leaves the loss's gradient to the Q-values, DeviceAdam.backward_step turns it into the weight gradients and the
step (five launches, the same weights on every run), and the target network is copied by one launch (sync_target) in place of
load_state_dict's copy per parameter.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from snac_amd import BatchedDMPEnv, CategoricalSupport, DeviceAdam, DeviceMLP, ReplayRing, TDLoss  # noqa: E402


class QNet(nn.Module):
    def __init__(self, obs_dim, plan_cells, actions, hidden=256):
        super().__init__()
        self.body = nn.Sequential(nn.Linear(obs_dim + plan_cells, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(),
                                  nn.Linear(hidden, actions))

    def forward(self, obs, plan):
        return self.body(torch.cat([obs, plan.flatten(1)], dim=1))


def run(envs=4096, ticks=200, batch=2048, gamma=0.95, lr=1e-4, replace=50, prefill=64, seed=1, log=print, prioritized=False, beta=0.4, n_step=None,
        device_sampling=False, distributional=False, atoms=51, vmin=None, vmax=None, info=None, projection=None, device_loss=False, huber=None,
        double=False, device_rollout=None, device_backward=False, device_optimizer=False):
    """distributional: the C51 head and target (the module's docstring); vmin / vmax None: 0 and 5 / (1 - gamma).  info: an optional dict
    that receives the run's device counters ("bad_rows": the samples project() and the device loss zeroed; with prioritized also
    "priorities", a copy of the priority tree's leaves at the end).  device_loss: the DQN loss from TDLoss (the module's docstring), with
    huber: its delta, None for the squared error, and double: double DQN.  projection: a callable
    (p_next, ret, discount, p_select=) -> m in place of CategoricalSupport.project, for comparisons (tools/c51_time.py).
    device_sampling: the epsilon-greedy actions come from one launch per tick (BatchedDMPEnv.epsilon_greedy: counter-RNG stream 5,
    independent of the sharding and of torch's generator) instead of torch.rand / torch.randint / argmax.  device_rollout: K, the ticks
    collected per update by one fused launch (the module's docstring); not with distributional, whose actions need the expected values.
    device_backward: the online network's pass of the update and its weight gradients come from the device (DeviceMLP.train_forward: the
    module's docstring); not with distributional, whose head is wider than a DeviceMLP's 64 outputs.  device_optimizer: with
    device_backward, the Adam step and the target's copy are the device's as well (DeviceAdam: the module's docstring); info then receives
    "bad_steps", the steps refused for a gradient that was not finite."""
    if device_optimizer and not device_backward:
        raise ValueError("device_optimizer needs device_backward: the flat gradient of DeviceMLP.backward")
    if device_backward and distributional:
        raise ValueError("device_backward is not for distributional: its head of actions * atoms outputs is wider than a DeviceMLP runs")
    if device_rollout is not None and (distributional or isinstance(device_rollout, bool) or not isinstance(device_rollout, int) or device_rollout < 1):
        raise ValueError("device_rollout is a number of ticks >= 1, and not for distributional")
    if (huber is not None or double) and not device_loss:
        raise ValueError("huber and double belong to device_loss")
    if (huber is not None or double) and distributional:
        raise ValueError("huber and double belong to the DQN loss, not to distributional (whose target is double DQN's already)")
    torch.manual_seed(seed)
    env = BatchedDMPEnv(2, True, envs, seed=seed, obs_dtype=torch.float32)
    dev = env.device
    obs = env.reset()
    td_loss = TDLoss(env, huber=huber) if device_loss and not distributional else None
    ring = ReplayRing(env, capacity_ticks=max(2 * prefill, 128), **(dict(prioritized=True) if prioritized else {}))
    ring.collect(prefill)                                          # random policy, one fused launch
    obs = env.observe()
    plan = env.input_plan().float()
    heads = env.num_actions
    if distributional:
        support = CategoricalSupport(env, atoms=atoms, vmin=0.0 if vmin is None else vmin, vmax=5.0 / (1.0 - gamma) if vmax is None else vmax)
        heads = env.num_actions * atoms

        def dist(model, o, pl, log=False):                         # [B, A, K]: a distribution per action
            logits = model(o, pl).view(-1, env.num_actions, atoms)
            return logits.log_softmax(-1) if log else logits.softmax(-1).contiguous()

        def project(p_next, ret, disc, p_select):
            return support.project(p_next, ret, disc, p_select=p_select, want_action=False)[0]
    net, target = QNet(env.obs_dim, 400, heads).to(dev), QNet(env.obs_dim, 400, heads).to(dev)
    target.load_state_dict(net.state_dict())
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    mlp = DeviceMLP(net.body, None) if device_rollout or device_backward else None     # the Q-network's parameters, read in place by every launch
    if device_optimizer:                                           # tau = 1: a step leaves the target alone, sync_target() copies it
        opt = DeviceAdam(mlp, lr=lr, target=DeviceMLP(target.body, None))
    held = {}

    def online(s, pl):                                             # the Q-values the loss differentiates
        if device_optimizer:                                       # no autograd node for the network: y is the leaf the loss differentiates
            held["x"] = torch.cat([s, pl.flatten(1)], dim=1)
            held["y"] = mlp.forward(held["x"]).requires_grad_()
            return held["y"]
        if device_backward:                                        # forward and backward on the device: float64 chains in a stated order
            return mlp.train_forward(torch.cat([s, pl.flatten(1)], dim=1))
        return net(s, pl)
    t0, losses, returns = time.time(), [], []
    for tick in range(ticks):
        eps = max(0.05, 1.0 - tick / (0.6 * ticks))
        if device_rollout:
            ring.collect_policy(mlp, device_rollout, mode="eps_greedy", epsilon=eps)     # K ticks, recorded in the ring: one launch
        else:
            with torch.no_grad():
                q_now = support.expected(dist(net, obs.float(), plan)) if distributional else net(obs.float(), plan)
            if device_sampling:
                actions = env.epsilon_greedy(q_now, eps)
            else:
                greedy = q_now.argmax(dim=1)
                explore = torch.rand(envs, device=dev) < eps
                actions = torch.where(explore, torch.randint(0, env.num_actions, (envs,), device=dev), greedy).to(torch.int8)
            ring.append(actions)                                   # one env tick, recorded in the ring (auto-reset)
            obs = env.observe()
            plan = env.input_plan().float()                        # resets change plans
        how = dict(prioritized=True, beta=beta) if prioritized else {}
        if n_step is not None:
            how.update(n_step=n_step, gamma=gamma)
        mb = ring.sample(batch, **how)
        if distributional:
            with torch.no_grad():                                  # the plan does not change inside an episode: step 0's serves s_next
                ret = mb["reward"] if n_step is None else mb["return"]
                disc = gamma * (~mb["done"]).float() if n_step is None else mb["discount"]
                m = (projection or project)(dist(target, mb["s_next"], mb["plan"]), ret.float().contiguous(), disc.float().contiguous(),
                                            p_select=dist(net, mb["s_next"], mb["plan"]))
            if device_loss:                                        # the mean, its gradient and the per-sample values from one call
                out = support.loss(net(mb["s"], mb["plan"]).view(-1, env.num_actions, atoms), mb["action"], m,
                                   weight=mb["weight"] if prioritized else None, want_per_sample=prioritized)
                if prioritized:
                    loss = out[0]
                    ring.update_priorities(mb["index"], out[1])
                else:
                    loss = out
            else:
                logp = dist(net, mb["s"], mb["plan"], log=True)[torch.arange(batch, device=dev), mb["action"]]
                ce = -(m * logp).sum(1)                            # per sample: the cross-entropy of the target and the online distribution
                if prioritized:
                    loss = (mb["weight"] * ce).mean()
                    ring.update_priorities(mb["index"], ce.detach())
                else:
                    loss = ce.mean()
        elif device_loss:
            with torch.no_grad():                                  # the plan does not change inside an episode: step 0's serves s_next
                ret = (mb["reward"] if n_step is None else mb["return"]).float().contiguous()
                disc = (gamma * (~mb["done"]).float() if n_step is None else mb["discount"].float()).contiguous()
                q_next = target(mb["s_next"], mb["plan"])
                q_select = net(mb["s_next"], mb["plan"]) if double else None
            out = td_loss.loss(online(mb["s"], mb["plan"]), mb["action"], q_next=q_next, ret=ret, discount=disc, q_select=q_select,
                               weight=mb["weight"] if prioritized else None, want_per_sample=prioritized)
            if prioritized:
                loss = out[0]
                ring.update_priorities(mb["index"], out[2])       # |td| of the same call, device to device
            else:
                loss = out
        else:
            with torch.no_grad():
                q_next = target(mb["s_next"], mb["plan"]).max(dim=1).values
                if n_step is None:
                    y = mb["reward"] + gamma * q_next * (~mb["done"]).float()
                else:                                              # the plan does not change inside an episode: step 0's serves s_next
                    y = mb["return"] + mb["discount"] * q_next
            q = online(mb["s"], mb["plan"]).gather(1, mb["action"][:, None]).squeeze(1)
            if prioritized:
                td = q - y
                loss = (mb["weight"] * td ** 2).mean()
                ring.update_priorities(mb["index"], td.detach().abs())
            else:
                loss = nn.functional.mse_loss(q, y)
        if device_optimizer:
            loss.backward()                                        # leaves y.grad
            opt.backward_step(held["x"], held["y"].grad)           # weight gradients and Adam: five launches
        else:
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        losses.append(float(loss.detach()))
        if (tick + 1) % replace == 0:
            if device_optimizer:
                opt.sync_target()                                  # one launch
            else:
                target.load_state_dict(net.state_dict())
            st = env.episodic_stats()
            returns.append(st["return_sum"] / max(st["episodes"], 1))
            log("tick %4d  eps %.2f  loss %.4f  episodes %d  mean return %.2f  mean IoU %.4f  (%.0f env-steps/s incl. learning)" % (
                tick + 1, eps, losses[-1], st["episodes"], returns[-1], st["iou_fx_sum"] / 2.0**40 / max(st["episodes"], 1),
                envs * (tick + 1) / (time.time() - t0)))
    if info is not None and distributional:
        info["bad_rows"] = int(support.bad_rows.cpu()[0])
    if info is not None and device_loss:
        if not distributional:
            info["bad_rows"] = int(td_loss.bad_rows.cpu()[0])
        info["stats"] = (support if distributional else td_loss).stats_dict()
    if info is not None and device_optimizer:
        info["bad_steps"] = int(opt.bad_steps.cpu()[0])
    if info is not None and prioritized:
        info["priorities"] = ring.tree.weights().clone()
    return losses, returns


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--prioritized", action="store_true", help="prioritised replay: sample in proportion to |td|")
    ap.add_argument("--n-step", type=int, default=None, help="multi-step targets: the discounted sum of up to N rewards, bootstrapped N steps on")
    ap.add_argument("--device-sampling", action="store_true", help="epsilon-greedy on the device from the counter RNG (epsilon_greedy)")
    ap.add_argument("--distributional", action="store_true", help="the categorical (C51) head and the projected target (CategoricalSupport)")
    ap.add_argument("--atoms", type=int, default=51, help="--distributional: the atoms of the support")
    ap.add_argument("--vmin", type=float, default=None, help="--distributional: the support's lowest value (default 0)")
    ap.add_argument("--vmax", type=float, default=None, help="--distributional: the support's highest value (default 5 / (1 - gamma))")
    ap.add_argument("--device-loss", action="store_true", help="the DQN loss, its gradient and the new priorities from TDLoss (one call)")
    ap.add_argument("--huber", type=float, default=None, help="--device-loss: Huber's delta (default: the squared error)")
    ap.add_argument("--double", action="store_true", help="--device-loss: double DQN, the online network chooses the next action")
    ap.add_argument("--device-rollout", type=int, default=None, metavar="K", help="collect K epsilon-greedy ticks per update in one fused launch")
    ap.add_argument("--device-backward", action="store_true", help="the update's forward pass and weight gradients from the device (DeviceMLP.train_forward)")
    ap.add_argument("--device-optimizer", action="store_true", help="with --device-backward: the Adam step and the target's copy from the device (DeviceAdam)")
    a = ap.parse_args()
    if a.device_optimizer and not a.device_backward:
        ap.error("--device-optimizer needs --device-backward")
    if a.device_backward and a.distributional:
        ap.error("--device-backward is not for --distributional")
    run(a.envs, a.ticks, a.batch, prioritized=a.prioritized, n_step=a.n_step, device_sampling=a.device_sampling, distributional=a.distributional,
        atoms=a.atoms, vmin=a.vmin, vmax=a.vmax, device_loss=a.device_loss, huber=a.huber, double=a.double, device_rollout=a.device_rollout,
        device_backward=a.device_backward, device_optimizer=a.device_optimizer)
