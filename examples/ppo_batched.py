"""A vectorised PPO loop on the batched API -- everything stays on the GPU: N envs step per tick with the policy's actions, the steps land
in a RolloutBuffer (a ReplayRing of horizon + 1 slots with the critic's values and the actions' log-probabilities beside it), the
advantages and returns of a horizon come from one launch (snac_gae), and every minibatch of the update from one more
(snac_replay_gather_onpolicy).  The update rule is PPO2's, as in the reference's script/PPO: the clipped surrogate, a value loss and an
entropy bonus, with advantages normalised over the horizon and an episode's end treated as terminal.  The network is an actor-critic MLP
over observation + plan; this file is an illustration of the API, not part of the parity surface.

With --device-loss the loss of a minibatch, its gradient with respect to the logits and the value, and PPO2's diagnostics come from one
call (PPOLoss: snac_ppo_loss) instead of the torch composition and autograd's pass back through it; --clip-vf then clips the value
function as PPO2 does by default.

With --device-rollout the actor-critic is one Sequential of Linear and ReLU with num_actions + 1 outputs (the logits and the value), a
DeviceMLP over its parameters acts inside the env launch (RolloutBuffer.collect_policy: a horizon in one launch, two on a ring wrap) and
gives the bootstrap value (one forward launch); the update trains the same parameters through autograd as before.

With --device-backward (which needs --device-rollout's network) the update's forward pass and the gradients of the weights come from the
device too (DeviceMLP.train_forward: float64 chains in a stated order, three launches for the backward pass); the optimiser and the
gradient clip stay torch's.

With --device-optimizer (which needs --device-backward) they come from the device as well: the network's pass is DeviceMLP.forward with no
autograd node behind it, loss.backward() leaves the loss's gradient to the outputs, and DeviceAdam.backward_step turns it into the weight
gradients, their global norm, the clip at 0.5 and the Adam step, written into the parameters where they lie: five launches, the same
weights on every run.

    python examples/ppo_batched.py --envs 4096 --iterations 20 [--device-loss [--clip-vf 0.2]] [--device-rollout [--device-backward [--device-optimizer]]]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from snac_amd import BatchedDMPEnv, DeviceAdam, DeviceMLP, PPOLoss, RolloutBuffer  # noqa: E402


class ActorCritic(nn.Module):
    def __init__(self, obs_dim, plan_cells, actions, hidden=256):
        super().__init__()
        self.body = nn.Sequential(nn.Linear(obs_dim + plan_cells, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh())
        self.policy = nn.Linear(hidden, actions)
        self.value = nn.Linear(hidden, 1)

    def forward(self, obs, plan):
        h = self.body(torch.cat([obs, plan.flatten(1)], dim=1))
        return self.policy(h), self.value(h).squeeze(1)


class ActorCriticMLP(nn.Module):
    """--device-rollout: the same shape with ReLU and one last layer of actions + 1 outputs, so that a DeviceMLP can run it."""

    def __init__(self, obs_dim, plan_cells, actions, hidden=256):
        super().__init__()
        self.actions = actions
        self.body = nn.Sequential(nn.Linear(obs_dim + plan_cells, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(),
                                  nn.Linear(hidden, actions + 1))

    def forward(self, obs, plan):
        y = self.body(torch.cat([obs, plan.flatten(1)], dim=1))
        return y[:, :self.actions], y[:, self.actions]


def run(envs=4096, iterations=20, horizon=32, epochs=4, batch=8192, gamma=0.99, lam=0.95, clip=0.2, vf_coef=0.5, ent_coef=0.01, lr=3e-4, seed=1,
        log=print, device_sampling=False, device_loss=False, clip_vf=None, info=None, device_rollout=False,
        device_backward=False, device_optimizer=False):
    """-> (the loss of every minibatch update, the mean episodic return after every iteration).  device_sampling: draw the actions and
    their log-probabilities with one launch per tick (RolloutBuffer.act_logits: counter-RNG stream 5, independent of the sharding and of
    torch's generator) instead of torch.distributions.  device_loss: the loss, its gradient and its statistics from PPOLoss (one call per
    minibatch) instead of the torch composition; clip_vf: with device_loss, the clip range of the value function (None: not clipped,
    as the composition).  info: a dict that receives the run's device counters with device_loss ("bad_rows": the samples PPOLoss
    zeroed) and the statistics of the last minibatch ("stats").  device_rollout: the horizon is collected by one fused launch with a DeviceMLP as
    the actor-critic (the module's docstring); the draws are device_sampling's.  device_backward: with device_rollout, the update's pass
    through the network and its weight gradients are the device's (DeviceMLP.train_forward).  device_optimizer: with device_backward, the
    gradient clip and the Adam step are the device's too (DeviceAdam.backward_step: the module's docstring); info then receives
    "bad_steps", the steps refused for a gradient that was not finite."""
    if device_optimizer and not device_backward:
        raise ValueError("device_optimizer needs device_backward: the flat gradient of DeviceMLP.backward")
    if device_backward and not device_rollout:
        raise ValueError("device_backward needs device_rollout: the actor-critic a DeviceMLP can run")
    if clip_vf is not None and not device_loss:
        raise ValueError("clip_vf belongs to device_loss: the torch composition does not clip the value function")
    torch.manual_seed(seed)
    env = BatchedDMPEnv(2, True, envs, seed=seed, obs_dtype=torch.float32)
    dev = env.device
    env.reset()
    buf = RolloutBuffer(env, horizon, gamma, lam)
    net = (ActorCriticMLP if device_rollout else ActorCritic)(env.obs_dim, 400, env.num_actions).to(dev)
    mlp = DeviceMLP(net.body, env) if device_rollout else None
    opt = DeviceAdam(mlp, lr=lr, max_norm=0.5) if device_optimizer else torch.optim.Adam(net.parameters(), lr=lr)
    ppo = PPOLoss(env, clip, -1.0 if clip_vf is None else clip_vf, vf_coef, ent_coef) if device_loss else None
    t0, losses, returns = time.time(), [], []
    for it in range(iterations):
        if device_rollout:
            buf.collect_policy(mlp, horizon)                       # observe -> network -> draw -> step, the whole horizon in one launch
        for _ in range(0 if device_rollout else horizon):
            with torch.no_grad():
                logits, value = net(env.observe().float(), env.input_plan().float())     # resets change plans
                if device_sampling:
                    buf.act_logits(logits, value)                                        # draw, log-probability and env tick
                    continue
                dist = torch.distributions.Categorical(logits=logits)
                actions = dist.sample()
                buf.act(actions.to(torch.int8), value, dist.log_prob(actions))           # one env tick, recorded in the ring (auto-reset)
        with torch.no_grad():
            if device_rollout:
                bootstrap = mlp.forward(torch.cat([env.observe().float(), env.input_plan().float().flatten(1)], dim=1))[:, env.num_actions]
            else:
                _, bootstrap = net(env.observe().float(), env.input_plan().float())
        buf.finish(bootstrap)                                      # advantages and returns of the horizon: one launch
        for mb in buf.minibatches(batch, epochs):                  # one gather launch each
            if device_optimizer:                                   # no autograd node for the network: y is the leaf the loss differentiates
                x = torch.cat([mb["s"], mb["plan"].flatten(1)], dim=1)
                y = mlp.forward(x).requires_grad_()
                logits, value = y[:, :env.num_actions].contiguous(), y[:, env.num_actions].contiguous()
            elif device_backward:
                y = mlp.train_forward(torch.cat([mb["s"], mb["plan"].flatten(1)], dim=1))
                logits, value = y[:, :env.num_actions].contiguous(), y[:, env.num_actions].contiguous()     # what PPOLoss reads
            else:
                logits, value = net(mb["s"], mb["plan"])
            if device_loss:
                loss = ppo.loss(logits, value, mb)                 # the mean loss, carrying its closed-form gradient
            else:
                dist = torch.distributions.Categorical(logits=logits)
                ratio = torch.exp(dist.log_prob(mb["action"]) - mb["logp"])
                surrogate = torch.min(ratio * mb["adv"], torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * mb["adv"]).mean()
                value_loss = 0.5 * ((value - mb["ret"]) ** 2).mean()
                loss = -surrogate + vf_coef * value_loss - ent_coef * dist.entropy().mean()
            if device_optimizer:
                loss.backward()                                    # leaves y.grad
                opt.backward_step(x, y.grad)                       # weight gradients, norm, clip and Adam: five launches
                losses.append(float(loss.detach()))
                continue
            opt.zero_grad(set_to_none=True)
            loss.backward()
            nn.utils.clip_grad_norm_(net.parameters(), 0.5)
            opt.step()
            losses.append(float(loss.detach()))
        st = env.episodic_stats()
        returns.append(st["return_sum"] / max(st["episodes"], 1))
        log("iteration %3d  loss %.4f  episodes %d  mean return %.2f  mean IoU %.4f  (%.0f env-steps/s incl. learning)" % (
            it + 1, losses[-1], st["episodes"], returns[-1], st["iou_fx_sum"] / 2.0**40 / max(st["episodes"], 1),
            envs * horizon * (it + 1) / (time.time() - t0)))
        if device_loss:
            st = ppo.stats_dict()
            log("               approx KL %.5f  clip fraction %.3f  entropy %.4f  value loss %.4f" % (
                st["approx_kl"], st["clip_fraction"], st["entropy"], st["value_loss"]))
    if info is not None and device_loss:
        info.update(bad_rows=int(ppo.bad_rows.cpu()[0]), stats=ppo.stats_dict())
    if info is not None and device_optimizer:
        info["bad_steps"] = int(opt.bad_steps.cpu()[0])
    return losses, returns


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--device-sampling", action="store_true", help="draw the actions on the device from the counter RNG (act_logits)")
    ap.add_argument("--device-loss", action="store_true", help="the loss, its gradient and its statistics from one device call (PPOLoss)")
    ap.add_argument("--clip-vf", type=float, default=None, help="with --device-loss: clip the value function by this range, as PPO2 does")
    ap.add_argument("--device-rollout", action="store_true", help="collect the horizon in one fused launch with a DeviceMLP actor-critic")
    ap.add_argument("--device-backward", action="store_true", help="with --device-rollout: the update's forward pass and weight gradients from the device")
    ap.add_argument("--device-optimizer", action="store_true", help="with --device-backward: the gradient clip and the Adam step from the device (DeviceAdam)")
    a = ap.parse_args()
    if a.device_optimizer and not a.device_backward:
        ap.error("--device-optimizer needs --device-backward")
    if a.device_backward and not a.device_rollout:
        ap.error("--device-backward needs --device-rollout")
    run(a.envs, a.iterations, a.horizon, a.epochs, a.batch, device_sampling=a.device_sampling, device_loss=a.device_loss, clip_vf=a.clip_vf,
        device_rollout=a.device_rollout, device_backward=a.device_backward, device_optimizer=a.device_optimizer)
