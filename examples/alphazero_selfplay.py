"""AlphaZero-style self-play on the device, end to end: a small MLP guides a PUCT search (UCTSearch(evaluator=)), SelfPlay plays
episodes with it and records (observation, visit distribution, return) per move, and the MLP is trained on minibatches of the ring --
cross-entropy to the visit distribution, squared error to the discounted return.  An illustration of the interfaces, not a tuned
trainer: nothing but the final printout crosses the bus.

    python examples/alphazero_selfplay.py [--kind 2] [--envs 64] [--steps 20] [--normalise] [--gumbel M [--gumbel-interior]]
                                          [--reanalyse R] [--td-steps N] [--prioritized [--per-alpha A] [--per-beta B]]
                                          [--device-loss [--huber D] [--vf-coef C]]
                                          [--dirichlet ALPHA [--noise-eps E]] [--temperature T] [--counter-noise]
                                          [--device-evaluator]

--normalise: the search compares q normalised by each tree's min-max bounds (UCTSearch(q_normalise=True)), so that c = 1.25 weighs
the priors against returns of any scale (a brick pays 5 here).
--gumbel M: the Gumbel root search (UCTSearch(gumbel=M), SelfPlay(gumbel=True); it normalises q): M root actions sampled by Gumbel noise
share the 8 iterations of a move by sequential halving, and the policy target is the improved policy, which is above zero for
actions the search never visited.
--gumbel-interior (with --gumbel M): the Gumbel rule below the root too (UCTSearch(gumbel_interior=True)): every node keeps its network
value, selection follows the node's improved policy in place of PUCT, and the policy target uses the full v_mix.
--reanalyse R: the ring keeps every move's root record (SelfPlay(keep_states=True)) and, once per training step, R stored positions drawn
on the device are searched again by a second search of R trees that shares the network, which overwrites their pi and value
(SelfPlay.reanalyse()).
--td-steps N: the value target is the N-step return that bootstraps from the ring's values (targets(td_steps=N)), so that refreshed
values reach z, in place of the return to the end of the episode.
--prioritized: MuZero's prioritised replay (SelfPlay(prioritized=True)): minibatches -- and the positions of --reanalyse -- are drawn in
proportion to |value - z| ** A from a sum tree on the device, the loss is weighted by the importance weights (exponent B), and the
sampled entries get their new priorities after every step (update_priorities()).
--device-loss: the loss, its gradient with respect to both heads, the importance weighting, the mean and the new priorities come from
one device call (SearchLoss: float64, a stated order of the sums) in place of the float32 torch composition and its autograd pass;
--huber D takes Huber's value error with delta D and --vf-coef C weighs the value error (they belong to --device-loss).
--dirichlet ALPHA: AlphaZero's root noise, (1 - E) * priors + E * Dirichlet(ALPHA) with E = --noise-eps (default 0.25), drawn on the
device from the counter RNG before every move's search (SelfPlay(dirichlet=)), in place of the uniform share the default run mixes in.
--temperature T: the sampled moves of an episode are drawn in proportion to N ** (1 / T) (SelfPlay(temperature=)).
--counter-noise (with --gumbel M): the Gumbel noise comes from the counter RNG too (SelfPlay(counter_noise=True)): the run then depends
neither on how the envs are sharded nor on a generator's state.
--device-evaluator: the network that guides the search runs as one launch of the package's own (DeviceMLP: float64 sums in index order,
the parameters read in place), and the search values its leaves in that same launch, in place of the torch evaluator below; training
goes through torch autograd as before.
--device-backward: the training step's pass through the network and the gradients of its weights come from the device as well
(DeviceMLP.train_forward: float64 chains in a stated order); the optimiser stays torch's.
--device-optimizer (needs --device-backward): the Adam step is the device's too.  The training pass is DeviceMLP.forward with no autograd
node behind it, loss.backward() leaves the loss's gradient to the outputs, and DeviceAdam.backward_step turns it into the weight gradients
and the step, written into the parameters where they lie: five launches, the same weights on every run.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from snac_amd import BatchedDMPEnv, DeviceAdam, DeviceMLP, SearchLoss, SelfPlay, UCTSearch  # noqa: E402


def train(kind=2, envs=64, steps=20, moves=4, iterations=8, paths=4, nodes=256, batch=256, capacity=64, hidden=64, seed=1, normalise=False,
          gumbel=None, gumbel_interior=False, reanalyse=0, td_steps=None, prioritized=False, per_alpha=1.0, per_beta=0.4, device_loss=False, huber=None,
          vf_coef=1.0, info=None, dirichlet=None, noise_eps=0.25, temperature=None, counter_noise=False, device_evaluator=False,
          device_backward=False, device_optimizer=False):
    """`steps` rounds of play(moves) -> [reanalyse()] -> targets() -> sample(batch) -> one optimiser step.  Returns (losses, the
    SelfPlay).  info: a dict that receives bad_rows and the last step's statistics of the device loss, and evaluator_bad_rows of the
    device evaluator, and bad_steps of the device optimiser (the steps refused for a gradient that was not finite)."""
    if device_optimizer and not device_backward:
        raise ValueError("device_optimizer needs device_backward: the flat gradient of DeviceMLP.backward")
    if not device_loss and (huber is not None or vf_coef != 1.0):
        raise ValueError("huber and vf_coef belong to device_loss")
    env = BatchedDMPEnv(kind, True, envs, seed=seed)
    env.reset()
    A = env.num_actions
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(env.obs_dim, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, A + 1)).to(env.device)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)

    @torch.no_grad()
    def evaluator(obs):                                              # leaves' observation rows -> (priors, value)
        y = net(obs.to(torch.float32))
        return torch.softmax(y[:, :A], 1), y[:, A]

    if device_evaluator:                                             # the same network, read in place by one launch per evaluation
        evaluator = DeviceMLP(net, env)
    trainer = None
    if device_backward:                                              # refused here if the network is not one a DeviceMLP runs
        trainer = evaluator if device_evaluator else DeviceMLP(net, env)
    if device_optimizer:
        opt = DeviceAdam(trainer, lr=1e-3)

    def noise(priors):                                               # exploration at the roots: the caller's (here: a uniform share)
        return 0.75 * priors + 0.25 / A

    search = UCTSearch(env, nodes, 0, 0.99, c=1.25, paths=paths, evaluator=evaluator, max_iterations=(env.total_step + 1) * iterations,
                       q_normalise=bool(normalise) or gumbel is not None, gumbel=gumbel,
                       gumbel_interior=bool(gumbel_interior))
    search.reset()
    keep = dict(keep_states=True) if reanalyse else {}
    if prioritized:
        keep["prioritized"] = True
    if temperature is not None:
        keep["temperature"] = temperature
    if gumbel is None and dirichlet is not None:                     # the root noise drawn on the device, keyed by the env ids
        play = SelfPlay(search, capacity, sample_moves=8, dirichlet=(dirichlet, noise_eps), **keep)
    elif gumbel is None:
        play = SelfPlay(search, capacity, sample_moves=8, root_noise=noise, **keep)
    else:                                                            # the Gumbel noise of the first moves explores
        play = SelfPlay(search, capacity, sample_moves=8, gumbel=True, **(dict(keep, counter_noise=True) if counter_noise else keep))
    again = None
    if reanalyse:                                                    # a second search over the same env and network: R trees
        again = UCTSearch(env, nodes, 0, 0.99, c=1.25, paths=paths, evaluator=evaluator, max_iterations=iterations, trees=reanalyse,
                          q_normalise=search.q_normalise, gumbel=gumbel, gumbel_interior=bool(gumbel_interior))
    search_loss = SearchLoss(env, vf_coef=vf_coef, huber=huber) if device_loss else None
    losses = []
    for _ in range(steps):
        play.play(moves, iterations)
        if again is not None:
            play.reanalyse(again, iterations, **(dict(prioritized=True) if prioritized else {}))
        play.targets(td_steps=td_steps)
        b = play.sample(batch, **(dict(prioritized=True, beta=per_beta) if prioritized else {}))
        if device_optimizer:                                         # no autograd node for the network: y is the leaf the loss differentiates
            y = trainer.forward(b["obs"]).requires_grad_()
        else:
            y = trainer.train_forward(b["obs"]) if device_backward else net(b["obs"])

        def update(loss):
            if device_optimizer:
                loss.backward()                                      # leaves y.grad
                opt.backward_step(b["obs"], y.grad)                  # weight gradients and Adam: five launches
            else:
                opt.zero_grad()
                loss.backward()
                opt.step()
        if device_loss:                                              # both heads as contiguous tensors; pi, z and the weights are read from b
            loss, _, priority = search_loss.loss(y[:, :A].contiguous(), y[:, A].contiguous(), b, want_per_sample=True)
            if prioritized:
                play.update_priorities(b["index"], priority if per_alpha == 1.0 else priority ** per_alpha)
            update(loss)
            losses.append(loss.detach())
            continue
        if prioritized:                                              # the importance weights undo the sampling bias
            policy_loss = -(b["weight"] * (b["pi"] * torch.log_softmax(y[:, :A], 1)).sum(1)).mean()
            value_loss = (b["weight"] * (y[:, A] - b["z"]) ** 2).mean()
            play.update_priorities(b["index"], (y[:, A].detach() - b["z"]).abs() ** per_alpha)
        else:
            policy_loss = -(b["pi"] * torch.log_softmax(y[:, :A], 1)).sum(1).mean()
            value_loss = ((y[:, A] - b["z"]) ** 2).mean()
        loss = policy_loss + value_loss
        update(loss)
        losses.append(loss.detach())
    if info is not None and device_loss:
        info.update(search_loss.stats_dict(), bad_rows=int(search_loss.bad_rows.cpu()[0]))
    if info is not None and device_optimizer:
        info.update(bad_steps=int(opt.bad_steps.cpu()[0]))
    if info is not None and device_evaluator:
        info.update(evaluator_bad_rows=int(evaluator.bad_rows.cpu()[0]))
    return [float(x) for x in torch.stack(losses).cpu()], play


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", type=int, default=2)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--normalise", action="store_true")
    ap.add_argument("--gumbel", type=int, default=None, metavar="M")
    ap.add_argument("--gumbel-interior", action="store_true")
    ap.add_argument("--reanalyse", type=int, default=0, metavar="R", help="stored positions searched again per training step (default: none)")
    ap.add_argument("--td-steps", type=int, default=None, metavar="N", help="the N-step value target (default: the return to the episode's end)")
    ap.add_argument("--prioritized", action="store_true", help="prioritised replay: sample and reanalyse in proportion to |value - z| ** alpha")
    ap.add_argument("--per-alpha", type=float, default=1.0, metavar="A", help="the priority exponent (default 1, MuZero's)")
    ap.add_argument("--per-beta", type=float, default=0.4, metavar="B", help="the exponent of the importance weights (default 0.4)")
    ap.add_argument("--device-loss", action="store_true", help="the loss, its gradient and the new priorities from one device call (SearchLoss)")
    ap.add_argument("--huber", type=float, default=None, metavar="D", help="with --device-loss: Huber's value error with delta D (default: squared)")
    ap.add_argument("--vf-coef", type=float, default=1.0, metavar="C", help="with --device-loss: the weight of the value error (default 1)")
    ap.add_argument("--dirichlet", type=float, default=None, metavar="ALPHA", help="Dirichlet(ALPHA) root noise from the counter RNG (PUCT)")
    ap.add_argument("--noise-eps", type=float, default=0.25, metavar="E", help="with --dirichlet: the noise's share of the root priors (default 0.25)")
    ap.add_argument("--temperature", type=float, default=None, metavar="T", help="draw the sampled moves in proportion to N ** (1 / T) (PUCT)")
    ap.add_argument("--counter-noise", action="store_true", help="with --gumbel M: the Gumbel noise from the counter RNG")
    ap.add_argument("--device-evaluator", action="store_true", help="the search's network as one device launch (DeviceMLP), fused into the search")
    ap.add_argument("--device-backward", action="store_true", help="the training step's forward pass and weight gradients from the device (DeviceMLP)")
    ap.add_argument("--device-optimizer", action="store_true", help="with --device-backward: the Adam step from the device (DeviceAdam)")
    args = ap.parse_args()
    if args.device_optimizer and not args.device_backward:
        ap.error("--device-optimizer needs --device-backward")
    if args.gumbel_interior and args.gumbel is None:
        ap.error("--gumbel-interior needs --gumbel M")
    if args.gumbel is not None and (args.dirichlet is not None or args.temperature is not None):
        ap.error("--dirichlet and --temperature belong to the PUCT run: not with --gumbel")
    if args.counter_noise and args.gumbel is None:
        ap.error("--counter-noise needs --gumbel M")
    if args.noise_eps != 0.25 and args.dirichlet is None:
        ap.error("--noise-eps needs --dirichlet ALPHA")
    if not args.device_loss and (args.huber is not None or args.vf_coef != 1.0):
        ap.error("--huber and --vf-coef need --device-loss")
    losses, play = train(kind=args.kind, envs=args.envs, steps=args.steps, normalise=args.normalise, gumbel=args.gumbel,
                         gumbel_interior=args.gumbel_interior, reanalyse=args.reanalyse, td_steps=args.td_steps,
                         prioritized=args.prioritized, per_alpha=args.per_alpha, per_beta=args.per_beta, device_loss=args.device_loss,
                         huber=args.huber, vf_coef=args.vf_coef, dirichlet=args.dirichlet, noise_eps=args.noise_eps, temperature=args.temperature,
                         counter_noise=args.counter_noise, device_evaluator=args.device_evaluator,
                         device_backward=args.device_backward, device_optimizer=args.device_optimizer)
    print("moves played per tree: %d, samples in the ring: %d, episodes finished: %d" % (play.moves, len(play), int(play.done.sum())))
    if args.reanalyse:
        print("entries reanalysed: %d" % int(play.refreshed.sum()))
    print("loss: first %.4f, last %.4f" % (losses[0], losses[-1]))


if __name__ == "__main__":
    main()
