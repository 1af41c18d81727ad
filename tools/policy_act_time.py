"""Acting from a policy (snac_policy_act in snac_amd/csrc/k_policy.hip; BatchedDMPEnv.sample_actions / epsilon_greedy,
RolloutBuffer.act_logits): device time over back-to-back calls, the median of five timed groups with min / max.  The reference of every
comparison is the torch composition the examples had before, on the same tensors, in the same process, its groups taking turns with the
new call's.

  part 1      the categorical mode with logp and entropy beside Categorical(logits=...), .sample(), .log_prob(), .entropy() and the cast to
              int8, at N = 1024 and 65 536 for A = 3 (1D) and A = 8 (3D): the C entry point alone into reused outputs, and
              env.sample_actions(want_entropy=True), which allocates its three outputs as the composition does.
  part 2      the epsilon-greedy mode (env.epsilon_greedy(q, 0.1)) beside argmax, torch.rand, torch.randint, torch.where and the cast, at
              the same shapes.
  part 3      one policy tick of examples/ppo_batched.py -- network forward, acting, RolloutBuffer.act / act_logits -- with and without
              device_sampling, at 4096 and 65 536 envs (2D dynamic).
Every part is a child process under its own time limit; the first child that fails ends the run.

    python tools/policy_act_time.py
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from snac_amd import BatchedDMPEnv, RolloutBuffer, _lib  # noqa: E402

SHAPES = ((1, 1024), (1, 65536), (3, 1024), (3, 65536))             # kind (A = 3 / 8), N
TICK_ENVS = (4096, 65536)
GROUPS = 5
REPS, TICK_REPS = 2000, 200                                          # calls per timed window: parts 1 and 2, part 3
EPSILON = 0.1
LIMIT = 300                                                          # seconds per child process


def timed(calls, reps):
    """{label: [ms per call] * GROUPS}: per group every call in turn, `reps` back-to-back calls between two events."""
    for call in calls.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    out = {k: [] for k in calls}
    for _ in range(GROUPS):
        for label, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                call()
            b.record()
            torch.cuda.synchronize()
            out[label].append(a.elapsed_time(b) / reps)
    return out


def torch_categorical(logits):
    d = torch.distributions.Categorical(logits=logits)
    a = d.sample()
    return a.to(torch.int8), d.log_prob(a), d.entropy()


def torch_epsilon_greedy(q, eps):
    """examples/dqn_batched.py without device_sampling"""
    n, A = q.shape
    greedy = q.argmax(dim=1)
    explore = torch.rand(n, device=q.device) < eps
    return torch.where(explore, torch.randint(0, A, (n,), device=q.device), greedy).to(torch.int8)


def _env(kind, N):
    env = BatchedDMPEnv(kind, False, N, seed=1)
    env.reset()
    g = torch.Generator(device=env.device).manual_seed(N + kind)
    return env, 2.0 * torch.randn((N, env.num_actions), device=env.device, generator=g)


def part1():
    out = {}
    for kind, N in SHAPES:
        env, logits = _env(kind, N)
        dev, what = env.device, "N = %d, A = %d" % (N, env.num_actions)
        action, logp, entropy = torch.empty(N, dtype=torch.int8, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
        vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        desc, L = C.byref(env._desc), env._lib

        def raw():
            _lib.check(L.snac_policy_act(desc, N, 0, _lib.POLICY_CATEGORICAL, vp(logits), 0.0, None, vp(action), vp(logp), vp(entropy), None, stream))
        with torch.cuda.device(dev):
            a, lp, en = env.sample_actions(logits, want_entropy=True)
            p = torch.softmax(logits.double(), dim=1)                # what the draw's logp and entropy must be, to float32 rounding
            want_lp, want_en = torch.log(p.gather(1, a.long()[:, None])[:, 0]), -(p * torch.log(p)).sum(dim=1)
            if float((lp.double() - want_lp).abs().max()) > 1e-5 or float((en.double() - want_en).abs().max()) > 1e-5:
                raise SystemExit("logp / entropy are not the softmax's at %s" % what)
            out.update({"%s, %s" % (k, what): v for k, v in timed({
                "snac_policy_act into reused outputs": raw,
                "env.sample_actions(want_entropy=True)": lambda: env.sample_actions(logits, want_entropy=True),
                "torch Categorical: sample, log_prob, entropy, cast": lambda: torch_categorical(logits)}, REPS).items()})
    return out


def part2():
    out = {}
    for kind, N in SHAPES:
        env, q = _env(kind, N)
        what = "N = %d, A = %d" % (N, env.num_actions)
        with torch.cuda.device(env.device):
            if not torch.equal(env.epsilon_greedy(q, 0.0).long(), q.argmax(dim=1)):
                raise SystemExit("epsilon_greedy(q, 0) is not the argmax at %s" % what)
            out.update({"%s, %s" % (k, what): v for k, v in timed({
                "env.epsilon_greedy(q, %.1f)" % EPSILON: lambda: env.epsilon_greedy(q, EPSILON),
                "torch argmax, rand, randint, where, cast": lambda: torch_epsilon_greedy(q, EPSILON)}, REPS).items()})
    return out


def part3():
    spec = importlib.util.spec_from_file_location("ppo_batched", os.path.join(ROOT, "examples", "ppo_batched.py"))
    ppo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ppo)
    out = {}
    for N in TICK_ENVS:
        torch.manual_seed(1)
        env = BatchedDMPEnv(2, True, N, seed=1, obs_dtype=torch.float32)
        env.reset()
        buf = RolloutBuffer(env, 32, 0.99, 0.95)
        net = ppo.ActorCritic(env.obs_dim, 400, env.num_actions).to(env.device)

        def tick(device_sampling):
            with torch.no_grad():
                logits, value = net(env.observe().float(), env.input_plan().float())
                if device_sampling:
                    buf.act_logits(logits, value)
                else:
                    dist = torch.distributions.Categorical(logits=logits)
                    actions = dist.sample()
                    buf.act(actions.to(torch.int8), value, dist.log_prob(actions))
        with torch.cuda.device(env.device):
            out.update({"%s, %d envs" % (k, N): v for k, v in timed({
                "policy tick, device_sampling=True": lambda: tick(True),
                "policy tick, device_sampling=False": lambda: tick(False)}, TICK_REPS).items()})
    return out


PARTS = dict(part1=part1, part2=part2, part3=part3)


def child(part):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", part], capture_output=True, text=True, timeout=LIMIT)
    if out.returncode != 0:                                          # nothing more is started on the device after a failure
        sys.stderr.write(out.stderr[-4000:])
        raise SystemExit("the worker for %s ended with status %d" % (part, out.returncode))
    return json.loads(out.stdout.strip().splitlines()[-1])


def show(rows):
    for label, t in rows.items():
        print("    %-80s median %9.4f   min %9.4f   max %9.4f" % (label, float(np.median(t)), min(t), max(t)), flush=True)
    return {k: float(np.median(t)) for k, t in rows.items()}


def ratios(med, old, new, shapes):
    for what in shapes:
        print("    %s: %s / %s  %.2f" % (what, old, new, med["%s, %s" % (old, what)] / med["%s, %s" % (new, what)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:
        print(json.dumps(PARTS[args.worker]()))
        return
    shapes = ["N = %d, A = %d" % (N, {1: 3, 3: 8}[kind]) for kind, N in SHAPES]
    print("ms per call on the device, %d groups of back-to-back calls, the rows of a shape taking turns group by group" % GROUPS)
    print("  part 1: a categorical action with its log-probability and its entropy")
    med = show(child("part1"))
    ratios(med, "torch Categorical: sample, log_prob, entropy, cast", "env.sample_actions(want_entropy=True)", shapes)
    ratios(med, "torch Categorical: sample, log_prob, entropy, cast", "snac_policy_act into reused outputs", shapes)
    print("  part 2: an epsilon-greedy action, epsilon %.1f" % EPSILON)
    med = show(child("part2"))
    ratios(med, "torch argmax, rand, randint, where, cast", "env.epsilon_greedy(q, %.1f)" % EPSILON, shapes)
    print("  part 3: one policy tick of examples/ppo_batched.py (network forward, acting, act): 2D dynamic, float32 observations")
    med = show(child("part3"))
    ratios(med, "policy tick, device_sampling=False", "policy tick, device_sampling=True", ["%d envs" % N for N in TICK_ENVS])


if __name__ == "__main__":
    main()
