"""The fused policy rollout (BatchedDMPEnv.rollout_policy, snac_policy_rollout; k_policy_roll.hip) beside the per-tick composition of the
entry points that were there before it, timed with HIP events on the current stream.  Medians of five groups with min .. max; no ratio
was fixed in advance, and the shapes where the fused launch loses are printed like the others.

  part 1      2D dynamic, float32 rows, N = 1024 / 4096 / 65 536 envs, the networks [51, 64, 6] and [451, 256, 256, 6] (observation +
              plan), T = 32 and 600 ticks, the categorical mode.  Fused: one rollout_policy call of T ticks, with obs="last" and (where
              the rows fit in 2 GiB) obs="all".  Composition, per tick: observe + DeviceMLP.forward + sample_actions + step(out=...) with
              preallocated outputs -- the fast path; the wide network's rows come from an env whose layout appends the plan, so that
              observe() writes all 451 values in its one launch; the scores are the first five of the network's six outputs, a slice
              made contiguous (one small copy).  us per tick = the call's device time / T.
  part 2      a collection horizon of examples/ppo_batched.py (4096 envs, 32 ticks, hidden 256): the per-tick loop with
              --device-sampling (observe, input_plan, the torch module, act_logits) and the fused one (--device-rollout:
              RolloutBuffer.collect_policy), host wall-clock around a synchronised horizon, ms.
  part 3      with --reference-root DIR (another checkout of this repository, built: the parent commit): the default run of
              examples/ppo_batched.py (no flag) of that build in a child process, before and after this build's -- the default path,
              which this build must not move.

    python tools/policy_rollout_time.py [--parts 1,2,3] [--reference-root DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                                             # a worker of --reference-root imports that build instead
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from snac_amd import BatchedDMPEnv, _lib  # noqa: E402

NETS = ((51, 64, 6), (451, 256, 256, 6))
SIZES = (1024, 4096, 65536)
TICKS = (32, 600)
ALL_ROWS_MAX_BYTES = 2 << 30


def network(dims, dev):
    torch.manual_seed(1)
    mods = []
    for l in range(len(dims) - 1):
        mods += [torch.nn.Linear(dims[l], dims[l + 1])] + ([torch.nn.ReLU()] if l < len(dims) - 2 else [])
    return torch.nn.Sequential(*mods).to(dev)


def groups(call, n=5):
    """Device ms per call: n single calls, each between two events, after one warm-up call."""
    call()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def cell(ms, T):
    us = [1e3 * x / T for x in ms]
    return "%9.1f  (%.1f .. %.1f)" % (statistics.median(us), min(us), max(us))


def part1():
    from snac_amd import DeviceMLP

    print("part 1: device us per tick (five calls of T ticks: median, then min .. max); 2D dynamic, float32 rows, categorical mode")
    print("  %-18s%8s%6s  %-32s%-32s%-32s%s" % ("network", "envs", "T", "fused, obs='last'", "fused, obs='all'", "per-tick composition", "fused / composition"))
    for dims in NETS:
        for N in SIZES:
            fused_env = BatchedDMPEnv(2, True, N, seed=1, obs_dtype=torch.float32)
            comp_env = BatchedDMPEnv(2, True, N, seed=1, obs_dtype=torch.float32, **(dict(obs_tail=("plan",)) if dims[0] == 451 else {}))
            dev, A = fused_env.device, fused_env.num_actions
            net = network(dims, dev)
            mlp = DeviceMLP(net, fused_env)
            for env in (fused_env, comp_env):
                env.reset()
            rows = torch.empty((N, comp_env.obs_dim), dtype=torch.float32, device=dev)
            y = torch.empty((N, A + 1), dtype=torch.float32, device=dev)
            outs = (torch.empty((N, comp_env.obs_dim), dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev),
                    torch.empty(N, dtype=torch.uint8, device=dev))
            act = (torch.empty(N, dtype=torch.int8, device=dev), torch.empty(N, dtype=torch.float32, device=dev), None)
            L, p = comp_env._lib, lambda t: t.data_ptr()

            def composition(T):
                import ctypes as C

                for _ in range(T):
                    _lib.check(L.snac_observe(C.byref(comp_env._desc), C.byref(comp_env._state), C.c_void_p(p(rows)), comp_env._stream()))
                    mlp.forward(rows, out=y)
                    a, _, _ = comp_env.sample_actions(y[:, :A].contiguous(), out=act)
                    comp_env.step(a, auto_reset=True, out=outs)

            for T in TICKS:
                last = groups(lambda: fused_env.rollout_policy(mlp, T, obs="last", want_value=False))
                whole = None
                if T * N * 51 * 4 <= ALL_ROWS_MAX_BYTES:
                    buf = dict(obs=torch.empty((T, N, 51), dtype=torch.float32, device=dev))
                    whole = groups(lambda: fused_env.rollout_policy(mlp, T, obs="all", want_value=False, out=buf))
                    del buf
                comp = groups(lambda: composition(T))
                ratio = statistics.median(last) / statistics.median(comp)
                print("  %-18s%8d%6d  %-32s%-32s%-32s%.2f%s" % ("x".join(map(str, dims)), N, T, cell(last, T), cell(whole, T) if whole else "      (rows above 2 GiB)",
                                                             cell(comp, T), ratio, "" if ratio < 1.0 else "   <- the fused launch loses"), flush=True)
            del fused_env, comp_env
            torch.cuda.empty_cache()


def horizon_ms(device_rollout, envs=4096, horizon=32, n=5):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import ppo_batched as ex
    from snac_amd import DeviceMLP, RolloutBuffer

    torch.manual_seed(1)
    env = BatchedDMPEnv(2, True, envs, seed=1, obs_dtype=torch.float32)
    env.reset()
    buf = RolloutBuffer(env, horizon, 0.99, 0.95)
    net = (ex.ActorCriticMLP if device_rollout else ex.ActorCritic)(env.obs_dim, 400, env.num_actions).to(env.device)
    mlp = DeviceMLP(net.body, env) if device_rollout else None

    def collect():
        if device_rollout:
            buf.collect_policy(mlp, horizon)
            return
        for _ in range(horizon):
            with torch.no_grad():
                logits, value = net(env.observe().float(), env.input_plan().float())
                buf.act_logits(logits, value)

    collect()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        collect()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def part2():
    print("\npart 2: one collection horizon of examples/ppo_batched.py, 4096 envs x 32 ticks, hidden 256; host wall-clock ms around a synchronised horizon")
    for label, flag in (("per tick, --device-sampling", False), ("fused, --device-rollout", True), ("per tick, --device-sampling (again)", False)):
        t = horizon_ms(flag)
        print("    %-40s%9.2f  (%.2f .. %.2f)   %.3f ms per tick" % (label, statistics.median(t), min(t), max(t), statistics.median(t) / 32), flush=True)


def default_run_ms(n=3):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import ppo_batched as ex

    kw = dict(envs=4096, iterations=2, horizon=32, epochs=1, batch=8192, log=lambda line: None)
    ex.run(**kw)
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        ex.run(**kw)
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def reference(root):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--worker", "default"], check=True, capture_output=True, text=True,
                         timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def part3(ref_root):
    print("\npart 3: the default run of examples/ppo_batched.py (4096 envs, 2 iterations x 32 ticks, 1 epoch; no flag), wall-clock ms of run(), three runs "
          "after a warm-up run, in child processes of this session")
    rows = [("reference build", reference(ref_root)), ("this build", reference(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))),
            ("reference build (again)", reference(ref_root))]
    for label, t in rows:
        print("    %-28s" % label + "".join("%10.1f" % x for x in t) + "   median %.1f" % statistics.median(t), flush=True)
    first, mine, again = (statistics.median(t) for _, t in rows)
    lo, hi = min(first, again), max(first, again)
    print("    this build %.1f ms; the reference's two runs %.1f and %.1f ms: %s" % (mine, first, again, "inside their spread" if lo <= mine <= hi else
          "below both" if mine < lo else "ABOVE both by %.1f ms" % (mine - hi)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2")
    ap.add_argument("--reference-root", default=None)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:
        print(json.dumps(default_run_ms()))
        return
    parts = [int(p) for p in args.parts.split(",")]
    if 1 in parts:
        part1()
    if 2 in parts:
        part2()
    if 3 in parts:
        if not args.reference_root:
            raise SystemExit("part 3 needs --reference-root DIR")
        part3(args.reference_root)


if __name__ == "__main__":
    main()
