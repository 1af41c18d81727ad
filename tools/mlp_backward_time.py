"""The backward pass of the device network (DeviceMLP.backward / train_forward, snac_amd/mlp.py; k_mlp_grad.hip) beside the same network
through torch autograd, timed with HIP events on the current stream.  Medians of five groups; parts 1 and 2 are device time between two
events, parts 3 and 4 wall time of whole example runs (they step envs and talk to the host).

  part 1      snac_mlp_backward alone (DeviceMLP.backward into a kept buffer) for [51, 64, 6] and [451, 256, 256, 6] at 256, 2048, 8192
              and 65 536 rows of float32 values.
  part 2      one training pass -- forward, SearchLoss, backward to every weight -- as train_forward + the device loss + .backward()
              and as the torch module + the same device loss + .backward(), same networks and rows.
  part 3      the three examples for a few updates with and without --device-backward (the other flags the same on both sides: the
              device loss for DQN and self-play, the device rollout for PPO, whose network a DeviceMLP can run).
  part 4      with --reference-root DIR (another checkout of this repository, built: the parent commit): each example's default run in
              that build, in this build and in that build again, in child processes of the same session -- the default path, which this
              build must not slow down; the reference's two runs give the spread a difference has to exceed.

  --root DIR  import the package from DIR instead (a copy of include/ and snac_amd/ built with another SNAC_MLP_GRAD_CHUNK): parts 1
              and 2 of that build, whose chunk length the table's head line prints.

    python tools/mlp_backward_time.py [--parts 1,2,3,4] [--reference-root DIR] [--root DIR]
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                                             # another build: a worker of --reference-root, or a copy with another chunk length
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--root") + 1]))
else:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

NETS = ((51, 64, 6), (451, 256, 256, 6))
ROWS = (256, 2048, 8192, 65536)
EXAMPLES = (("dqn_batched", "run", dict(envs=1024, ticks=20, batch=2048, prefill=16, replace=1000), dict(device_loss=True)),
            ("ppo_batched", "run", dict(envs=1024, iterations=3, horizon=16, epochs=2, batch=4096), dict(device_rollout=True)),
            ("alphazero_selfplay", "train", dict(kind=2, envs=64, steps=8, moves=4, iterations=8, paths=4, nodes=256, batch=256), dict(device_loss=True)))


def network(dims, dev):
    torch.manual_seed(1)
    mods = []
    for l in range(len(dims) - 1):
        mods += [torch.nn.Linear(dims[l], dims[l + 1])] + ([torch.nn.ReLU()] if l < len(dims) - 2 else [])
    return torch.nn.Sequential(*mods).to(dev)


def groups(call, reps, n=5):
    """Device ms per call: n groups of `reps` calls between two events."""
    call()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out


def cell(t):
    return "%-30s" % ("%9.1f  (%.1f .. %.1f)" % (1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t)))


def parts12(which):
    from snac_amd import DeviceMLP, SearchLoss, _lib

    dev = torch.device("cuda", torch.cuda.current_device())
    A = 5
    print("parts 1 and 2: device us per call (five groups: median, then min .. max); float32 rows; chunk length %d" % _lib.MLP_GRAD_CHUNK)
    print("  %-18s%8s  %-30s%-30s%-30s%s" % ("network", "rows", "snac_mlp_backward", "train_forward + loss + bwd", "torch module + loss + bwd", "device / torch"))
    for dims in NETS:
        net = network(dims, dev)
        mlp = DeviceMLP(net)
        loss = SearchLoss(A, device=dev)
        for rows in ROWS:
            reps = 50 if rows <= 8192 else 10
            x = torch.randn(rows, dims[0], device=dev)
            grad_y = torch.randn(rows, dims[-1], device=dev) / rows
            out = torch.empty(mlp.num_params, device=dev)
            mb = (torch.softmax(torch.randn(rows, A, device=dev), 1).contiguous(), torch.randn(rows, device=dev))

            def device_pass():
                net.zero_grad(set_to_none=True)
                y = mlp.train_forward(x)
                loss.loss(y[:, :A].contiguous(), y[:, A].contiguous(), mb).backward()

            def torch_pass():
                net.zero_grad(set_to_none=True)
                y = net(x)
                loss.loss(y[:, :A].contiguous(), y[:, A].contiguous(), mb).backward()
            cols = [groups(lambda: mlp.backward(x, grad_y, out=out), reps) if 1 in which else None,
                    groups(device_pass, reps) if 2 in which else None, groups(torch_pass, reps) if 2 in which else None]
            ratio = "" if 2 not in which else "%.2f" % (statistics.median(cols[1]) / statistics.median(cols[2]))
            print("  %-18s%8d  " % ("x".join(map(str, dims)), rows) + "".join(cell(t) if t else "%-30s" % "-" for t in cols) + ratio, flush=True)


def example(root, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed_runs(root, name, fn, kw, R=5):
    """Wall ms of R runs of an example's entry point after one warm-up run."""
    mod = example(root, name)
    if "log" in getattr(mod, fn).__code__.co_varnames:
        kw = dict(kw, log=lambda line: None)
    out = []
    for i in range(R + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        getattr(mod, fn)(**kw)
        torch.cuda.synchronize()
        if i:
            out.append(1e3 * (time.perf_counter() - t0))
    return out


def line(label, t):
    print("    %-34s" % label + "".join("%9.1f" % x for x in t) + "%10.1f%8.1f" % (statistics.median(t), max(t) - min(t)), flush=True)
    return statistics.median(t)


def part3():
    print("\npart 3: the examples with and without --device-backward; wall ms of a whole run (five runs after a warm-up: each, median, spread)")
    for name, fn, kw, flags in EXAMPLES:
        print("  %s %s %s" % (name, kw, flags))
        a = line("torch autograd", timed_runs(ROOT, name, fn, dict(kw, **flags)))
        b = line("--device-backward", timed_runs(ROOT, name, fn, dict(kw, device_backward=True, **flags)))
        c = line("torch autograd (again)", timed_runs(ROOT, name, fn, dict(kw, **flags)))
        print("    --device-backward: %.1f ms; torch autograd: %.1f and %.1f ms" % (b, a, c), flush=True)


def worker(root, name, fn, kw):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--worker", json.dumps([name, fn, kw])], check=True,
                         capture_output=True, text=True, timeout=900).stdout
    return json.loads(out.strip().splitlines()[-1])


def part4(ref_root):
    print("\npart 4: each example's default run beside the reference build's, in child processes of this session; wall ms")
    for name, fn, kw, _ in EXAMPLES:
        print("  %s %s" % (name, kw))
        first = line("reference build", worker(ref_root, name, fn, kw))
        mine = line("this build", worker(ROOT, name, fn, kw))
        again = line("reference build (again)", worker(ref_root, name, fn, kw))
        lo, hi = min(first, again), max(first, again)
        print("    this build %.1f ms; the reference's two runs %.1f and %.1f ms: %s" % (mine, first, again, "inside their spread" if lo <= mine <= hi else
              "below both" if mine < lo else "ABOVE both by %.1f ms" % (mine - hi)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--reference-root", default=None)
    ap.add_argument("--root", default=None, help="import the package from this build instead (parts 1 and 2)")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:                                                  # one build's default run of one example, one JSON line
        name, fn, kw = json.loads(args.worker)
        print(json.dumps(timed_runs(os.path.abspath(args.root), name, fn, kw)))
        return
    parts = [int(p) for p in args.parts.split(",")]
    if 1 in parts or 2 in parts:
        parts12(parts)
    if 3 in parts:
        part3()
    if 4 in parts:
        if not args.reference_root:
            raise SystemExit("part 4 needs --reference-root DIR")
        part4(args.reference_root)


if __name__ == "__main__":
    main()
