"""The optimiser step of the device network (DeviceAdam, snac_amd/optim.py; k_adam.hip) beside torch's clip_grad_norm_ and Adam over the
same parameters, timed with HIP events on the current stream.  Medians of five groups with min and max; parts 1 to 3 are device time
between two events, part 4 wall time of whole runs.  Both launches of a step run at the launch rate (P is at most about 2 x 10^5): the
point is the launch count and the stated bytes, not bandwidth, and a column that is host-bound shows the host, not the kernels.

  part 1      snac_mlp_adam_step alone, through ctypes with its arguments made once, for [51, 64, 6] and [451, 256, 256, 6]: the clip on
              and off, with and without a target.
  part 2      DeviceAdam.step(flat) beside clip_grad_norm_ + torch.optim.Adam (the default foreach form) and beside clip_grad_norm_ +
              torch.optim.Adam(fused=True), over the same parameters with their .grad set.
  part 3      one whole update -- mlp.forward + SearchLoss + backward_step -- beside train_forward + the same loss + .backward() +
              clip_grad_norm_ + Adam.step(), both networks at 256, 2048, 8192 and 65 536 rows.  Every group is printed: the column is
              host-bound and bimodal.
  part 4      with --reference-root DIR (another checkout of this repository, built: the parent commit): each example's default run and
              bench.py in that build, in this build and in that build again, in child processes of the same session -- the default paths,
              which run no new code; the reference's two runs give the spread a difference has to exceed.

    python tools/adam_time.py [--parts 1,2,3,4] [--reference-root DIR]
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                                             # another build: a worker of --reference-root
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--root") + 1]))
else:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

NETS = ((51, 64, 6), (451, 256, 256, 6))
ROWS = (256, 2048, 8192, 65536)
EXAMPLES = (("dqn_batched", "run", dict(envs=1024, ticks=20, batch=2048, prefill=16, replace=1000)),
            ("ppo_batched", "run", dict(envs=1024, iterations=3, horizon=16, epochs=2, batch=4096)),
            ("alphazero_selfplay", "train", dict(kind=2, envs=64, steps=8, moves=4, iterations=8, paths=4, nodes=256, batch=256)))
BENCH = ["--gpus", "1", "--steps", "5", "--warmup", "2"]


def network(dims, dev, seed=1):
    torch.manual_seed(seed)
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


def cell(t, width=30):
    return ("%%-%ds" % width) % ("%9.1f  (%.1f .. %.1f)" % (1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t)))


def part1():
    from snac_amd import DeviceAdam, DeviceMLP

    dev = torch.device("cuda", torch.cuda.current_device())
    print("part 1: snac_mlp_adam_step alone, device us per call of two launches (five groups of 200: median, then min .. max)")
    print("  %-18s%8s  %-30s%-30s%-30s%s" % ("network", "P", "no clip, no target", "clip 0.5, no target", "no clip, target 0.005", "clip 0.5, target 0.005"))
    for dims in NETS:
        mlp, tmlp = DeviceMLP(network(dims, dev)), DeviceMLP(network(dims, dev, 2))
        flat = torch.randn(mlp.num_params, device=dev)
        cols = []
        for max_norm, target in ((None, None), (0.5, None), (None, tmlp), (0.5, tmlp)):
            opt = DeviceAdam(mlp, max_norm=max_norm, target=target, tau=0.005)
            opt._state()
            fn, stream = opt._lib.snac_mlp_adam_step, opt._stream()
            p = lambda t: C.c_void_p(t.data_ptr())                   # noqa: E731
            args = (mlp._descriptor(), p(flat), p(opt._m), p(opt._v), 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, opt.max_norm,
                    None if target is None else tmlp._descriptor(), 0.005, p(opt._norm), p(opt._partials), p(opt._bad), stream)
            cols.append(groups(lambda: fn(*args), 200))
        print("  %-18s%8d  " % ("x".join(map(str, dims)), mlp.num_params) + "".join(cell(t) for t in cols), flush=True)


def part2():
    from snac_amd import DeviceAdam, DeviceMLP

    dev = torch.device("cuda", torch.cuda.current_device())
    print("\npart 2: one optimiser step over the same parameters, clip at 0.5; device us per call (five groups of 100: median, then min .. max)")
    print("  %-18s%8s  %-30s%-30s%-30s%s" % ("network", "P", "DeviceAdam.step(flat)", "clip + Adam (foreach)", "clip + Adam(fused=True)", "device / foreach, / fused"))
    for dims in NETS:
        net = network(dims, dev)
        mlp = DeviceMLP(net)
        flat = torch.randn(mlp.num_params, device=dev)
        for p, g in zip(net.parameters(), [g for wb in mlp._views(flat) for g in wb]):
            p.grad = g.clone()
        opt = DeviceAdam(mlp, max_norm=0.5)
        cols = [groups(lambda: opt.step(flat), 100)]
        for kw in (dict(), dict(fused=True)):
            topt = torch.optim.Adam(net.parameters(), lr=1e-3, **kw)

            def torch_step():
                torch.nn.utils.clip_grad_norm_(net.parameters(), 0.5)
                topt.step()
            cols.append(groups(torch_step, 100))
        med = [statistics.median(t) for t in cols]
        print("  %-18s%8d  " % ("x".join(map(str, dims)), mlp.num_params) + "".join(cell(t) for t in cols) + "%.2f, %.2f" % (med[0] / med[1], med[0] / med[2]),
              flush=True)


def part3():
    from snac_amd import DeviceAdam, DeviceMLP, SearchLoss

    dev = torch.device("cuda", torch.cuda.current_device())
    A = 5
    print("\npart 3: one whole update, clip at 0.5; device us per update, every group, then the median")
    print("  device: mlp.forward + SearchLoss + DeviceAdam.backward_step        torch: train_forward + SearchLoss + .backward() + clip_grad_norm_ + Adam.step()")
    for dims in NETS:
        for rows in ROWS:
            reps = 50 if rows <= 8192 else 10
            x = torch.randn(rows, dims[0], device=dev)
            mb = (torch.softmax(torch.randn(rows, A, device=dev), 1).contiguous(), torch.randn(rows, device=dev))
            loss = SearchLoss(A, device=dev)
            net_d, net_t = network(dims, dev), network(dims, dev)
            mlp_d, mlp_t = DeviceMLP(net_d), DeviceMLP(net_t)
            opt_d, opt_t = DeviceAdam(mlp_d, max_norm=0.5), torch.optim.Adam(net_t.parameters(), lr=1e-3)

            def device_update():
                y = mlp_d.forward(x).requires_grad_()
                loss.loss(y[:, :A].contiguous(), y[:, A].contiguous(), mb).backward()
                opt_d.backward_step(x, y.grad)

            def torch_update():
                opt_t.zero_grad(set_to_none=True)
                y = mlp_t.train_forward(x)
                loss.loss(y[:, :A].contiguous(), y[:, A].contiguous(), mb).backward()
                torch.nn.utils.clip_grad_norm_(net_t.parameters(), 0.5)
                opt_t.step()
            d, t = groups(device_update, reps), groups(torch_update, reps)
            show = lambda g: " ".join("%8.1f" % (1e3 * v) for v in g) + "  | %8.1f" % (1e3 * statistics.median(g))      # noqa: E731
            print("  %-18s%8d  device %s    torch %s    device / torch %.2f" % ("x".join(map(str, dims)), rows, show(d), show(t),
                                                                                   statistics.median(d) / statistics.median(t)), flush=True)


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


def worker(root, name, fn, kw):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--worker", json.dumps([name, fn, kw])], check=True,
                         capture_output=True, text=True, timeout=900).stdout
    return json.loads(out.strip().splitlines()[-1])


def bench(root):
    """The JSON result line of one bench.py run in `root`."""
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + BENCH, check=True, capture_output=True, text=True, timeout=900, cwd=root).stdout
    return json.loads([ln for ln in out.strip().splitlines() if ln.startswith("{")][-1])


def verdict(mine, first, again, higher_is_better=False):
    lo, hi = min(first, again), max(first, again)
    if lo <= mine <= hi:
        return "inside their spread"
    worse = mine < lo if higher_is_better else mine > hi
    return ("WORSE than both by %.3g" % (lo - mine if higher_is_better else mine - hi)) if worse else "better than both"


def part4(ref_root):
    print("\npart 4: the default paths beside the reference build's, in child processes of this session")
    for name, fn, kw in EXAMPLES:
        print("  %s %s; wall ms of a whole run (five runs after a warm-up: each, median, spread)" % (name, kw))
        first = line("reference build", worker(ref_root, name, fn, kw))
        mine = line("this build", worker(ROOT, name, fn, kw))
        again = line("reference build (again)", worker(ref_root, name, fn, kw))
        print("    this build %.1f ms; the reference's two runs %.1f and %.1f ms: %s" % (mine, first, again, verdict(mine, first, again)), flush=True)
    print("  bench.py %s: the numeric fields of the result line" % " ".join(BENCH))
    runs = [("reference build", bench(ref_root)), ("this build", bench(ROOT)), ("reference build (again)", bench(ref_root))]
    for label, r in runs:
        print("    %-26s%s" % (label, json.dumps(r, separators=(",", ":"))), flush=True)
    for k, v in runs[1][1].items():
        if isinstance(v, (int, float)) and not isinstance(v, bool) and all(isinstance(r.get(k), (int, float)) for _, r in runs):
            a, b = runs[0][1][k], runs[2][1][k]
            if a != v or b != v:
                print("    %-28s this %-14.6g reference %-14.6g and %-14.6g" % (k, v, a, b), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--reference-root", default=None)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:                                                  # one build's default run of one example, one JSON line
        name, fn, kw = json.loads(args.worker)
        print(json.dumps(timed_runs(os.path.abspath(args.root), name, fn, kw)))
        return
    parts = [int(p) for p in args.parts.split(",")]
    if 1 in parts:
        part1()
    if 2 in parts:
        part2()
    if 3 in parts:
        part3()
    if 4 in parts:
        if not args.reference_root:
            raise SystemExit("part 4 needs --reference-root DIR")
        part4(os.path.abspath(args.reference_root))


if __name__ == "__main__":
    main()
