"""The policy / value network on the device (DeviceMLP, snac_amd/mlp.py; k_mlp.hip) beside the same network through torch, timed with HIP
events on the current stream.  Medians of five groups; every figure is device time between two events.

  part 1      the three entry points -- snac_mlp_forward, snac_mlp_policy_value, snac_mlp_uct_value_leaves -- at 64, 4096 and 65 536
              rows of 51 float64 values, for the example's network [51, 64, 6] and for [51, 256, 256, 6], beside the torch evaluator of
              examples/alphazero_selfplay.py on the same rows (the cast, two or three Linear, ReLU, the slice and the softmax).
  part 2      the PUCT search as tools/uct_puct_time.py runs it, 2D dynamic: B = 4096 trees x 512 nodes, 512 iterations x paths=1, and
              B = 64 trees x 8192 nodes, 256 iterations x paths=16, with the example's network: as a torch callable, as a DeviceMLP
              (the fused launch), and as the torch callable again -- the spread of the reference's two runs is what a difference has to
              exceed.  Columns: R repeats of reset() + run(n), their median; then the evaluate phase (first-reward ops + valuing the
              leaves) of one pass with events between the phases, summed over the iterations.
  part 3      with --reference-root DIR (another checkout of this repository, built: the parent commit): the torch-callable search of
              that build in a child process of the same session, before and after this build's torch-callable search -- the default
              path, which this build must not slow down.

    python tools/mlp_time.py [--repeat 5] [--parts 1,2,3] [--reference-root DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                                             # a worker of --reference-root imports that build instead
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--root") + 1]))
else:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from snac_amd import BatchedDMPEnv, UCTSearch, _lib  # noqa: E402

SEARCHES = ((4096, 512, 1, 512), (64, 8192, 16, 256))                # B, cap, K, iterations
NETS = ((51, 64, 6), (51, 256, 256, 6))
ROWS = (64, 4096, 65536)


def network(dims, dev):
    torch.manual_seed(1)
    mods = []
    for l in range(len(dims) - 1):
        mods += [torch.nn.Linear(dims[l], dims[l + 1])] + ([torch.nn.ReLU()] if l < len(dims) - 2 else [])
    return torch.nn.Sequential(*mods).to(dev)


def torch_evaluator(net, A):
    @torch.no_grad()
    def fn(obs):                                                     # examples/alphazero_selfplay.py's
        y = net(obs.to(torch.float32))
        return torch.softmax(y[:, :A], 1), y[:, A]
    return fn


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


def part1():
    from snac_amd import DeviceMLP

    dev = torch.device("cuda", torch.cuda.current_device())
    A = 5
    print("part 1: device us per call (five groups of 50 calls: median, then min .. max); rows of 51 float64 values, A = 5")
    print("  %-18s%8s  %-28s%-28s%-28s%-28s" % ("network", "rows", "snac_mlp_forward", "snac_mlp_policy_value", "snac_mlp_uct_value_leaves",
                                              "torch evaluator"))
    for dims in NETS:
        net = network(dims, dev)
        mlp = DeviceMLP(net, A)
        fn = torch_evaluator(net, A)
        for rows in ROWS:
            obs = torch.randn(rows, dims[0], dtype=torch.float64, device=dev)
            y = torch.empty((rows, A + 1), dtype=torch.float32, device=dev)
            priors, value = torch.empty((rows, A), dtype=torch.float32, device=dev), torch.empty(rows, dtype=torch.float64, device=dev)
            est = torch.zeros(rows, dtype=torch.float64, device=dev)
            first_has = torch.zeros(rows, dtype=torch.uint8, device=dev)
            first_idx, leaf = torch.zeros(rows, dtype=torch.int32, device=dev), torch.arange(rows, dtype=torch.int32, device=dev)
            done, stats = torch.zeros(rows, dtype=torch.uint8, device=dev), torch.zeros((rows, 64), dtype=torch.int32, device=dev)
            p = _lib.ptr
            L = _lib.lib()

            def leaves():
                _lib.check(L.snac_mlp_uct_value_leaves(mlp._descriptor(), A, p(obs), 1, rows, p(first_has), p(first_idx), p(done), p(stats), rows,
                                                       p(leaf), p(priors), p(value), p(est), p(mlp.bad_rows), mlp._stream()))
            cols = [groups(c, 50) for c in (lambda: mlp.forward(obs, out=y), lambda: mlp.policy_value(obs), leaves, lambda: fn(obs))]
            print("  %-18s%8d  " % ("x".join(map(str, dims)), rows)
                  + "".join("%-28s" % ("%8.1f  (%.1f .. %.1f)" % (1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t))) for t in cols), flush=True)


def make(B, cap, K, n, mode):
    env = BatchedDMPEnv(2, True, B, seed=1)
    env.reset()
    net = network((env.obs_dim, 64, env.num_actions + 1), env.device)
    if mode == "device":
        from snac_amd import DeviceMLP

        fn = DeviceMLP(net, env)
    else:
        fn = torch_evaluator(net, env.num_actions)
    return UCTSearch(env, cap, 0, 0.99, c=1.25, max_iterations=n, evaluator=fn, **({} if K == 1 else dict(paths=K)))


def totals(search, n, R):
    out = []
    for _ in range(R):
        search.reset()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        search.run(n)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def evaluate_phase(search, n):
    """Device ms of the evaluate phase (the first-reward ops and the valuing of the leaves) summed over n iterations."""
    search.reset()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    with torch.cuda.device(search.env.device):
        for a, b in ev:
            search._select()
            search._edges()
            search._observe_leaves()
            a.record()
            search._first_reward()
            search._value_leaves()
            b.record()
            search._backup()
            search._set_priors()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev)


def measure(B, cap, K, n, mode, R):
    search = make(B, cap, K, n, mode)
    search.reset()
    search.run(min(n, 8))                                            # warm-up: every kernel and torch op of the timed window
    torch.cuda.synchronize()
    return dict(totals=totals(search, n, R), evaluate=evaluate_phase(search, n))


def row(label, m):
    t = m["totals"]
    print("    %-34s" % label + "".join("%9.1f" % x for x in t) + "%10.1f%8.1f  |%10.1f" % (statistics.median(t), max(t) - min(t), m["evaluate"]), flush=True)
    return statistics.median(t)


def header(R):
    print("    %-34s" % "" + "".join("%9s" % ("run %d" % i) for i in range(R)) + "%10s%8s  |%10s" % ("median", "spread", "evaluate"))


def part2(R):
    print("\npart 2: the PUCT search, 2D dynamic, the example's network [51, 64, 6]; device ms (HIP events)")
    for B, cap, K, n in SEARCHES:
        print("  B = %d trees x %d nodes, %d iterations x paths=%d" % (B, cap, n, K))
        header(R)
        first = row("torch callable", measure(B, cap, K, n, "torch", R))
        fused = row("DeviceMLP (the fused launch)", measure(B, cap, K, n, "device", R))
        again = row("torch callable (again)", measure(B, cap, K, n, "torch", R))
        gain, spread = min(first, again) - fused, abs(first - again)
        print("    the fused search is %.1f ms %s than the slower-to-beat reference run; the reference's two runs are %.1f ms apart: %s"
              % (abs(gain), "faster" if gain > 0 else "slower", spread, "faster by more than the spread" if gain > spread else "NOT faster by more than the spread"),
              flush=True)


def reference(root, cfg, R):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--worker", json.dumps(cfg), "--repeat", str(R)], check=True,
                         capture_output=True, text=True, timeout=900).stdout
    return json.loads(out.strip().splitlines()[-1])


def part3(R, ref_root):
    print("\npart 3: the default path (a torch callable as the evaluator) beside the reference build's, in child processes of this session")
    for B, cap, K, n in SEARCHES:
        print("  B = %d trees x %d nodes, %d iterations x paths=%d" % (B, cap, n, K))
        header(R)
        cfg = [B, cap, K, n]
        first = row("reference build", reference(ref_root, cfg, R))
        mine = row("this build", reference(ROOT, cfg, R))
        again = row("reference build (again)", reference(ref_root, cfg, R))
        lo, hi = min(first, again), max(first, again)
        print("    this build %.1f ms; the reference's two runs %.1f and %.1f ms: %s" % (mine, first, again, "inside their spread" if lo <= mine <= hi else
              "below both" if mine < lo else "ABOVE both by %.1f ms" % (mine - hi)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--reference-root", default=None)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:                                                  # one build's torch-callable search at one shape, one JSON line
        B, cap, K, n = json.loads(args.worker)
        print(json.dumps(measure(B, cap, K, n, "torch", args.repeat)))
        return
    parts = [int(p) for p in args.parts.split(",")]
    if 1 in parts:
        part1()
    if 2 in parts:
        part2(args.repeat)
    if 3 in parts:
        if not args.reference_root:
            raise SystemExit("part 3 needs --reference-root DIR")
        part3(args.repeat, args.reference_root)


if __name__ == "__main__":
    main()
