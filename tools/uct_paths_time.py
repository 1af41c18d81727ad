"""K paths per tree and iteration (UCTSearch(paths=K), snac_amd/uct.py) timed with HIP events on the env's stream.

  part 1  the purpose: few wide trees.  2D dynamic, H = 100, B = 64 trees of 8192 nodes, the same 4096 leaf evaluations per tree
          spent as 4096 x paths=1, 256 x 16 and 64 x 64.  Per configuration: R repeats of reset() + run(n) between two events (the
          total a caller sees), then one pass with events between the four phases of every iteration, the tree sizes and the mean
          depth of the allocated nodes.  --reference-root DIR times run(4096) of the build in DIR (another checkout of this
          repository, built; it needs no `paths` argument) in a child process of the same session, before and after this build's rows.
  part 3  what it does to play (reported, not gated): one 2D dynamic episode per env, B = 16, 512 nodes per tree, H = 100, 64 leaf
          evaluations per move as 64 x 1, 16 x 4 and 4 x 16 paths, virtual_loss 0 and --virtual-loss: mean episodic reward, mean final
          IoU, wall time.
  (part 2, no cost where paths is not used, is tools/uct_time.py run on both builds in one session.)

    python tools/uct_paths_time.py [--parts 1,3] [--repeat 5] [--reference-root DIR] [--virtual-loss 0.5]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                                             # a worker of --reference-root imports that build instead
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--root") + 1]))
else:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from snac_amd import BatchedDMPEnv, UCTSearch  # noqa: E402

PHASES = ("select", "transition", "evaluate", "backup")
B1, CAP1, H1, LEAVES = 64, 8192, 100, 4096


def make(B, cap, H, n, K, vl=0.0, seed=1):
    env = BatchedDMPEnv(2, True, B, seed=seed)
    env.reset()
    kw = {} if K == 1 else dict(paths=K, virtual_loss=vl)            # K == 1: the call a build without `paths` accepts
    search = UCTSearch(env, cap, H, 0.99, max_iterations=n, **kw)
    return env, search


def totals(search, n, R):
    """Device ms of run(n) after reset(), R times."""
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


def phases(search, n):
    """Device ms per phase summed over n iterations (events between the phases)."""
    search.reset()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(5)] for _ in range(n)]
    with torch.cuda.device(search.env.device):
        for i in range(n):
            e = ev[i]
            e[0].record()
            for k, f in enumerate((search._select, search._edges, search._evaluate, search._backup)):
                f()
                e[k + 1].record()
    torch.cuda.synchronize()
    return [sum(ev[i][k].elapsed_time(ev[i][k + 1]) for i in range(n)) for k in range(4)]


def shape(search):
    """(mean tree size, mean depth of the allocated nodes) over every tree."""
    par, used = search.parent.cpu().numpy(), search.tree_sizes().cpu().numpy()
    cap = search.nodes_per_tree
    d = np.zeros(par.size, dtype=np.int64)
    rows = [b * cap + j for b in range(search.trees) for j in range(int(used[b]))]
    for x in rows:                                                   # allocation order: a parent before its children
        p = int(par[x])
        d[x] = d[p] + 1 if p >= 0 else 0
    return float(used.mean()), float(d[rows].mean())


def measure(K, R, with_phases=True):
    n = LEAVES // K
    env, search = make(B1, CAP1, H1, n, K)
    search.reset()
    search.run(min(n, 8))                                            # warm-up: every kernel and torch op of the timed window
    torch.cuda.synchronize()
    t = totals(search, n, R)
    size, depth = shape(search)
    ph = phases(search, n) if with_phases else None
    return dict(K=K, n=n, totals=t, phases=ph, size=size, depth=depth)


def row(label, m):
    t = m["totals"]
    s = "  %-26s %5d x %-3d" % (label, m["n"], m["K"]) + "".join("%9.1f" % x for x in t) + "%10.1f%8.1f" % (float(np.mean(t)), max(t) - min(t))
    if m["phases"]:
        s += "  |" + "".join("%9.1f" % p for p in m["phases"])
    print(s + "  |%9.0f%7.2f" % (m["size"], m["depth"]), flush=True)


def reference(root, R):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--worker", "--repeat", str(R)], check=True,
                         capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def part1(R, ref_root):
    print("part 1: 2D dynamic, H = %d, B = %d trees x %d nodes, %d leaf evaluations per tree; device ms (HIP events)" % (H1, B1, CAP1, LEAVES))
    print("  %-26s %-11s" % ("", "iter x K") + "".join("%9s" % ("run %d" % i) for i in range(R)) + "%10s%8s" % ("mean", "spread")
          + "  |" + "".join("%9s" % p[:8] for p in PHASES) + "  |%9s%7s" % ("nodes", "depth"))
    ref = []
    if ref_root:
        ref.append(reference(ref_root, R))
        row("reference build", ref[-1])
    ours = [measure(K, R) for K in (1, 16, 64)]
    for m in ours:
        row("this build, paths=%d" % m["K"], m)
    if ref_root:
        ref.append(reference(ref_root, R))
        row("reference build (again)", ref[-1])
        rt = [x for m in ref for x in m["totals"]]
        base, spread = float(np.mean(rt)), max(max(m["totals"]) - min(m["totals"]) for m in ref)
        print("  reference: mean %.1f ms, spread (max - min of five repeats, the larger of the two visits) %.1f ms; paths=1 of this build: "
              "mean %.1f ms" % (base, spread, float(np.mean(ours[0]["totals"]))))
        for m in ours[1:]:
            mean = float(np.mean(m["totals"]))
            print("  paths=%-3d mean %.1f ms: reference / this = %.2f, saves %.1f ms (%s the spread)"
                  % (m["K"], mean, base / mean, base - mean, "more than" if base - mean > spread else "NOT more than"))


def play(per, K, vl, B=16, H=100):
    env = BatchedDMPEnv(2, True, B, seed=7)
    env.reset()
    moves = env.sizes.total_step
    kw = {} if K == 1 else dict(paths=K, virtual_loss=vl)
    search = UCTSearch(env, 512, H, 0.99, max_iterations=per * moves + per, **kw)
    search.reset()
    total = torch.zeros(B, dtype=torch.float64, device=env.device)
    alive = torch.ones(B, dtype=torch.bool, device=env.device)
    played = 0
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(moves):
        search.run(per)
        r, d = search.advance(search.best_actions(), check=False)
        total += torch.where(alive, r.to(torch.float64), torch.zeros_like(total))
        alive &= ~d
        played += 1
        if played % 20 == 0 and not bool(alive.any()):
            break
    search.store_roots()
    iou = env.iou()
    torch.cuda.synchronize()
    return float(total.mean()), float(iou.mean()), played, time.time() - t0


def part3(vl):
    print("\npart 3: one 2D dynamic episode per env, B = 16, 512 nodes per tree, H = 100, 64 leaf evaluations per move")
    print("  %-12s %13s %14s %14s %8s %8s" % ("iter x paths", "virtual_loss", "mean reward", "mean IoU", "moves", "wall s"))
    for per, K, v in ((64, 1, 0.0), (16, 4, 0.0), (16, 4, vl), (4, 16, 0.0), (4, 16, vl)):
        r, iou, n, wall = play(per, K, v)
        print("  %5d x %-4d %13.2f %14.4f %14.4f %8d %8.1f" % (per, K, v, r, iou, n, wall), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,3")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--reference-root", default=None)
    ap.add_argument("--virtual-loss", type=float, default=0.5)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:                                                  # the reference build's run(4096), one JSON line
        print(json.dumps(measure(1, args.repeat, with_phases=False)))
        return
    parts = [int(p) for p in args.parts.split(",")]
    if 1 in parts:
        part1(args.repeat, args.reference_root)
    if 3 in parts:
        part3(args.virtual_loss)


if __name__ == "__main__":
    main()
