"""Phases of a batched UCT iteration (snac_amd/uct.py: UCTSearch) timed with HIP events on the env's stream, at B = 4096 trees of
512 nodes: select (k_uct_select), transition (the B tree edges), evaluate (the leaves' first reward + k_eval), backup (k_uct_backup),
and the whole iteration.  Each window is R iterations ending after 64 and after 512 iterations, so that the trees have grown deeper.

  phase rows     events between the four phases of each of the R iterations, mean per iteration
  iteration      run(R) between two events, no events inside (what a caller sees), mean per iteration
  select+backup  their share of the iteration's device time (the events-inside sum)

    python tools/uct_time.py [--kinds 2,3,1] [--trees 4096] [--nodes 512] [--window 16]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from snac_amd import BatchedDMPEnv, UCTSearch  # noqa: E402

HORIZON = {2: 600, 3: 200, 1: 300}
PHASES = ("select", "transition", "evaluate", "backup")


def window(search, R):
    """(per-phase mean ms, whole-iteration mean ms) over R iterations each way."""
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(5)] for _ in range(R)]
    with torch.cuda.device(search.env.device):
        for i in range(R):
            e = ev[i]
            e[0].record()
            for k, f in enumerate((search._select, search._edges, search._evaluate, search._backup)):
                f()
                e[k + 1].record()
    torch.cuda.synchronize()
    phase = [sum(ev[i][k].elapsed_time(ev[i][k + 1]) for i in range(R)) / R for k in range(4)]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    search.run(R)
    b.record()
    torch.cuda.synchronize()
    return phase, a.elapsed_time(b) / R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="2,3,1")
    ap.add_argument("--trees", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=512)
    ap.add_argument("--window", type=int, default=16)
    args = ap.parse_args()
    B, cap, R = args.trees, args.nodes, args.window
    marks = (64, 512)
    print("B = %d trees x %d nodes, %d-iteration windows ending after %s iterations; times are device ms per iteration" % (B, cap, R, marks))
    for kind in [int(k) for k in args.kinds.split(",")]:
        H = HORIZON[kind]
        env = BatchedDMPEnv(kind, True, B, seed=1)
        env.reset()
        search = UCTSearch(env, cap, H, 0.99, max_iterations=max(marks))
        search.reset()
        torch.cuda.synchronize()
        print("\n%dD dynamic, H = %d" % (kind, H))
        print("  after  " + "".join("%12s" % p for p in PHASES) + "%12s%12s%16s%14s" % ("sum", "iteration", "select+backup", "mean depth"))
        for mark in marks:
            search.run(mark - 2 * R - search.iterations)                 # two windows end at the mark
            phase, whole = window(search, R)
            par, used = search.parent.cpu().numpy(), search.tree_sizes().cpu().numpy()   # mean depth of the allocated nodes of 64 sampled trees
            d = np.zeros(par.size, dtype=np.int64)
            rows = [b * cap + j for b in range(0, B, max(1, B // 64)) for j in range(int(used[b]))]
            for x in rows:                                           # allocation order: a parent before its children
                p = int(par[x])
                d[x] = d[p] + 1 if p >= 0 else 0
            depth = float(d[rows].mean())
            s = sum(phase)
            print("  %5d  " % search.iterations + "".join("%12.4f" % p for p in phase)
                  + "%12.4f%12.4f%15.1f%%%14.2f" % (s, whole, 100.0 * (phase[0] + phase[3]) / s, depth))
        del search, env
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
