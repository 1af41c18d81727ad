"""The Gumbel root search (UCTSearch(gumbel=m), snac_amd/uct.py) beside the normalised PUCT search it extends, timed with HIP events on
the env's stream.  A sibling of tools/uct_puct_time.py at that tool's two extreme shapes.

  shapes      2D dynamic, a constant evaluator (uniform priors, value 0: what the search machinery alone costs).  B = 4096 trees x 512
              nodes with paths=1, and B = 64 trees x 8192 nodes with paths=16; N iterations from reset() per timed group.
  part 1      the selection launch alone: events around every select of a group, us per launch = the group's sum / N, five groups, their
              mean and spread.  Rows: snac_uct_select_puct_norm of --reference-root DIR (another checkout of this repository, built: the
              parent commit) in a child process of the same session, before and after; snac_uct_select_puct_norm of this build;
              snac_uct_select_gumbel with cand all zero (run()); snac_uct_select_gumbel steered by gumbel_begin() / the halving schedule
              with m = 4 and m = A candidates (the HALVE launches are outside the events).
  part 2      snac_uct_gumbel_candidates on the trees part 1 left: BEGIN, HALVE and PICK, five windows of 20 calls, us per call.  A move
              costs one BEGIN, phases - 1 HALVEs and one PICK.

    python tools/uct_gumbel_time.py [--iterations 64] [--reference-root DIR]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                                             # a worker of --reference-root imports that build instead
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--root") + 1]))
else:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from snac_amd import BatchedDMPEnv, UCTSearch  # noqa: E402

SHAPES = ((4096, 512, 1), (64, 8192, 16))                            # B, cap, K
GROUPS = 5


def constant(A):
    def fn(obs):
        S = obs.shape[0]
        return torch.full((S, A), 1.0 / A, dtype=torch.float32, device=obs.device), torch.zeros(S, dtype=torch.float32, device=obs.device)
    return fn


def make(B, cap, K, n, gumbel=None):
    env = BatchedDMPEnv(2, True, B, seed=1)
    env.reset()
    kw = {} if gumbel is None else dict(gumbel=gumbel)
    return UCTSearch(env, cap, 0, 0.99, c=1.25, max_iterations=n, paths=K, evaluator=constant(env.num_actions), q_normalise=True, **kw)


def select_group(search, n, steered):
    """us per selection launch over n iterations from reset(); steered: candidates from noisy scores and the halving schedule."""
    search.reset()
    plan = [(False, 0)] * n
    if steered:
        from snac_amd.uct import gumbel_schedule

        g = torch.Generator(device=search.env.device)
        g.manual_seed(1)
        search.gumbel_begin(search.gumbel_scores(generator=g))
        plan = gumbel_schedule(n, min(search.gumbel, search.num_actions))
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    with torch.cuda.device(search.env.device):
        for (halve, i), (a, b) in zip(plan, ev):
            if halve:
                search._candidates(1)
            a.record()
            if steered:
                search._select(i * search.paths)
            else:
                search._select()
            b.record()
            search._edges()
            search._evaluate()
            search._backup()
            search._set_priors()
    torch.cuda.synchronize()
    return 1e3 * sum(a.elapsed_time(b) for a, b in ev) / n


def select_row(B, cap, K, n, gumbel=None, steered=False):
    search = make(B, cap, K, n, gumbel)
    select_group(search, min(n, 8), steered)                         # warm-up: every kernel and torch op of the timed window
    return [select_group(search, n, steered) for _ in range(GROUPS)], search


def row(label, t):
    print("    %-44s" % label + "".join("%9.2f" % x for x in t) + "%10.2f%8.2f" % (float(np.mean(t)), max(t) - min(t)), flush=True)


def reference(root, cfg):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--worker", json.dumps(cfg)], check=True, capture_output=True,
                         text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def timed(call, reps=20):
    call()
    torch.cuda.synchronize()
    out = []
    for _ in range(GROUPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        torch.cuda.synchronize()
        out.append(1e3 * a.elapsed_time(b) / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--reference-root", default=None)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:                                                  # the reference build's snac_uct_select_puct_norm at one shape, one JSON line
        B, cap, K, n = json.loads(args.worker)
        print(json.dumps(select_row(B, cap, K, n)[0]))
        return
    n = args.iterations
    for B, cap, K in SHAPES:
        A = 5
        print("B = %d trees x %d nodes, paths=%d, %d iterations per group; us per selection launch (HIP events)" % (B, cap, K, n))
        print("    %-44s" % "" + "".join("%9s" % ("group %d" % i) for i in range(GROUPS)) + "%10s%8s" % ("mean", "spread"))
        cfg = [B, cap, K, n]
        if args.reference_root:
            row("reference snac_uct_select_puct_norm", reference(args.reference_root, cfg))
        row("snac_uct_select_puct_norm", select_row(B, cap, K, n)[0])
        row("snac_uct_select_gumbel, cand = 0", select_row(B, cap, K, n, gumbel=4)[0])
        row("snac_uct_select_gumbel, m = 4", select_row(B, cap, K, n, gumbel=4, steered=True)[0])
        t, search = select_row(B, cap, K, n, gumbel=A, steered=True)
        row("snac_uct_select_gumbel, m = %d" % A, t)
        if args.reference_root:
            row("reference snac_uct_select_puct_norm (again)", reference(args.reference_root, cfg))
        print("  snac_uct_gumbel_candidates on these trees; us per call, windows of 20 calls")
        out = torch.empty(B, dtype=torch.int8, device=search.env.device)
        with torch.cuda.device(search.env.device):
            for label, call in (("BEGIN", lambda: search._candidates(0)), ("HALVE", lambda: search._candidates(1)),
                                ("PICK", lambda: search._candidates(2, out))):
                if label == "HALVE":                                 # every window halves full candidate sets
                    full = torch.full_like(search.cand, (1 << A) - 1)

                    def call(inner=call):
                        search.cand.copy_(full)
                        inner()
                    copy = timed(lambda: search.cand.copy_(full))
                    row("  (the copy that refills cand)", copy)
                row("  " + label, timed(call))
        print(flush=True)


if __name__ == "__main__":
    main()
