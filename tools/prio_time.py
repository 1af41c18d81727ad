"""Prioritised replay (snac_amd/priority.py: PriorityTree; snac_amd/csrc/k_prio.hip): what update(), fill() and sample() cost per call,
against the two ways to draw the same minibatch with torch alone, and what the tree adds to a self-play move.

  part 1      us per call (HIP events on the current stream; five windows of 20 calls, warm; the median, the mean and the spread) at
              entries = 512 x 64 and 512 x 4096 (capacity_moves = 512 of B = 64 and B = 4096 trees):
                update     n = 1024 and 4096 distinct random entries (snac_prio_update: 2 + levels launches)
                fill       B = 64 and 4096 contiguous entries with the largest weight (snac_prio_fill: 1 + levels launches)
                sample     n = 1024 and 4096, stratified (snac_prio_sample alone, one launch, and PriorityTree.sample() with its two
                           output allocations and the int64 conversion)
                baselines  the same n draws from a float32 priority vector of the same size: torch.multinomial(p, n, replacement=True),
                           and cumsum + searchsorted (torch.cumsum(p, 0), n uniform positions scaled by the total, torch.searchsorted)
              and the ratio baseline / PriorityTree.sample() of the medians.
  part 2      wall ms per move of play(moves, iterations) between two synchronisations, each row a child process of its own under a
              time limit, at the two shapes of tools/reanalyse_time.py: --reference-root DIR (another checkout of this repository,
              built: the parent commit), this build with prioritized=False, this build with prioritized=True, and the reference again --
              the spread of the two reference rows is the noise the difference has to be read against.  The first child that fails
              ends the run.

    python tools/prio_time.py [--moves 24] [--iterations 32] [--reference-root DIR] [--skip-play]
"""
import argparse
import ctypes as C
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

from snac_amd import BatchedDMPEnv, SelfPlay, UCTSearch, _lib  # noqa: E402

SHAPES = ((64, 8192, 16), (4096, 512, 1))                            # B, cap, K
CAPACITY = 512
GROUPS, REPS = 5, 20
LIMIT = 420                                                          # seconds per child process


def mlp(env, hidden=128):
    A = env.num_actions
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Linear(env.obs_dim, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, A + 1)).to(env.device)

    @torch.no_grad()
    def fn(obs):
        y = net(obs.to(torch.float32))
        return torch.softmax(y[:, :A], 1), torch.tanh(y[:, A])
    return fn


def make(B, cap, K, n):
    """tools/selfplay_time.py's env and PUCT search: a third of the episodes end within the first 18 moves."""
    env = BatchedDMPEnv(2, True, B, seed=1)
    env.reset()
    cs = env._hdr.view(torch.int16).view(B, 8)[:, 3]
    ends = torch.arange(B, device=env.device)
    cs[0::3] = (env.total_step - 2 - ends[0::3] % 16).to(torch.int16)
    kw = dict(paths=K) if K > 1 else {}
    search = UCTSearch(env, cap, 0, 0.99, max_iterations=(env.total_step + 1) * n, evaluator=mlp(env), **kw)
    search.reset()
    return env, search


def whole(B, cap, K, n, moves, prioritized):
    """Wall ms per move of play(moves, n); prioritized: None (a build without the argument), False or True."""
    env, s = make(B, cap, K, n)
    kw = {} if prioritized is None else dict(prioritized=prioritized)
    play = SelfPlay(s, moves + 2, sample_moves=4, **kw)
    play.play(2, n)                                                  # warm-up: every kernel and torch op of the timed window
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    play.play(moves, n)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / moves


def timed(call):
    call()
    torch.cuda.synchronize()
    out = []
    for _ in range(GROUPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            call()
        b.record()
        torch.cuda.synchronize()
        out.append(1e3 * a.elapsed_time(b) / REPS)
    return out


def calls(B):
    """us per call of the tree's operations and of the torch baselines at entries = CAPACITY * B."""
    from snac_amd.priority import PriorityTree

    dev = torch.device("cuda", 0)
    entries = CAPACITY * B
    g = torch.Generator(device=dev).manual_seed(1)
    tree = PriorityTree(entries, dev, seed=1)
    pri = torch.rand(entries, device=dev, generator=g) + 1e-3        # the float32 priority vector of the baselines
    tree.update(torch.arange(entries, device=dev), pri)
    L, st = tree._lib, tree._stream()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = {}
    with torch.cuda.device(dev):
        for n in (1024, 4096):
            idx = torch.randperm(entries, device=dev, generator=g)[:n].to(torch.int32)
            new = torch.rand(n, device=dev, generator=g)
            out["update, n = %d" % n] = timed(lambda: _lib.check(L.snac_prio_update(*tree._tree, tree.scale_log2, vp(idx), vp(new), n, st)))
        for count in (64, 4096):
            out["fill, %d contiguous" % count] = timed(lambda: _lib.check(L.snac_prio_fill(*tree._tree, tree.scale_log2, 3 * count, count, -1.0, st)))
        for n in (1024, 4096):
            oi, op = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
            out["snac_prio_sample, n = %d" % n] = timed(lambda: _lib.check(L.snac_prio_sample(*tree._tree, 1, 0, 7, n, 1, vp(oi), vp(op), None, st)))
            out["PriorityTree.sample(%d)" % n] = timed(lambda: tree.sample(n))
            out["torch.multinomial, n = %d" % n] = timed(lambda: torch.multinomial(pri, n, replacement=True))

            def by_cumsum():
                c = torch.cumsum(pri, 0)
                return torch.searchsorted(c, torch.rand(n, device=dev) * c[-1]).clamp_(max=entries - 1)
            out["cumsum + searchsorted, n = %d" % n] = timed(by_cumsum)
    return out


def child(cfg, root=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + (["--root", root] if root else []) + ["--worker", json.dumps(cfg)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    if out.returncode != 0:                                          # nothing more is started on the device after a failure
        sys.stderr.write(out.stderr[-4000:])
        raise SystemExit("the worker for %r ended with status %d" % (cfg, out.returncode))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--moves", type=int, default=24)
    ap.add_argument("--iterations", type=int, default=32)
    ap.add_argument("--reference-root", default=None)
    ap.add_argument("--skip-play", action="store_true", help="part 1 only")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:
        cfg = json.loads(args.worker)
        print(json.dumps(calls(cfg[1]) if cfg[0] == "calls" else whole(*cfg[1:])))
        return
    n, moves = args.iterations, args.moves
    for B, _, _ in SHAPES:
        print("entries = %d x %d = %d, scale_log2 = 16" % (CAPACITY, B, CAPACITY * B))
        print("  us per call (HIP events), windows of %d calls" % REPS)
        print("    %-36s" % "" + "".join("%9s" % ("group %d" % i) for i in range(GROUPS)) + "%10s%10s%8s" % ("median", "mean", "spread"))
        got = child(["calls", B])
        for label, t in got.items():
            print("    %-36s" % label + "".join("%9.2f" % x for x in t) + "%10.2f%10.2f%8.2f" % (float(np.median(t)), float(np.mean(t)), max(t) - min(t)),
                  flush=True)
        for k in (1024, 4096):
            ours = float(np.median(got["PriorityTree.sample(%d)" % k]))
            for base in ("torch.multinomial", "cumsum + searchsorted"):
                print("    %-36s%9.1fx" % ("%s / sample(%d)" % (base, k), float(np.median(got["%s, n = %d" % (base, k)])) / ours))
        print(flush=True)
    if args.skip_play:
        return
    for B, cap, K in SHAPES:
        print("2D dynamic PUCT, B = %d trees x %d nodes, paths=%d, %d iterations per move, a ring of %d moves" % (B, cap, K, n, moves))
        print("  wall ms per move of play(%d, %d)" % (moves, n))
        rows = [("prioritized=False", None, False), ("prioritized=True", None, True)]
        if args.reference_root:
            ref = ("reference play()", args.reference_root, None)
            rows = [ref] + rows + [("reference play() (again)",) + ref[1:]]
        got = {}
        for label, root, prio in rows:
            got[label] = child(["whole", B, cap, K, n, moves, prio], root)
            print("    %-36s%10.3f" % (label, got[label]), flush=True)
        print("    %-36s%+10.3f" % ("prioritized=True - False", got["prioritized=True"] - got["prioritized=False"]))
        if args.reference_root:
            base = 0.5 * (got["reference play()"] + got["reference play() (again)"])
            print("    %-36s%+10.3f   (the two reference rows differ by %.3f)"
                  % ("prioritized=True - reference", got["prioritized=True"] - base, abs(got["reference play()"] - got["reference play() (again)"])))
        print(flush=True)


if __name__ == "__main__":
    main()
