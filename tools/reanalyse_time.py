"""Reanalyse (snac_amd/selfplay.py: SelfPlay(keep_states=True), reanalyse(), targets(td_steps=n); snac_amd/csrc/k_uct_reanalyse.hip): what
the four entry points cost per call, and what keeping the states adds to a self-play move.  A sibling of tools/selfplay_time.py at that
tool's two shapes.

  shapes      2D dynamic, the PUCT search (a two-layer MLP).  B = 64 trees x 8192 nodes, paths=16, and B = 4096 trees x 512 nodes,
              paths=1; 32 iterations per move.
  part 1      us per call (HIP events on the env's stream; five windows of 20 calls, their mean and spread) after a play of the ring:
              snac_uct_save_roots of the B roots; snac_uct_load_roots of R = B trees from ring entries drawn on the device;
              snac_uct_store_targets of those trees; snac_uct_returns_nstep (n = 5) beside snac_uct_returns over the same ring.
  part 2      wall ms per move of play(moves, iterations) between two synchronisations, each row a child process of its own under a
              time limit: --reference-root DIR (another checkout of this repository, built: the parent commit), this build with
              keep_states=False, this build with keep_states=True, and the reference again -- the spread of the two reference rows is
              the noise the difference has to be read against.  The first child that fails ends the run.

    python tools/reanalyse_time.py [--moves 24] [--iterations 32] [--reference-root DIR]
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
GROUPS, REPS = 5, 20
TD_STEPS = 5
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


def whole(B, cap, K, n, moves, keep):
    """Wall ms per move of play(moves, n); keep: None (a build without the argument), False or True."""
    env, s = make(B, cap, K, n)
    kw = {} if keep is None else dict(keep_states=keep)
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


def calls(B, cap, K, n, moves):
    """us per call of the four entry points (and snac_uct_returns) on a ring that play() filled."""
    env, s = make(B, cap, K, n)
    play = SelfPlay(s, moves, sample_moves=4, keep_states=True)
    play.play(moves, n)
    kw = dict(paths=K) if K > 1 else {}
    again = UCTSearch(env, cap, 0, 0.99, max_iterations=n, evaluator=s.evaluator, trees=B, **kw)
    index = play.reanalyse(again, 1)                                 # B entries drawn on the device; warm-up of every launch below
    idx = index.to(torch.int32)
    torch.cuda.synchronize()
    L, st = s._lib, env._stream()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    flat = play.state.view(play.cap * B, -1)
    ring = (B, play.cap, 0, play.cap)
    out = {}
    with torch.cuda.device(env.device):
        out["snac_uct_save_roots"] = timed(lambda: _lib.check(L.snac_uct_save_roots(*play._save_args, vp(play.state[0]), st)))
        out["snac_uct_load_roots"] = timed(lambda: _lib.check(L.snac_uct_load_roots(*again._load_args, vp(flat), play.cap * B, vp(idx),
                                                                                   vp(again._used), st)))
        again._run(1)                                                # roots with visits to store
        out["snac_uct_store_targets"] = timed(lambda: _lib.check(L.snac_uct_store_targets(
            again.num_actions, vp(again.stats), again.rows, B, cap, vp(idx), play.cap * B, None, vp(play.pi), vp(play.value), vp(play.refreshed), st)))
        out["snac_uct_returns_nstep, n = %d" % TD_STEPS] = timed(lambda: _lib.check(L.snac_uct_returns_nstep(
            *ring, TD_STEPS, play.gamma, vp(play.reward), vp(play.done), vp(play.value), None, vp(play.z), st)))
        out["snac_uct_returns"] = timed(lambda: _lib.check(L.snac_uct_returns(*ring, play.gamma, vp(play.reward), vp(play.done), None, vp(play.z),
                                                                             st)))
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
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:
        what, B, cap, K, n, moves, keep = json.loads(args.worker)
        print(json.dumps(calls(B, cap, K, n, moves) if what == "calls" else whole(B, cap, K, n, moves, keep)))
        return
    n, moves = args.iterations, args.moves
    for B, cap, K in SHAPES:
        print("2D dynamic PUCT, B = %d trees x %d nodes, paths=%d, %d iterations per move, a ring of %d moves" % (B, cap, K, n, moves))
        print("  us per call (HIP events), windows of %d calls" % REPS)
        print("    %-34s" % "" + "".join("%9s" % ("group %d" % i) for i in range(GROUPS)) + "%10s%8s" % ("mean", "spread"))
        for label, t in child(["calls", B, cap, K, n, moves, True]).items():
            print("    %-34s" % label + "".join("%9.2f" % x for x in t) + "%10.2f%8.2f" % (float(np.mean(t)), max(t) - min(t)), flush=True)
        print("  wall ms per move of play(%d, %d)" % (moves, n))
        rows = [("keep_states=False", None, False), ("keep_states=True", None, True)]
        if args.reference_root:
            ref = ("reference play()", args.reference_root, None)
            rows = [ref] + rows + [("reference play() (again)",) + ref[1:]]
        got = {}
        for label, root, keep in rows:
            got[label] = child(["whole", B, cap, K, n, moves, keep], root)
            print("    %-34s%10.3f" % (label, got[label]), flush=True)
        print("    %-34s%+10.3f" % ("keep_states=True - False", got["keep_states=True"] - got["keep_states=False"]))
        if args.reference_root:
            base = 0.5 * (got["reference play()"] + got["reference play() (again)"])
            print("    %-34s%+10.3f   (the two reference rows differ by %.3f)"
                  % ("keep_states=True - reference", got["keep_states=True"] - base, abs(got["reference play()"] - got["reference play() (again)"])))
        print(flush=True)


if __name__ == "__main__":
    main()
