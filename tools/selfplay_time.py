"""A self-play move on the device (SelfPlay.play, snac_amd/selfplay.py) phase by phase, beside the same move driven from the host, timed
with HIP events on the env's stream.

  shapes      2D dynamic.  B = 64 trees x 8192 nodes, paths=16, and B = 4096 trees x 512 nodes, paths=1; 32 iterations per move; the
              rollout search (H = 100) and the PUCT search (a two-layer MLP).
  phases      device ms per move, summed over the timed moves and divided by them: run (the iterations), observe (the roots' rows into
              the ring slot), pick (snac_uct_pick_moves), advance (the root edges and the re-rooting), env reset (the finished trees'
              rows), restart (the scratch records, snac_uct_restart), priming (PUCT: the evaluator on the B roots and their priors).
              A third of the env rows start a few steps before the time limit, staggered, so that episodes end inside the timed moves.
  whole       wall ms per move of play(moves, iterations) between two synchronisations, and of the host-driven move below.
  host move   the same move with what a caller had before pick_moves / restart: run, best_actions(), advance(check=False), a host read of
              `done`, and for the finished trees index tensors of a data-dependent length (nonzero) -- the env rows reset by mask, the
              records loaded row by row (pool.load), the root statistics rows written with torch indexing.  It keeps the unfinished trees'
              subtrees, like restart(); reset() of every tree whenever one finishes would throw them away and is not the same search.
  ended       episodes that ended in the phase pass (its two warm-up moves included) / in the timed moves of the host-driven loop.
  --normalise adds a row with q_normalise=True under each row: its advance and restart phases include snac_uct_bounds.
  Each (shape, search) runs in a child process of its own under a time limit; the first one that fails ends the run.

    python tools/selfplay_time.py [--moves 24] [--iterations 32] [--normalise]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from snac_amd import BatchedDMPEnv, SelfPlay, UCTSearch, _lib  # noqa: E402

H = 100
SHAPES = ((64, 8192, 16), (4096, 512, 1))                            # B, cap, K
PHASES = ("run", "observe", "pick", "advance", "env reset", "restart", "priming")
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


def make(B, cap, K, n, puct, norm=False):
    env = BatchedDMPEnv(2, True, B, seed=1)
    env.reset()
    cs = env._hdr.view(torch.int16).view(B, 8)[:, 3]
    ends = torch.arange(B, device=env.device)
    cs[0::3] = (env.total_step - 2 - ends[0::3] % 16).to(torch.int16)     # a third of the episodes end within the first 18 moves
    kw = dict(paths=K) if K > 1 else {}
    if puct:
        kw["evaluator"] = mlp(env)
    if norm:
        kw["q_normalise"] = True
    search = UCTSearch(env, cap, 0 if puct else H, 0.99, max_iterations=(env.total_step + 1) * n, **kw)
    search.reset()
    return env, search


def phases(B, cap, K, n, puct, moves, norm=False):
    """Device ms per move and phase: play()'s own sequence, with an event between the phases."""
    env, s = make(B, cap, K, n, puct, norm)
    play = SelfPlay(s, moves + 2, sample_moves=4)
    play.play(2, n)                                                  # warm-up: every kernel and torch op of the timed window
    torch.cuda.synchronize()
    P = s.pool
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(PHASES) + 1)] for _ in range(moves)]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with torch.cuda.device(env.device):
        for i in range(moves):
            h, e = play.head, ev[i]
            e[0].record()
            s._run(n)
            e[1].record()
            _lib.check(play._observe(C.byref(env._desc), C.byref(env._state), vp(P.records), P.rows, B, vp(play._root_rows), vp(play.obs[h]), env._stream()))
            e[2].record()
            torch.ge(play._move, play.sample_moves, out=play._greedy.view(torch.bool))
            s._pick(play._greedy, play.moves, play.action[h], play.pi[h], play.value[h])
            e[3].record()
            s._advance_into(play.action[h], play.reward[h], play.done[h], prime=False)
            play.move[h].copy_(play._move)
            e[4].record()
            env.reset(mask=play.done[h], want_obs=False)
            e[5].record()
            ev_fn, s.evaluator = s.evaluator, None                   # restart() without its priming, which is timed on its own
            try:
                s.restart(play.done[h])
            finally:
                s.evaluator = ev_fn
            e[6].record()
            if puct:
                s._prime_roots()
            e[7].record()
            torch.add(play._move, 1, out=play._next)
            torch.where(play.done[h].view(torch.bool), play._zero, play._next, out=play._move)
            play.head, play.moves = (h + 1) % play.cap, play.moves + 1
    torch.cuda.synchronize()
    ms = [sum(ev[i][k].elapsed_time(ev[i][k + 1]) for i in range(moves)) / moves for k in range(len(PHASES))]
    return ms, int(play.done[:play.valid_moves()].sum())


def whole(B, cap, K, n, puct, moves, norm=False):
    """Wall ms per move of play(moves, n)."""
    env, s = make(B, cap, K, n, puct, norm)
    play = SelfPlay(s, moves + 2, sample_moves=4)
    play.play(2, n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    play.play(moves, n)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / moves, int(play.done[:play.valid_moves()].sum())


def host_move(env, s, fresh_row):
    """One move the way a caller of run / best_actions / advance alone makes it (the module docstring: "host move")."""
    B, cap = s.trees, s.nodes_per_tree
    a = s.best_actions()
    r, d = s.advance(a, check=False)
    if bool(d.any()):                                                # the host read
        idx = d.nonzero().reshape(-1)                                # a data-dependent length
        env.reset(mask=d, want_obs=False)
        s.pool.load(rows=idx, node_rows=idx * cap)
        s.pool.load(rows=idx, node_rows=B * cap + idx)
        s.stats[idx * cap] = fresh_row
        s._used[idx] = 1
        if s.q_normalise:
            s.q_bounds[idx] = s._no_bounds                           # a one-node tree: empty bounds
        if s.evaluator is not None:
            with torch.cuda.device(env.device):
                s._prime_roots()
    return r, d


def host(B, cap, K, n, puct, moves, norm=False):
    """Wall ms per move of the host-driven loop."""
    env, s = make(B, cap, K, n, puct, norm)
    fresh = torch.zeros(64, dtype=torch.int32, device=env.device)
    fresh[0:8] = -1
    fresh[32:34] = -1
    finished = 0
    for i in range(moves + 2):
        if i == 2:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        s._run(n)
        _, d = host_move(env, s, fresh)
        if i >= 2:
            finished += int(d.sum())
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / moves, finished


def worker(cfg):
    B, cap, K, n, puct, moves, norm = cfg
    ph, ended = phases(B, cap, K, n, puct, moves, norm)
    w, _ = whole(B, cap, K, n, puct, moves, norm)
    h, h_ended = host(B, cap, K, n, puct, moves, norm)
    print(json.dumps(dict(phases=ph, ended=ended, whole=w, host=h, host_ended=h_ended)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--moves", type=int, default=24)
    ap.add_argument("--iterations", type=int, default=32)
    ap.add_argument("--normalise", action="store_true", help="a q_normalise=True row under each row")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:
        worker(json.loads(args.worker))
        return
    n, moves = args.iterations, args.moves
    print("2D dynamic, %d iterations per move, %d timed moves; device ms per move by phase (HIP events), then wall ms per move" % (n, moves))
    print("  %-34s" % "" + "".join("%10s" % p for p in PHASES) + "  |%10s%10s%10s%9s" % ("additions", "play()", "host move", "ended"))
    for B, cap, K in SHAPES:
        for puct, norm in ((False, False), (False, True), (True, False), (True, True)):
            if norm and not args.normalise:
                continue
            cfg = [B, cap, K, n, puct, moves, norm]
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(cfg)], capture_output=True, text=True,
                                 timeout=LIMIT)
            if out.returncode != 0:                                  # nothing more is started on the device after a failure
                sys.stderr.write(out.stderr[-4000:])
                raise SystemExit("the worker for %r ended with status %d" % (cfg, out.returncode))
            m = json.loads(out.stdout.strip().splitlines()[-1])
            label = "  q_normalise=True" if norm else "B = %d x %d nodes, paths=%d, %s" % (B, cap, K, "PUCT" if puct else "rollout")
            print("  %-34s" % label + "".join("%10.3f" % x for x in m["phases"]) + "  |%10.3f%10.3f%10.3f%5d/%d"
                  % (sum(m["phases"][1:]), m["whole"], m["host"], m["ended"], m["host_ended"]), flush=True)


if __name__ == "__main__":
    main()
