"""The PUCT search (UCTSearch(evaluator=fn), snac_amd/uct.py) beside the rollout search, timed with HIP events on the env's stream.

  shapes      2D dynamic.  B = 64 trees x 8192 nodes with 4096 leaf evaluations per tree as 4096 x paths=1, 256 x 16 and 64 x 64;
              B = 4096 trees x 512 nodes, 512 x paths=1.
  rows        the rollout search (H = 100) of --reference-root DIR (another checkout of this repository, built: the parent commit) in
              a child process of the same session, before and after; this build's rollout search; the PUCT search with a constant
              evaluator (uniform priors, value 0: what the search machinery alone costs) and with a two-layer MLP.
  columns     R repeats of reset() + run(n) between two events, their mean and spread; then one pass with events between the phases
              (device ms summed over the iterations): select, transition, observe, evaluator (the first-reward ops, the function and
              the estimate; the rollout rows: the rollout), backup + priors; mean tree size, mean depth of the allocated nodes, and
              levels = the summed depth of the iterations' leaves, wave levels = the same with each wave of 64 trees counted as its
              deepest lane, select us per wave level = select ms / wave levels (a pass of its own).
              --normalise adds a row with q_normalise=True (k_uct_select_paths / k_uct_select_puct / k_uct_backup_paths in their NORM
              forms) under each of this build's rows.
  part 2      snac_observe_nodes2d beside snac_transition_nodes2d at m = 524 288 random records of a 2^20-record pool (the shape of
              bench.py's transition_2d_nodes_524288_edges): ms and bytes per second by lines read + lines / rows written.
  part 3      snac_uct_bounds alone on full trees (every row visited) at B = 64 x 8192 nodes and B = 4096 x 512 nodes: ms per call and
              bytes read per second (32 bytes per row: pieces P_HDR and P_OWN), with the lanes per tree the library picks from cap and
              with each forced width (SNAC_UCT_BOUNDS_WIDTH), every width in a child process of its own.

    python tools/uct_puct_time.py [--repeat 5] [--reference-root DIR] [--parts 1,2] [--normalise]
"""
import argparse
import ctypes as C
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

from snac_amd import BatchedDMPEnv, UCTSearch, _lib  # noqa: E402

H = 100
SHAPES = ((64, 8192, 1, 4096), (64, 8192, 16, 256), (64, 8192, 64, 64), (4096, 512, 1, 512))     # B, cap, K, iterations


def constant(A):
    def fn(obs):
        S = obs.shape[0]
        return torch.full((S, A), 1.0 / A, dtype=torch.float32, device=obs.device), torch.zeros(S, dtype=torch.float32, device=obs.device)
    return fn


def mlp(env, hidden=128):
    A = env.num_actions
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Linear(env.obs_dim, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, A + 1)).to(env.device)

    @torch.no_grad()
    def fn(obs):
        y = net(obs.to(torch.float32))
        return torch.softmax(y[:, :A], 1), torch.tanh(y[:, A])
    return fn


def make(B, cap, K, n, mode, norm=False):
    env = BatchedDMPEnv(2, True, B, seed=1)
    env.reset()
    kw = {} if K == 1 else dict(paths=K)
    if norm:
        kw["q_normalise"] = True
    if mode != "rollout":
        kw["evaluator"] = constant(env.num_actions) if mode == "const" else mlp(env)
    return UCTSearch(env, cap, H, 0.99, max_iterations=n, **kw)


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


def phase_fns(search):
    if getattr(search, "evaluator", None) is None:
        return (search._select, search._edges, lambda: None, search._evaluate, search._backup)

    def value():
        search._first_reward()
        search._value_leaves()

    def backup():
        search._backup()
        search._set_priors()
    return (search._select, search._edges, search._observe_leaves, value, backup)


def phases(search, n):
    """Device ms per phase summed over n iterations (events between the phases)."""
    search.reset()
    torch.cuda.synchronize()
    fns = phase_fns(search)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(n)]
    with torch.cuda.device(search.env.device):
        for i in range(n):
            ev[i][0].record()
            for k, f in enumerate(fns):
                f()
                ev[i][k + 1].record()
    torch.cuda.synchronize()
    return [sum(ev[i][k].elapsed_time(ev[i][k + 1]) for i in range(n)) for k in range(5)]


def levels(search, n):
    """(levels, wave levels): the summed depth of the n iterations' leaves (a leaf at depth d cost d + 1 dependent trips, the root's
    included), and the same with every wave of 64 trees counted as its deepest lane -- what a lane = tree kernel waits for."""
    search.reset()
    dev = search.env.device
    depth = torch.zeros(search.rows, dtype=torch.int64, device=dev)
    total = torch.zeros((), dtype=torch.int64, device=dev)
    waves = torch.zeros((), dtype=torch.int64, device=dev)
    B, K = search.trees, search.paths
    pad = (-B) % 64
    fns = phase_fns(search)
    with torch.cuda.device(dev):
        for _ in range(n):
            fns[0]()
            src, leaf, exp = search._src.long(), search._leaf.long(), search._expanded.bool()
            depth[leaf[exp]] = depth[src[exp]] + 1
            trips = (depth[leaf] + 1).view(B, K).sum(1)                # a lane walks its tree's K paths one after the other
            total += trips.sum()
            waves += torch.nn.functional.pad(trips, (0, pad)).view(-1, 64).max(1).values.sum()   # a wave takes as long as its deepest lane
            for f in fns[1:]:
                f()
    torch.cuda.synchronize()
    return int(total), int(waves)


def shape(search):
    par, used = search.parent.cpu().numpy(), search.tree_sizes().cpu().numpy()
    cap = search.nodes_per_tree
    d = np.zeros(par.size, dtype=np.int64)
    rows = [b * cap + j for b in range(search.trees) for j in range(int(used[b]))]
    for x in rows:
        p = int(par[x])
        d[x] = d[p] + 1 if p >= 0 else 0
    return float(used.mean()), float(d[rows].mean())


def measure(B, cap, K, n, mode, R, norm=False):
    search = make(B, cap, K, n, mode, norm)
    search.reset()
    search.run(min(n, 8))                                            # warm-up: every kernel and torch op of the timed window
    torch.cuda.synchronize()
    t = totals(search, n, R)
    size, depth = shape(search)
    return dict(totals=t, phases=phases(search, n), levels=levels(search, n), size=size, depth=depth)


def row(label, m):
    t, p = m["totals"], m["phases"]
    print("    %-26s" % label + "".join("%9.1f" % x for x in t) + "%10.1f%8.1f" % (float(np.mean(t)), max(t) - min(t)) + "  |"
          + "".join("%9.1f" % x for x in p) + "  |%8.0f%7.2f%12d%12d%11.3f" % (m["size"], m["depth"], m["levels"][0], m["levels"][1], 1e3 * p[0] / m["levels"][1]), flush=True)


def reference(root, cfg, R):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--worker", json.dumps(cfg), "--repeat", str(R)], check=True,
                         capture_output=True, text=True, timeout=900).stdout
    return json.loads(out.strip().splitlines()[-1])


def part1(R, ref_root, norm=False):
    print("part 1: 2D dynamic; the rollout rows with H = %d; device ms (HIP events); us/wavelvl = 1000 x select ms / wave levels" % H)
    for B, cap, K, n in SHAPES:
        print("  B = %d trees x %d nodes, %d iterations x paths=%d" % (B, cap, n, K))
        print("    %-26s" % "" + "".join("%9s" % ("run %d" % i) for i in range(R)) + "%10s%8s" % ("mean", "spread") + "  |"
              + "".join("%9s" % s for s in ("select", "transit", "observe", "evaluat", "backup+p")) + "  |%8s%7s%12s%12s%11s" % ("nodes", "depth", "levels", "wave levels", "us/wavelvl"))
        cfg = [B, cap, K, n]
        if ref_root:
            row("reference rollout", reference(ref_root, cfg, R))
        for label, mode in (("this build, rollout", "rollout"), ("PUCT, constant evaluator", "const"), ("PUCT, two-layer MLP", "mlp")):
            row(label, measure(B, cap, K, n, mode, R))
            if norm:
                row("  q_normalise=True", measure(B, cap, K, n, mode, R, norm=True))
        if ref_root:
            row("reference rollout (again)", reference(ref_root, cfg, R))


def timed(call, reps):
    call()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out


def part2():
    from snac_amd import NodePool2D

    pool, m = 1 << 20, 524288
    e = BatchedDMPEnv(2, True, pool, seed=1)
    e.reset()
    e.rollout(20, obs=None)
    dev = e.device
    src = torch.randint(0, pool - m, (m,), device=dev, dtype=torch.int32)
    dst = (pool - m + torch.arange(m, device=dev, dtype=torch.int32)).contiguous()
    acts = torch.randint(0, e.num_actions, (m,), device=dev).to(torch.int8)
    ob = torch.empty((m, e.obs_dim), dtype=torch.float64, device=dev)
    rw, dn = torch.empty(m, dtype=torch.float32, device=dev), torch.empty(m, dtype=torch.uint8, device=dev)
    recs = NodePool2D(e, pool)
    recs.load()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def edges():
        _lib.check(e._lib.snac_transition_nodes2d(C.byref(e._desc), C.byref(e._state), vp(recs.records), pool, m, vp(src), vp(dst), 0, vp(acts), None,
                                                  vp(ob), vp(rw), vp(dn), e._stream()))

    def observe():
        _lib.check(e._lib.snac_observe_nodes2d(C.byref(e._desc), C.byref(e._state), vp(recs.records), pool, m, vp(src), vp(ob), e._stream()))

    print("\npart 2: m = %d random records of a 2^20-record 2D pool, float64 rows; five windows of 20 calls, ms per call" % m)
    for name, call, nbytes in (("snac_transition_nodes2d", edges, 128 + 128 + 51 * 8 + 4 + 4 + 1 + 4 + 1), ("snac_observe_nodes2d", observe, 128 + 51 * 8 + 4)):
        t = timed(call, 20)
        best = min(t)
        print("  %-26s" % name + "".join("%9.4f" % x for x in t) + "   best %.4f ms, %d bytes per record (lines read + lines / rows written): %.0f GB/s"
              % (best, nbytes, nbytes * m / (best * 1e-3) / 1e9), flush=True)


BOUNDS_SHAPES = ((64, 8192), (4096, 512))


def bounds_worker():
    """ms per snac_uct_bounds call on full trees at BOUNDS_SHAPES, one JSON line."""
    out = []
    for B, cap in BOUNDS_SHAPES:
        env = BatchedDMPEnv(2, True, B, seed=1)
        env.reset()
        s = UCTSearch(env, cap, 0, 0.99, max_iterations=4, q_normalise=True)
        s.reset()
        g = torch.Generator(device=env.device).manual_seed(1)
        s.stats[:, 35] = torch.randint(1, 6, (s.rows,), generator=g, device=env.device, dtype=torch.int32)
        s.value_sum.copy_(300.0 * torch.randn(s.rows, generator=g, device=env.device, dtype=torch.float64))
        s._used.fill_(cap)
        with torch.cuda.device(env.device):
            out.append(timed(lambda: s._rebound(None), 20))
        lo_hi = s.q_bounds_of_trees()
        means = (s.value_sum / s.visits.double())[:B * cap].view(B, cap)[:, 1:]
        assert torch.equal(lo_hi[:, 0], means.min(1).values) and torch.equal(lo_hi[:, 1], means.max(1).values)
    print(json.dumps(out))


def part3():
    print("\npart 3: snac_uct_bounds on full trees; five windows of 20 calls, ms per call; bytes = 32 per row below the root")
    for width in ("", "8", "16", "32", "64"):
        env = dict(os.environ)
        env.pop("SNAC_UCT_BOUNDS_WIDTH", None)
        if width:
            env["SNAC_UCT_BOUNDS_WIDTH"] = width
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--bounds-worker"], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:                                        # nothing more is started on the device after a failure
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("the bounds worker (width %s) ended with status %d" % (width or "from cap", r.returncode))
        for (B, cap), t in zip(BOUNDS_SHAPES, json.loads(r.stdout.strip().splitlines()[-1])):
            best = min(t)
            print("  %-22s B = %4d x %4d nodes" % ("lanes per tree: " + (width or "from cap"), B, cap) + "".join("%9.4f" % x for x in t)
                  + "   best %.4f ms: %.0f GB/s" % (best, 32 * B * (cap - 1) / (best * 1e-3) / 1e9), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--reference-root", default=None)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--normalise", action="store_true", help="part 1: a q_normalise=True row under each of this build's rows")
    ap.add_argument("--bounds-worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:                                                  # the reference build's rollout search at one shape, one JSON line
        B, cap, K, n = json.loads(args.worker)
        print(json.dumps(measure(B, cap, K, n, "rollout", args.repeat)))
        return
    if args.bounds_worker:
        bounds_worker()
        return
    parts = [int(p) for p in args.parts.split(",")]
    if 1 in parts:
        part1(args.repeat, args.reference_root, args.normalise)
    if 2 in parts:
        part2()
    if 3 in parts:
        part3()


if __name__ == "__main__":
    main()
