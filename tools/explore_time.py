"""Self-play's exploration noise from the counter RNG (snac_explore_root_dirichlet / snac_explore_gumbel_scores in snac_amd/csrc/k_explore.hip,
snac_explore_pick_moves_temp in k_uct_play.hip; UCTSearch.add_dirichlet_noise / gumbel_scores(t=) / pick_moves(temperature=)): device time
over back-to-back calls, the median of five timed groups with min / max, the rows of a shape taking turns group by group.

  part 1      each entry point through the C ABI, each wrapper, and the torch composition it replaces on the same search --
              Dirichlet(alpha).sample() plus the mix plus set_root_priors(); two gumbel_scores() calls plus a where; multinomial of
              N ** (1 / T) -- at B = 64 and 4096 trees for A = 3, 5 and 8.
  part 2      a move of SelfPlay.play() (8 iterations) at B = 64 with paths=16 and at B = 4096 with paths=1, wall time per move: with the
              callback of examples/alphazero_selfplay.py (the default move) and with dirichlet=(0.3, 0.25) plus temperature=0.5.  With
              --parent DIR (a checkout of the parent commit with its library built) also the parent's move with the callback, twice,
              before and after this tree's rows: the spread of the two is what the default move is held against.
  --resources the VGPRs, LDS and scratch of the new kernels from the compiler's resource report (needs hipcc, no GPU).
Every row of part 2 is a child process under its own time limit; the first child that fails ends the run.

    python tools/explore_time.py [--resources | --no-gpu] [--parent DIR] [--out profiles/r30_explore.txt]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = 5
REPS = 200
LIMIT = 300                                                          # seconds per child process
MOVES = ((64, 16), (4096, 1))                                        # (trees, paths) of part 2
KINDS = {3: 1, 5: 2, 8: 3}
ALPHA, EPS, T = 0.3, 0.25, 0.5


def timed(calls, reps):
    """{label: [ms per call] * GROUPS}: per group every call in turn, `reps` back-to-back calls between two events."""
    import torch

    for call in calls.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    out = {k: [] for k in calls}
    for _ in range(GROUPS):
        for label, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                call()
            b.record()
            torch.cuda.synchronize()
            out[label].append(a.elapsed_time(b) / reps)
    return out


def _net(env, torch):
    A = env.num_actions
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Linear(env.obs_dim, 64), torch.nn.ReLU(), torch.nn.Linear(64, A + 1)).to(env.device)

    @torch.no_grad()
    def evaluator(obs):
        y = net(obs.to(torch.float32))
        return torch.softmax(y[:, :A], 1), y[:, A]

    return evaluator


def part1():
    import torch

    from snac_amd import BatchedDMPEnv, UCTSearch, _lib

    out = {}
    L = _lib.lib()
    for A, kind in KINDS.items():
        for B in (64, 4096):
            what = "B = %d, A = %d" % (B, A)
            env = BatchedDMPEnv(kind, True, B, seed=1)
            env.reset()
            s = UCTSearch(env, 16, 0, 0.99, c=1.25, paths=1, evaluator=_net(env, torch), max_iterations=16, q_normalise=True, gumbel=min(4, A))
            s.reset()
            s.run(8)
            dev, stream = env.device, env._stream()
            keep = s.root_priors().clone()
            conc = torch.full((A,), ALPHA, device=dev)
            dist = torch.distributions.Dirichlet(conc)
            mask = (torch.arange(B, device=dev) % 2 == 0).view(B, 1)
            m8 = mask.view(torch.uint8).reshape(-1).contiguous()
            scores = torch.empty((B, A), dtype=torch.float32, device=dev)
            act, pi, val = torch.empty(B, dtype=torch.int8, device=dev), torch.empty((B, A), device=dev), torch.empty(B, device=dev)
            head = s._pick_args
            vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
            bad, none = vp(s.noise_bad_rows), vp(s._sample_all)
            calls = {
                "snac_explore_root_dirichlet (C ABI)": lambda: _lib.check(L.snac_explore_root_dirichlet(*head, None, 3, ALPHA, EPS, 16, bad, stream)),
                "add_dirichlet_noise()": lambda: s.add_dirichlet_noise(ALPHA, EPS, t=3),
                "Dirichlet().sample(), the mix, set_root_priors()": lambda: s.set_root_priors((1 - EPS) * s.root_priors() + EPS * dist.sample((B,))),
                "snac_explore_gumbel_scores (C ABI)": lambda: _lib.check(L.snac_explore_gumbel_scores(*head, vp(m8), 3, vp(scores), stream)),
                "gumbel_scores(noise=mask, t=)": lambda: s.gumbel_scores(mask, t=3),
                "where(mask, gumbel_scores(True), gumbel_scores(False))": lambda: torch.where(mask, s.gumbel_scores(True), s.gumbel_scores(False)),
                "snac_explore_pick_moves_temp (C ABI)": lambda: _lib.check(L.snac_explore_pick_moves_temp(*head, none, 3, None, T, vp(act), vp(pi), vp(val),
                                                                                                          stream)),
                "pick_moves(greedy=False, temperature=)": lambda: s.pick_moves(greedy=False, t=3, temperature=T),
                "multinomial(root_visits() ** (1 / T))": lambda: torch.multinomial(s.root_visits().to(torch.float32) ** (1.0 / T), 1),
            }
            with torch.cuda.device(dev):
                rows = timed(calls, REPS)
            s.set_root_priors(keep)
            out.update({"%s, %s" % (k, what): v for k, v in rows.items()})
    return out


def move(B, K, mode):
    """[ms per move] * GROUPS of play(4, 8): wall time between two synchronisations, 3 calls a group."""
    import torch

    from snac_amd import BatchedDMPEnv, SelfPlay, UCTSearch

    env = BatchedDMPEnv(2, True, B, seed=1)
    env.reset()
    A = env.num_actions
    s = UCTSearch(env, 256 if K > 1 else 16, 0, 0.99, c=1.25, paths=K, evaluator=_net(env, torch), max_iterations=(env.total_step + 1) * 8)
    s.reset()
    if mode == "noise":
        play = SelfPlay(s, 16, sample_moves=8, dirichlet=(ALPHA, EPS), temperature=T)
    else:
        play = SelfPlay(s, 16, sample_moves=8, root_noise=lambda p: 0.75 * p + 0.25 / A)
    play.play(4, 8)
    torch.cuda.synchronize()
    out = []
    for _ in range(GROUPS):
        t0 = time.perf_counter()
        for _ in range(3):
            play.play(4, 8)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1000.0 / 12)
    return out


def child(args):
    sys.path.insert(0, args.package)
    print("RESULT " + json.dumps(move(args.trees, args.paths, args.mode)))


def part2(parent):
    rows = {}
    for B, K in MOVES:
        what = "B = %d, paths = %d" % (B, K)
        plan = [("the default move (the example's callback), this tree", ROOT, "callback"),
                ("dirichlet=(0.3, 0.25), temperature=0.5, this tree", ROOT, "noise")]
        if parent:
            plan = ([("the example's callback, the parent, run 1", parent, "callback")] + plan
                    + [("the example's callback, the parent, run 2", parent, "callback")])
        for label, package, mode in plan:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--package", package, "--trees", str(B), "--paths", str(K),
                                "--mode", mode], capture_output=True, text=True, timeout=LIMIT)
            if r.returncode != 0:
                raise SystemExit("%s, %s failed (%d):\n%s" % (label, what, r.returncode, r.stderr[-2000:]))
            rows["%s, %s" % (label, what)] = json.loads(re.search(r"^RESULT (.*)$", r.stdout, re.M).group(1))
    return rows


def resources():
    src = os.path.join(ROOT, "snac_amd", "csrc")
    lines = []
    for unit, names in (("k_explore.hip", ("k_root_dirichlet", "k_gumbel_scores")), ("k_uct_play.hip", ("k_uct_pick",))):
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-I",
                            os.path.join(ROOT, "include"), "-fno-strict-aliasing", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                            os.path.join(src, unit)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(r.stderr[-2000:])
        report = (r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)"
                  r".*?LDS Size \[bytes/block\]: (\d+)")
        for m in re.finditer(report, r.stderr, re.S):
            k = re.search(r"(k_[a-z_]+)ILi(\d)E(?:Lb(\d)E)?", m.group(1))
            if k and k.group(1) in names:
                name = "%s<%s%s>" % (k.group(1), k.group(2), "" if k.group(3) is None else ", temperature" if k.group(3) == "1" else ", plain")
                lines.append("    %-34s VGPRs %3s   scratch %s bytes/lane   LDS %s bytes/block   occupancy %s waves/SIMD"
                             % (name, m.group(2), m.group(3), m.group(5), m.group(4)))
    return lines


def stat(v):
    v = sorted(v)
    return "median %9.4f   min %9.4f   max %9.4f" % (v[len(v) // 2], v[0], v[-1])


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-gpu", action="store_true", help="the resource report alone")
    ap.add_argument("--parent", default=None, metavar="DIR")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--package", default=ROOT)
    ap.add_argument("--trees", type=int, default=64)
    ap.add_argument("--paths", type=int, default=16)
    ap.add_argument("--mode", default="callback")
    args = ap.parse_args()
    if args.child:
        return child(args)
    sys.path.insert(0, ROOT)
    if args.no_gpu:
        print("\n".join(["  the compiler's resource report"] + resources()))
        return
    text = ["ms per call on the device, %d groups of %d back-to-back calls, the rows of a shape taking turns group by group" % (GROUPS, REPS),
            "  part 1: the entry points, the wrappers and the torch compositions they replace"]
    rows = part1()
    for k, v in rows.items():
        text.append("    %-86s %s" % (k, stat(v)))
    slower = []
    for A in KINDS:
        for B in (64, 4096):
            what = "B = %d, A = %d" % (B, A)
            pairs = (("add_dirichlet_noise()", "Dirichlet().sample(), the mix, set_root_priors()"),
                     ("gumbel_scores(noise=mask, t=)", "where(mask, gumbel_scores(True), gumbel_scores(False))"),
                     ("pick_moves(greedy=False, temperature=)", "multinomial(root_visits() ** (1 / T))"))
            ratios = []
            for new, ref in pairs:
                r = med(rows["%s, %s" % (ref, what)]) / med(rows["%s, %s" % (new, what)])
                ratios.append("%s %.2f" % (new.split("(")[0], r))
                if r < 1.0:
                    slower.append("%s at %s" % (new, what))
            text.append("    %s: composition / wrapper: %s" % (what, "; ".join(ratios)))
    text.append("    wrappers whose median is above their composition's: %s" % ("; ".join(slower) or "none"))
    text.append("  part 2: a move of SelfPlay.play() with 8 iterations, wall ms per move (kind 2, 3 x play(4, 8) a group)")
    rows = part2(args.parent)
    for k, v in rows.items():
        text.append("    %-86s %s" % (k, stat(v)))
    if args.parent:
        for B, K in MOVES:
            what = "B = %d, paths = %d" % (B, K)
            p1, p2 = (rows["the example's callback, the parent, run %d, %s" % (i, what)] for i in (1, 2))
            d = rows["the default move (the example's callback), this tree, " + what]
            n = rows["dirichlet=(0.3, 0.25), temperature=0.5, this tree, " + what]
            lo, hi = min(p1 + p2), max(p1 + p2)
            text.append("    %s: the default move %.4f; the parent's two runs %.4f and %.4f (their groups %.4f .. %.4f): %s; with the noise %.4f"
                        % (what, med(d), med(p1), med(p2), lo, hi, "inside their spread" if lo <= med(d) <= hi else "OUTSIDE their spread", med(n)))
    if args.resources:
        text.append("  the compiler's resource report")
        text += resources()
    text = "\n".join(text) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
