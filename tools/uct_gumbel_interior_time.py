"""The Gumbel interior search (UCTSearch(gumbel=m, gumbel_interior=True), snac_amd/uct.py) beside the Gumbel root search it extends, timed
with HIP events on the env's stream.  A sibling of tools/uct_gumbel_time.py at that tool's two shapes.

  shapes      2D dynamic, a constant evaluator (uniform priors, value 0: what the search machinery alone costs).  B = 4096 trees x 512
              nodes with paths=1, and B = 64 trees x 8192 nodes with paths=16; N iterations from reset() per timed group, steered by
              gumbel_begin() and the halving schedule with m = 4.
  part 1      the selection launch alone, snac_uct_select_gumbel against snac_uct_select_gumbel_interior ON THE SAME TREES: before every
              selection of a group the statistics and the tree sizes are saved; the driver's own entry point is launched untimed and the
              statistics are put back (so that both timed launches follow a launch and a copy over the same lines); the other entry
              point is launched between events, the statistics are put back, and the driver's own is launched between events; the
              search goes on from that one.
              Both drivers are timed: trees grown by the interior rule, and trees grown by PUCT below the root.  us per launch = the
              group's sum / N; five groups: median, min, max.  One more group, untimed, counts the levels each entry point walks
              (levels(): the mean over the paths, and the critical lane's, which is what a launch waits for); us/crit. = the median
              over the critical levels, the time of one level of each of a lane's `paths` paths.
  part 2      snac_uct_set_priors against snac_uct_set_priors_value on an iteration's B * paths rows, and snac_uct_improved_policy on the
              B roots against the float64 torch formula of the root search; five windows of 20 calls, us per call.

    python tools/uct_gumbel_interior_time.py [--iterations 64]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from snac_amd import BatchedDMPEnv, UCTSearch, _lib  # noqa: E402
from snac_amd.uct import gumbel_schedule  # noqa: E402

SHAPES = ((4096, 512, 1), (64, 8192, 16))                            # B, cap, K
GROUPS, M = 5, 4


def constant(A):
    def fn(obs):
        S = obs.shape[0]
        return torch.full((S, A), 1.0 / A, dtype=torch.float32, device=obs.device), torch.zeros(S, dtype=torch.float32, device=obs.device)
    return fn


def make(B, cap, K, n, interior):
    env = BatchedDMPEnv(2, True, B, seed=1)
    env.reset()
    return UCTSearch(env, cap, 0, 0.99, c=1.25, max_iterations=n, paths=K, evaluator=constant(env.num_actions), q_normalise=True, gumbel=M,
                     gumbel_interior=interior)


def launch(search, interior, offset):
    L, s = search._lib, search.env._stream()
    if interior:
        _lib.check(L.snac_uct_select_gumbel_interior(*search._select_args, offset, search.gumbel_c_visit, search.gumbel_c_scale, s))
    else:
        _lib.check(L.snac_uct_select_gumbel(*search._select_args, offset, s))


def levels(search):
    """(mean, critical) numbers of stored nodes on the paths of the launch just made.  A path's count is 1 + the depth of the node it
    stopped at or expanded from (a path that stopped on a row made by an earlier path of the launch: that row's parent, and one more).
    mean: over all paths.  critical: a lane walks its tree's K paths one after the other and a wave of 64 trees ends with its slowest
    lane, so per wave the largest sum over a tree's paths, divided by K, and the mean of that over the waves."""
    parent = search.stats[:, 32].long()
    src, first = search._src.long(), search._first_slot.long()
    on_fresh = (search._expanded == 0) & (first >= 0)
    x = torch.where(on_fresh, src[first.clamp(min=0)], src)
    d = on_fresh.long() + 1
    while True:
        p = parent[x]
        live = p >= 0
        if not bool(live.any()):
            per_tree = d.view(search.trees, search.paths).sum(1).double()
            waves = torch.nn.functional.pad(per_tree, (0, -search.trees % 64)).view(-1, 64).max(1).values
            return torch.tensor([float(d.double().mean()), float(waves.mean()) / search.paths])
        d += live
        x = torch.where(live, p, x)


def group(search, n, saved, count=False):
    """(us per launch of the other entry point, of the driver's own) over n steered iterations from reset(), on the same trees;
    count: (levels per path of the other, of the own) instead, untimed."""
    search.reset()
    g = torch.Generator(device=search.env.device)
    g.manual_seed(1)
    search.gumbel_begin(search.gumbel_scores(generator=g))
    plan = gumbel_schedule(n, min(search.gumbel, search.num_actions))
    own = search.gumbel_interior
    stats, used = saved
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(n)]
    walked = [torch.zeros(2), torch.zeros(2)]
    with torch.cuda.device(search.env.device):
        for (halve, i), (a, b, c, d) in zip(plan, ev):
            if halve:
                search._candidates(1)
            stats.copy_(search.stats)
            used.copy_(search._used)
            launch(search, own, i * search.paths)                    # untimed: both timed launches follow a launch over the same lines
            search.stats.copy_(stats)
            search._used.copy_(used)
            a.record()
            launch(search, not own, i * search.paths)
            b.record()
            if count:
                walked[0] += levels(search) / n
            search.stats.copy_(stats)
            search._used.copy_(used)
            c.record()
            launch(search, own, i * search.paths)
            d.record()
            if count:
                walked[1] += levels(search) / n
            search._edges()
            search._evaluate()
            search._backup()
            search._set_priors()
    torch.cuda.synchronize()
    if count:
        return tuple(walked)
    return (1e3 * sum(a.elapsed_time(b) for a, b, _, _ in ev) / n, 1e3 * sum(c.elapsed_time(d) for _, _, c, d in ev) / n)


def row(label, t, walked=None):
    tail = "" if walked is None else "%10.2f%10.2f%10.2f" % (float(walked[0]), float(walked[1]), float(np.median(t)) / float(walked[1]))
    print("    %-70s" % label + "%10.2f%10.2f%10.2f" % (float(np.median(t)), min(t), max(t)) + tail, flush=True)


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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    n = args.iterations
    for B, cap, K in SHAPES:
        print("B = %d trees x %d nodes, paths=%d, m = %d, %d iterations per group; us per selection launch (HIP events), %d groups"
              % (B, cap, K, M, n, GROUPS))
        print("    %-70s" % "" + "%10s%10s%10s%10s%10s%10s" % ("median", "min", "max", "levels", "critical", "us/crit."))
        searches = {}
        for interior in (True, False):
            search = searches[interior] = make(B, cap, K, n, interior)
            saved = (torch.empty_like(search.stats), torch.empty_like(search._used))
            group(search, min(n, 8), saved)                          # warm-up: every kernel and torch op of the timed window
            t = [group(search, n, saved) for _ in range(GROUPS)]
            other, own = [x for x, _ in t], [y for _, y in t]
            w_other, w_own = group(search, n, saved, count=True)
            grown = "trees grown by the interior rule" if interior else "trees grown by PUCT below the root"
            row("snac_uct_select_gumbel, %s" % grown, *((other, w_other) if interior else (own, w_own)))
            row("snac_uct_select_gumbel_interior, %s" % grown, *((own, w_own) if interior else (other, w_other)))
            del saved
        print("  on the trees the interior search left; us per call, windows of 20 calls")
        search, plain = searches[True], searches[False]
        with torch.cuda.device(search.env.device):
            s = search.env._stream()
            row("snac_uct_set_priors, %d rows" % (B * K), timed(lambda: _lib.check(search._lib.snac_uct_set_priors(*search._prior_args, s))))
            value = C.c_void_p(search._value.data_ptr())
            row("snac_uct_set_priors_value, %d rows" % (B * K),
                timed(lambda: _lib.check(search._lib.snac_uct_set_priors_value(*search._prior_args[:-1], value, 0, s))))
            row("snac_uct_improved_policy, %d roots" % B, timed(search.improved_policy))
            plain.stats.copy_(search.stats)
            plain.q_bounds.copy_(search.q_bounds)
            row("improved_policy() of the root search (float64 torch ops)", timed(plain.improved_policy))
        print(flush=True)
        del searches, search, plain
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
