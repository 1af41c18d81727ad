"""Re-rooting after a move (snac_amd/uct.py: UCTSearch.advance) timed with HIP events on the env's stream.

  part 1  B = 4096 trees of 512 nodes after 64 and after 512 iterations, 2D H = 600, 3D H = 200, 1D H = 300 (the shapes of
          profiles/r10_uct.txt): the root edges (the B transitions into the scratch records), the re-rooting kernel (k_uct_advance) and
          the whole advance(), each the mean over R calls on the same tree (statistics, records and sizes restored between calls,
          outside the timed windows); the bytes the kernel moves (kept nodes x 2 x (256 + record bytes)) and their share of the 8 TB/s
          HBM peak; one iteration's device time for scale.
  part 2  the wide-and-few shape, 64 trees of 8192 nodes (2D, H = 100), where one workgroup per tree is at its weakest.
  part 3  one played 2D episode per env (B = 256, 50 iterations per move, H = 100), with the subtree kept (advance) and with a fresh
          tree every move (store_roots + reset): mean episodic reward and mean final IoU.  Reported, not gated.

    python tools/uct_advance_time.py [--parts 1,2,3] [--repeat 8]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from snac_amd import BatchedDMPEnv, UCTSearch  # noqa: E402

PEAK = 8.0e12                                                        # HBM bytes / s


def _ev():
    return torch.cuda.Event(enable_timing=True)


def time_advance(search, R):
    """(edges ms, kernel ms, advance ms, kept nodes moved, trees that kept a subtree) as means over R calls on the same tree."""
    a = search.best_actions()
    snap = (search.stats.clone(), search.pool.records.clone(), search._used.clone())
    B = search.trees
    reward = torch.empty(B, dtype=torch.float32, device=search.env.device)
    done = torch.empty(B, dtype=torch.uint8, device=search.env.device)
    tried = search.stats[search._roots].gather(1, a.view(-1, 1)).view(-1) >= 0

    def restore():
        search.stats.copy_(snap[0])
        search.pool.records.copy_(snap[1])
        search._used.copy_(snap[2])

    e_sum = k_sum = w_sum = 0.0
    kept = 0
    with torch.cuda.device(search.env.device):
        search.advance(a, check=False)                              # warm-up
        for _ in range(R):
            restore()
            e0, e1, e2 = _ev(), _ev(), _ev()
            search._adv_action.copy_(a)
            e0.record()
            search._root_edges()
            e1.record()
            search._reroot(reward, done)
            e2.record()
            torch.cuda.synchronize()
            e_sum += e0.elapsed_time(e1)
            k_sum += e1.elapsed_time(e2)
            kept = int(search._used[tried].sum())
            restore()
            w0, w1 = _ev(), _ev()
            w0.record()
            search.advance(a, check=False)
            w1.record()
            torch.cuda.synchronize()
            w_sum += w0.elapsed_time(w1)
    restore()
    return e_sum / R, k_sum / R, w_sum / R, kept, int(tried.sum())


def iteration_ms(search, n=4):
    a, b = _ev(), _ev()
    a.record()
    search.run(n)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def report(tag, search, R):
    edges, kernel, whole, kept, trees = time_advance(search, R)
    rb = search.pool.WORDS * 4
    moved = kept * 2 * (256 + rb)
    print("  %-24s %8.4f %8.4f %8.4f %10d %6d %12.1f %8.3f" % (tag, edges, kernel, whole, kept, trees, moved / 1e6, moved / (kernel * 1e-3) / PEAK))


def header():
    print("  %-24s %8s %8s %8s %10s %6s %12s %8s" % ("", "edges", "kernel", "advance", "kept", "trees", "MB moved", "of peak"))


def part1(R):
    H = {2: 600, 3: 200, 1: 300}
    B, cap = 4096, 512
    print("part 1: B = %d trees x %d nodes; device ms, mean of %d calls on the same tree; kept = nodes moved by the kernel, trees = trees "
          "that kept a subtree" % (B, cap, R))
    for kind in (2, 3, 1):
        env = BatchedDMPEnv(kind, True, B, seed=1)
        env.reset()
        search = UCTSearch(env, cap, H[kind], 0.99, max_iterations=520)
        search.reset()
        print("\n %dD dynamic, H = %d, record %d bytes" % (kind, H[kind], search.pool.WORDS * 4))
        header()
        for mark in (64, 512):
            search.run(mark - search.iterations)
            torch.cuda.synchronize()
            report("after %d iterations" % mark, search, R)
        print("  one iteration (run(4) / 4) after 512: %.4f ms" % iteration_ms(search))
        del search, env
        torch.cuda.empty_cache()


def part2(R):
    B, cap, its = 64, 8192, 8000
    env = BatchedDMPEnv(2, True, B, seed=1)
    env.reset()
    search = UCTSearch(env, cap, 100, 0.99, max_iterations=its + 8)
    search.reset()
    search.run(its)
    torch.cuda.synchronize()
    print("\npart 2: B = %d trees x %d nodes, 2D dynamic H = 100, after %d iterations (tree sizes %d-%d)"
          % (B, cap, its, int(search._used.min()), int(search._used.max())))
    header()
    report("wide and few", search, R)
    del search, env
    torch.cuda.empty_cache()


def play(reuse, B=256, per=50, H=100):
    env = BatchedDMPEnv(2, True, B, seed=7)
    env.reset()
    moves = env.sizes.total_step
    search = UCTSearch(env, 512, H, 0.99, max_iterations=per * moves + per)
    search.reset()
    total = torch.zeros(B, dtype=torch.float64, device=env.device)
    alive = torch.ones(B, dtype=torch.bool, device=env.device)
    played = 0
    t0 = time.time()
    for _ in range(moves):
        if not reuse:
            search.store_roots()
            search.reset()
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
    return float(total.mean()), float(iou.mean()), played, int(alive.sum()), time.time() - t0


def part3():
    print("\npart 3: one 2D dynamic episode per env, B = 256, 50 iterations per move, 512 nodes per tree, H = 100")
    print("  %-22s %14s %14s %8s %10s %8s" % ("", "mean reward", "mean IoU", "moves", "not done", "wall s"))
    for reuse in (True, False):
        r, iou, n, left, wall = play(reuse)
        print("  %-22s %14.4f %14.4f %8d %10d %8.1f" % ("subtree kept" if reuse else "fresh tree every move", r, iou, n, left, wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--repeat", type=int, default=8)
    args = ap.parse_args()
    parts = [int(p) for p in args.parts.split(",")]
    if 1 in parts:
        part1(args.repeat)
    if 2 in parts:
        part2(args.repeat)
    if 3 in parts:
        part3()


if __name__ == "__main__":
    main()
