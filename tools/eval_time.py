"""Default-policy evaluation of tree leaves (script/MCTS/utils/mcts.py:100-110) timed on the host, per call, two ways on the same leaves:

  pool.evaluate()           NodePool*.evaluate: one launch of k_eval on the node records (no fork, no reward / done arrays)
  store() + env.evaluate()  the records copied into a batch of m rows (pool.store), then BatchedDMPEnv.evaluate on them: a fork, a rollout
                            writing reward / done [H][m], the powers uploaded, snac_discounted_return

4096 and 65 536 leaves drawn at random from a 2^20-record pool (2D / 1D; 3D: 2^18) holding the rows of a 65 536-env batch; the two paths
alternate call by call, and their results are compared byte for byte.  SNAC_EVAL_E / SNAC_EVAL3D_E override the leaves per wave.

    python tools/eval_time.py [--kinds 2,3,1] [--reps 10]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from snac_amd import BatchedDMPEnv, NodePool  # noqa: E402

HORIZON = {2: 600, 3: 200, 1: 300}
POOL = {2: 1 << 20, 3: 1 << 18, 1: 1 << 20}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="2,3,1")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    print("SNAC_EVAL_E=%s SNAC_EVAL3D_E=%s" % (os.environ.get("SNAC_EVAL_E", "default"), os.environ.get("SNAC_EVAL3D_E", "default")), flush=True)
    for kind in [int(k) for k in args.kinds.split(",")]:
        H, n = HORIZON[kind], 1 << 16
        env = BatchedDMPEnv(kind, True, n, seed=1)
        env.reset()
        env.rollout(5, obs=None)
        pool = NodePool(env, POOL[kind])
        g = torch.Generator(device="cpu").manual_seed(kind)
        where = torch.randperm(POOL[kind], generator=g)[:n].to("cuda")
        pool.load(rows=torch.arange(n, device="cuda"), node_rows=where)
        for m in (4096, 65536):
            leaves = where[torch.randint(0, n, (m,), generator=g).to("cuda")]
            first = torch.rand(m, dtype=torch.float64, device="cuda")
            batch = BatchedDMPEnv(kind, True, m, plans=env.plans_full, seed=1)
            tmp_rows = torch.arange(m, device="cuda")

            def old():
                pool.store(node_rows=leaves, rows=tmp_rows, env=batch)
                return batch.evaluate(tmp_rows, H, 0.99, first)

            def new():
                return pool.evaluate(leaves, H, 0.99, first)

            a, b = old(), new()
            torch.cuda.synchronize()
            same = a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and torch.equal(a[1], b[1])
            times = {"store + evaluate": [], "pool.evaluate": []}
            for _ in range(args.reps):                               # alternating, one call timed at a time
                for name, fn in (("store + evaluate", old), ("pool.evaluate", new)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) * 1e3)
            steps = b[1].double().mean().item()
            for name, ts in times.items():
                ts = sorted(ts)
                print("%dD %6d leaves H=%d %-17s median %.3f ms  min %.3f ms per call  (mean steps %.1f, equal %s)"
                      % (kind, m, H, name, ts[len(ts) // 2], ts[0], steps, same), flush=True)
            del batch


if __name__ == "__main__":
    main()
