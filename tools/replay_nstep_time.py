"""n-step transitions and episode windows from the replay ring (snac_amd/replay.py: gather_nstep / sample(n_step=) / gather_windows /
sample_windows; snac_amd/csrc/k_replay.hip): device time over back-to-back launches, the median of five timed groups with min / max.

  shape       2D dynamic, 65 536 envs, a float64 ring of 64 ticks (collected once, full), 65 536 samples: the shape of bench.py's
              replay_gather_65536.  New random samples every launch, drawn before the timed window.
  part 1      the C ABI alone: snac_replay_gather_nstep at n = 1, 3, 5 beside snac_replay_gather at the same batch, and their ratio.
  part 2      ReplayRing.sample(batch, n_step=3, gamma) beside what a caller had before: three gather() calls put together with torch
              (compose() below; tests/test_gpu_replay_nstep.py pins the new call against the same composition).
  part 3      gather_windows(L = 8, 32) for 4096 windows beside gather() of the same B * L flattened (slot, env) pairs -- what
              sample_sequences() launches -- and the rows read per window from the arithmetic: L + 1 against 2 L.
  part 4      ReplayRing.sample(batch) on the default path, each row a child process of its own: --reference-root DIR (another checkout
              of this repository, built: the parent commit), this build, and the reference again -- the spread of the two reference rows
              is the noise the difference has to be read against.
Every part is a child process under its own time limit; the first child that fails ends the run.

    python tools/replay_nstep_time.py [--reference-root DIR]
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

from snac_amd import BatchedDMPEnv, ReplayRing, _lib  # noqa: E402

ENVS, CAP, BATCH, WINDOWS = 65536, 64, 65536, 4096
GROUPS, REPS, SETS = 5, 20, 8
GAMMA = 0.95
LIMIT = 300                                                          # seconds per child process


def make():
    env = BatchedDMPEnv(2, True, ENVS, seed=1)
    env.reset()
    ring = ReplayRing(env, CAP)
    ring.collect(CAP)
    return env, ring


def draws(ring, batch, dtype=torch.int64):
    """SETS index sets over the addressable transitions, handed out in turn."""
    dev, v = ring.env.device, ring.valid_ticks()
    sets = [(((ring.head - 1 - torch.randint(0, v, (batch,), device=dev)) % ring.cap).to(dtype), torch.randint(0, ENVS, (batch,), device=dev).to(dtype))
            for _ in range(SETS)]
    state = [0]

    def nxt():
        state[0] += 1
        return sets[state[0] % SETS]
    return nxt


def timed(call):
    """ms per call: GROUPS windows of REPS back-to-back calls between two events."""
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
        out.append(a.elapsed_time(b) / REPS)
    return out


def compose(ring, slot, env, n, gamma):
    """The n-step transition from n gather() calls and torch: what a caller had before gather_nstep()."""
    cap, N = ring.cap, ring.env.num_envs
    newest = (ring.head - 1) % cap
    steps = [ring.gather((slot + k) % cap, env, with_plan=k == 0) for k in range(n)]
    first = ring.first.view(-1)
    m, alive = torch.zeros_like(slot), torch.ones_like(slot, dtype=torch.bool)
    for k in range(n):
        sk = (slot + k) % cap
        stop = steps[k]["done"] | (sk == newest) | (first[((sk + 1) % cap) * N + env] != 0) if k + 1 < n else torch.ones_like(alive)
        m = torch.where(alive & stop, k + 1, m)
        alive = alive & ~stop
    g, d = torch.zeros(slot.shape, dtype=torch.float64, device=slot.device), torch.ones(slot.shape, dtype=torch.float64, device=slot.device)
    for k in range(n - 1, -1, -1):
        g = torch.where(k < m, steps[k]["reward"].double() + gamma * g, g)
        d = torch.where(k < m, d * gamma, d)
    at = torch.arange(slot.numel(), device=slot.device)
    done = torch.stack([s["done"] for s in steps])[m - 1, at]
    out = dict(s=steps[0]["s"], action=steps[0]["action"], plan=steps[0]["plan"], s_next=torch.stack([s["s_next"] for s in steps])[m - 1, at], done=done,
               steps=m.to(torch.int32), discount=torch.where(done, 0.0, d).float())
    out["return"] = g.float()
    return out


def part1():
    env, ring = make()
    L, st, dev = env._lib, env._stream(), env.device
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    idx = draws(ring, BATCH, torch.int32)
    s, sn = torch.empty((BATCH, 51), device=dev), torch.empty((BATCH, 51), device=dev)
    pl = torch.empty((BATCH, 400), device=dev)
    act, ret, disc = torch.empty(BATCH, dtype=torch.int64, device=dev), torch.empty(BATCH, device=dev), torch.empty(BATCH, device=dev)
    dn, stp = torch.empty(BATCH, dtype=torch.bool, device=dev), torch.empty(BATCH, dtype=torch.int32, device=dev)
    head = (C.byref(env._desc), C.byref(env._state), CAP)
    rings = (vp(ring.obs), vp(ring.first), vp(ring.done), vp(ring.reward), vp(ring.action), vp(ring.plan_idx))
    out = {}

    def gather():
        slot, e = idx()
        _lib.check(L.snac_replay_gather(*head, vp(ring.obs), vp(ring.first), vp(ring.plan_idx), vp(slot), vp(e), BATCH, vp(s), vp(sn), vp(pl), st))

    def nstep(n):
        slot, e = idx()
        _lib.check(L.snac_replay_gather_nstep(*head, 0, *rings, (ring.head - 1) % CAP, vp(slot), vp(e), BATCH, n, GAMMA, vp(s), vp(sn), vp(pl),
                                              vp(act), vp(ret), vp(disc), vp(dn), vp(stp), st))
    with torch.cuda.device(dev):
        out["snac_replay_gather"] = timed(gather)
        for n in (1, 3, 5):
            out["snac_replay_gather_nstep, n = %d" % n] = timed(lambda: nstep(n))
        out["snac_replay_gather (again)"] = timed(gather)
    return out


def part2():
    env, ring = make()
    nxt = draws(ring, BATCH)
    out = {}
    with torch.cuda.device(env.device):
        out["sample(n_step=3)"] = timed(lambda: ring.sample(BATCH, n_step=3, gamma=GAMMA))
        out["gather_nstep(n=3) of given pairs"] = timed(lambda: ring.gather_nstep(*nxt(), 3, GAMMA))
        out["3 x gather() + torch, given pairs"] = timed(lambda: compose(ring, *nxt(), 3, GAMMA))
    return out


def part3():
    env, ring = make()
    nxt = draws(ring, WINDOWS)
    out = {}
    with torch.cuda.device(env.device):
        for L in (8, 32):
            steps = torch.arange(L, device=env.device)

            def flat():
                slot, e = nxt()
                return ring.gather(((slot[:, None] - (L - 1) + steps[None, :]) % CAP).reshape(-1), e[:, None].expand(WINDOWS, L).reshape(-1), with_plan=False)
            out["gather_windows(L = %d)" % L] = timed(lambda: ring.gather_windows(*nxt(), L, with_plan=False))
            out["gather() of %d x %d pairs" % (WINDOWS, L)] = timed(flat)
    return out


def part4():
    env, ring = make()
    with torch.cuda.device(env.device):
        return {"sample(%d)" % BATCH: timed(lambda: ring.sample(BATCH))}


PARTS = dict(part1=part1, part2=part2, part3=part3, part4=part4)


def child(part, root=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + (["--root", root] if root else []) + ["--worker", part]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    if out.returncode != 0:                                          # nothing more is started on the device after a failure
        sys.stderr.write(out.stderr[-4000:])
        raise SystemExit("the worker for %s ended with status %d" % (part, out.returncode))
    return json.loads(out.stdout.strip().splitlines()[-1])


def show(rows):
    for label, t in rows.items():
        print("    %-40s median %8.4f   min %8.4f   max %8.4f" % (label, float(np.median(t)), min(t), max(t)), flush=True)
    return {k: float(np.median(t)) for k, t in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-root", default=None)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:
        print(json.dumps(PARTS[args.worker]()))
        return
    print("2D dynamic, %d envs, a float64 ring of %d ticks; ms per call on the device, %d groups of %d back-to-back calls" % (ENVS, CAP, GROUPS, REPS))
    print("  part 1: the C ABI alone, %d samples" % BATCH)
    rows = child("part1")
    med = show(rows)
    base = 0.5 * (med["snac_replay_gather"] + med["snac_replay_gather (again)"])
    both = rows["snac_replay_gather"] + rows["snac_replay_gather (again)"]
    for n in (1, 3, 5):
        print("    n = %d / snac_replay_gather: %.3f" % (n, med["snac_replay_gather_nstep, n = %d" % n] / base))
    print("    (snac_replay_gather's own groups span %.4f .. %.4f: +- %.1f %% of their mean)" % (min(both), max(both), 50 * (max(both) - min(both)) / base))
    print("  part 2: the python calls, %d samples" % BATCH)
    med = show(child("part2"))
    print("    3 x gather() + torch / gather_nstep(n=3): %.2f" % (med["3 x gather() + torch, given pairs"] / med["gather_nstep(n=3) of given pairs"]))
    print("  part 3: %d windows" % WINDOWS)
    med = show(child("part3"))
    for L in (8, 32):
        print("    L = %2d: flattened gather / gather_windows %.2f; rows read per window: %d against %d (%d against %d bytes of float64 rows)"
              % (L, med["gather() of %d x %d pairs" % (WINDOWS, L)] / med["gather_windows(L = %d)" % L], L + 1, 2 * L, (L + 1) * 408, 2 * L * 408))
    print("  part 4: sample(%d) on the default path" % BATCH)
    order = [("this build", None)]
    if args.reference_root:
        order = [("reference", args.reference_root)] + order + [("reference (again)", args.reference_root)]
    for label, root in order:
        show({label: list(child("part4", root).values())[0]})


if __name__ == "__main__":
    main()
