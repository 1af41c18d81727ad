"""On-policy rollouts (snac_amd/onpolicy.py: RolloutBuffer; snac_gae in snac_amd/csrc/k_onpolicy.hip, snac_replay_gather_onpolicy in
k_replay.hip): device time over back-to-back calls, the median of five timed groups with min / max.  The reference of every comparison is
the torch composition a caller had before, on the same arrays.

  part 1      snac_gae beside torch_gae() below -- the same recurrence as a Python loop over the span, in float64 -- on generated
              [cap, N] arrays, cap = horizon + 1, the span wrapping: N = 65 536 x horizon 128, and N = 1024 x horizon 2048.  For the first
              shape also the bytes the rule moves (17 per slot and env: reward, value and done read, adv and ret written) over the time,
              as a share of the HBM peak.  Four sets of arrays are taken in turn (at the first shape 4 x 143 MB), so that a call finds
              nothing of its arrays in the 256 MiB Infinity Cache.
  part 2      RolloutBuffer.gather() -- one launch -- beside compose(): snac_replay_gather (s, the unwanted s_next, plan) plus five flat
              index gathers and the normalisation, at batch 4096 and 65 536.  2D dynamic, 65 536 envs, a float64 ring of 64 slots (the
              shape of tools/replay_nstep_time.py); new random samples every call, drawn before the timed window.
  part 3      a whole update's data path on that buffer: finish() and one epoch of minibatches(65 536), every minibatch gathered.
Every part is a child process under its own time limit; the first child that fails ends the run.

    python tools/onpolicy_time.py
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from snac_amd import BatchedDMPEnv, RolloutBuffer, _lib  # noqa: E402

ENVS, HORIZON = 65536, 63
GAE_SHAPES = ((65536, 128), (1024, 2048))                            # N, horizon
BATCHES = (4096, 65536)
GROUPS, SETS = 5, 8
GAE_SETS = 4                                                         # sets of arrays that part 1 takes in turn
GAMMA, LAM = 0.99, 0.95
HBM_PEAK = 8.0e12                                                    # bytes / s, the data sheet's
LIMIT = 300                                                          # seconds per child process


def timed(call, reps):
    """ms per call: GROUPS windows of `reps` back-to-back calls between two events."""
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
        out.append(a.elapsed_time(b) / reps)
    return out


def torch_gae(reward, done, value, bootstrap, first, count, gamma, lam, adv, ret):
    """The header's rule with torch: one pass of small launches per slot, newest first."""
    cap = reward.shape[0]
    nv, c = bootstrap.double(), gamma * lam
    a, zero = torch.zeros_like(nv), torch.zeros_like(nv)
    for j in range(count - 1, -1, -1):
        s = (first + j) % cap
        v, d = value[s].double(), done[s] != 0
        delta = (reward[s].double() + torch.where(d, zero, gamma * nv)) - v
        a = delta + torch.where(d, zero, c * a)
        adv[s] = a.float()
        ret[s] = (a + v).float()
        nv = v


def part1():
    dev = torch.device("cuda", torch.cuda.current_device())
    L, vp = _lib.lib(), lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = {}
    for N, H in GAE_SHAPES:
        cap, first = H + 1, H // 2                                   # the span wraps
        g = torch.Generator(device=dev).manual_seed(N)
        sets = []                                                    # GAE_SETS sets of arrays in turn: at the first shape 4 x 143 MB, past the 256 MiB Infinity Cache
        for _ in range(GAE_SETS):
            sets.append(dict(reward=torch.randn((cap, N), device=dev, generator=g) * 10, value=torch.randn((cap, N), device=dev, generator=g) * 10,
                             done=(torch.rand((cap, N), device=dev, generator=g) < 0.05).to(torch.uint8), boot=torch.randn((N,), device=dev, generator=g),
                             adv=torch.zeros((cap, N), device=dev), ret=torch.zeros((cap, N), device=dev)))
        adv_t, ret_t = torch.zeros((cap, N), device=dev), torch.zeros((cap, N), device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        turn = [0]

        def nxt():
            turn[0] += 1
            return sets[turn[0] % GAE_SETS]

        def new():
            a = nxt()
            _lib.check(L.snac_gae(N, cap, first, H, GAMMA, LAM, vp(a["reward"]), vp(a["done"]), vp(a["value"]), vp(a["boot"]), vp(a["adv"]), vp(a["ret"]), stream))

        def old():
            a = nxt()
            torch_gae(a["reward"], a["done"], a["value"], a["boot"], first, H, GAMMA, LAM, adv_t, ret_t)
        out["snac_gae, N = %d x horizon %d" % (N, H)] = timed(new, 20)
        out["torch loop, N = %d x horizon %d" % (N, H)] = timed(old, 2)
        a = nxt()
        new_adv, new_ret = a["adv"].clone(), a["ret"].clone()        # every set was filled in the timed windows
        torch_gae(a["reward"], a["done"], a["value"], a["boot"], first, H, GAMMA, LAM, adv_t, ret_t)
        if not (torch.equal(new_adv, adv_t) and torch.equal(new_ret, ret_t)):
            raise SystemExit("snac_gae and the torch loop differ at N = %d x horizon %d" % (N, H))
    return out


def make():
    env = BatchedDMPEnv(2, True, ENVS, seed=1)
    env.reset()
    buf = RolloutBuffer(env, HORIZON, GAMMA, LAM)
    buf.ring.collect(HORIZON)                                        # random policy, one fused launch
    buf.collected = HORIZON
    g = torch.Generator(device=env.device).manual_seed(2)
    buf.value.copy_(torch.randn(buf.value.shape, device=env.device, generator=g))
    buf.logp.copy_(-torch.rand(buf.logp.shape, device=env.device, generator=g))
    buf.finish(torch.randn((ENVS,), device=env.device, generator=g))
    buf.update_norm()
    return env, buf


def draws(buf, batch):
    """SETS index sets over the span, handed out in turn."""
    dev = buf.env.device
    slots = buf.span_slots()
    sets = [(slots[torch.randint(0, buf.horizon, (batch,), device=dev)].to(torch.int32), torch.randint(0, ENVS, (batch,), device=dev).to(torch.int32))
            for _ in range(SETS)]
    state = [0]

    def nxt():
        state[0] += 1
        return sets[state[0] % SETS]
    return nxt


def compose(buf, slot, env_index):
    """What a caller had before: snac_replay_gather for s and plan (it writes s_next too), five flat index gathers, the normalisation."""
    e, r = buf.env, buf.ring
    B = int(slot.numel())
    s = torch.empty((B, e.obs_dim), dtype=torch.float32, device=e.device)
    s_next = torch.empty_like(s)
    plan = torch.empty((B, r.plan_cells), dtype=torch.float32, device=e.device)
    _lib.check(e._lib.snac_replay_gather(C.byref(e._desc), C.byref(e._state), r.cap, _lib.ptr(r.obs), _lib.ptr(r.first), _lib.ptr(r.plan_idx),
                                         _lib.ptr(slot), _lib.ptr(env_index), B, _lib.ptr(s), _lib.ptr(s_next), _lib.ptr(plan), e._stream()))
    flat = slot.long() * e.num_envs + env_index.long()
    return dict(s=s, plan=plan.view(B, 20, 20), action=r.action.view(-1)[flat].long(), value=buf.value.view(-1)[flat], logp=buf.logp.view(-1)[flat],
                adv=(buf.adv.view(-1)[flat] - buf.norm[0]) * buf.norm[1], ret=buf.ret.view(-1)[flat])


def part2():
    env, buf = make()
    out = {}
    with torch.cuda.device(env.device):
        for B in BATCHES:
            nxt = draws(buf, B)
            slot, idx = nxt()
            a, b = buf.gather(slot, idx), compose(buf, slot, idx)
            for k in b:
                if not torch.equal(a[k], b[k]):
                    raise SystemExit("gather() and the composition differ in %s at batch %d" % (k, B))
            out["RolloutBuffer.gather(), batch %d" % B] = timed(lambda: buf.gather(*nxt()), 20)
            out["snac_replay_gather + 5 index gathers, batch %d" % B] = timed(lambda: compose(buf, *nxt()), 20)
    return out


def part3():
    env, buf = make()
    boot = torch.randn((ENVS,), device=env.device)

    def update():
        buf.collected = HORIZON                                      # the same span again
        buf.finish(boot)
        for mb in buf.minibatches(BATCHES[-1]):
            pass
    with torch.cuda.device(env.device):
        return {"finish() + one epoch of minibatches(%d): %d launches" % (BATCHES[-1], 1 + -(-ENVS * HORIZON // BATCHES[-1])): timed(update, 3)}


PARTS = dict(part1=part1, part2=part2, part3=part3)


def child(part):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", part], capture_output=True, text=True, timeout=LIMIT)
    if out.returncode != 0:                                          # nothing more is started on the device after a failure
        sys.stderr.write(out.stderr[-4000:])
        raise SystemExit("the worker for %s ended with status %d" % (part, out.returncode))
    return json.loads(out.stdout.strip().splitlines()[-1])


def show(rows):
    for label, t in rows.items():
        print("    %-60s median %9.4f   min %9.4f   max %9.4f" % (label, float(np.median(t)), min(t), max(t)), flush=True)
    return {k: float(np.median(t)) for k, t in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:
        print(json.dumps(PARTS[args.worker]()))
        return
    print("ms per call on the device, %d groups of back-to-back calls; gamma %.2f, lambda %.2f" % (GROUPS, GAMMA, LAM))
    print("  part 1: snac_gae beside the same recurrence as a torch loop (float64), equal byte for byte")
    med = show(child("part1"))
    for N, H in GAE_SHAPES:
        print("    N = %d x horizon %d: torch loop / snac_gae %.1f" % (N, H, med["torch loop, N = %d x horizon %d" % (N, H)] / med["snac_gae, N = %d x horizon %d" % (N, H)]))
    N, H = GAE_SHAPES[0]
    rate = 17.0 * N * H / (med["snac_gae, N = %d x horizon %d" % (N, H)] * 1e-3)
    print("    N = %d x horizon %d: %d bytes moved, %.2f TB/s, %.1f %% of the HBM peak of %.1f TB/s" % (N, H, 17 * N * H, rate / 1e12, 100 * rate / HBM_PEAK, HBM_PEAK / 1e12))
    print("  part 2: a PPO minibatch; 2D dynamic, %d envs, a float64 ring of %d slots" % (ENVS, HORIZON + 1))
    med = show(child("part2"))
    for B in BATCHES:
        print("    batch %d: composition / gather() %.2f" % (B, med["snac_replay_gather + 5 index gathers, batch %d" % B] / med["RolloutBuffer.gather(), batch %d" % B]))
    print("  part 3: the data path of one update, %d entries" % (ENVS * HORIZON))
    show(child("part3"))


if __name__ == "__main__":
    main()
