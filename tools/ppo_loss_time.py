"""PPO's loss on the device (snac_ppo_loss in snac_amd/csrc/k_ppo.hip; PPOLoss): device time over back-to-back calls, the median of five
timed groups with min / max.  The reference of every comparison is the torch composition of examples/ppo_batched.py (Categorical,
log_prob, exp, clamp, min, three means, entropy, and autograd back through all of it) on the same tensors, in the same process, its
groups taking turns with the new call's.

  part 1      snac_ppo_loss through the C ABI with every output asked for (both launches), PPOLoss.loss() with backward(), and the
              composition with backward(), at B = 8192 and 65 536 for A = 3, 5 and 8.  The calls through PPOLoss carry its argument
              checks, five small allocations and autograd's node: the host's issue rate bounds them.
  part 2      one update minibatch of examples/ppo_batched.py (the network's forward pass, the loss, backward, the gradient clip and
              Adam) with --device-loss and without: wall time per minibatch, from the difference of runs of 3 iterations and of 1.
  --resources the VGPRs and the scratch of the seven kernels from the compiler's resource report (needs hipcc, no GPU).
Every part is a child process under its own time limit; the first child that fails ends the run.

    python tools/ppo_loss_time.py [--resources] [--out profiles/r26_ppo_loss.txt]
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from snac_amd import PPOLoss, _lib  # noqa: E402

SHAPES = tuple((B, A) for A in (3, 5, 8) for B in (8192, 65536))
GROUPS = 5
REPS = {8192: 300, 65536: 150}                                       # calls per timed window
CLIP, VF_COEF, ENT_COEF = 0.2, 0.5, 0.01
STEP_ENVS, STEP_HORIZON, STEP_BATCH, STEP_EPOCHS, STEP_ITERS = 4096, 16, 8192, 4, (1, 3)
LIMIT = 420                                                          # seconds per child process
RAW, NEW, REF = "snac_ppo_loss, every output (C ABI)", "PPOLoss.loss().backward()", "torch composition, forward and backward"


def timed(calls, reps):
    """{label: [ms per call] * GROUPS}: per group every call in turn, `reps` back-to-back calls between two events."""
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


def example():
    spec = importlib.util.spec_from_file_location("ppo_batched", os.path.join(ROOT, "examples", "ppo_batched.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def part1():
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {}
    for B, A in SHAPES:
        what = "B = %d, A = %d" % (B, A)
        g = torch.Generator(device=dev).manual_seed(B + A)
        logits = (2.0 * torch.randn((B, A), device=dev, generator=g)).requires_grad_()
        value = torch.randn(B, device=dev, generator=g).requires_grad_()
        action = torch.randint(0, A, (B,), device=dev, generator=g)
        logp = (torch.log_softmax(logits.detach(), 1).gather(1, action[:, None])[:, 0] - 0.15 * torch.randn(B, device=dev, generator=g)).contiguous()
        adv, ret = torch.randn(B, device=dev, generator=g), torch.randn(B, device=dev, generator=g)
        value_old = (value.detach() + 0.3 * torch.randn(B, device=dev, generator=g)).contiguous()
        mb = dict(action=action, logp=logp, adv=adv, ret=ret, value=value_old)
        ppo = PPOLoss(A, CLIP, -1.0, VF_COEF, ENT_COEF, device=dev)  # the value function not clipped: what the composition computes
        loss, gl, gv = torch.empty(B, device=dev), torch.empty((B, A), device=dev), torch.empty(B, device=dev)
        stats, partials = torch.empty(8, dtype=torch.float64, device=dev), torch.empty(((B + 63) // 64, 8), dtype=torch.float64, device=dev)
        mean = torch.empty((), device=dev)
        vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        L, stream = _lib.lib(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ld, vd = logits.detach(), value.detach()

        def raw():
            _lib.check(L.snac_ppo_loss(B, A, vp(ld), vp(action), vp(logp), vp(adv), vp(vd), None, vp(ret), CLIP, -1.0, VF_COEF, ENT_COEF, 1.0 / B,
                                       vp(loss), vp(gl), vp(gv), vp(stats), vp(mean), vp(partials), None, stream))

        def new():
            logits.grad = value.grad = None
            ppo.loss(logits, value, mb).backward()

        def ref():
            logits.grad = value.grad = None
            dist = torch.distributions.Categorical(logits=logits)
            ratio = torch.exp(dist.log_prob(action) - logp)
            surrogate = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * adv).mean()
            value_loss = 0.5 * ((value - ret) ** 2).mean()
            total = -surrogate + VF_COEF * value_loss - ENT_COEF * dist.entropy().mean()
            total.backward()
            return total
        new()
        mine_l, mine_v, mine = logits.grad.clone(), value.grad.clone(), float(ppo.stats[0])
        theirs = float(ref())
        if abs(mine - theirs) > 1e-4 * max(1.0, abs(theirs)) or float((mine_l - logits.grad).abs().max()) > 1e-6 or float((mine_v - value.grad).abs().max()) > 1e-6:
            raise SystemExit("the kernel and the composition disagree at %s" % what)
        rows = timed({RAW: raw, NEW: new, REF: ref}, REPS[B])
        out.update({"%s, %s" % (k, what): v for k, v in rows.items()})
    return out


def part2():
    mod = example()
    per_iteration = STEP_EPOCHS * (STEP_ENVS * STEP_HORIZON // STEP_BATCH)

    def per_minibatch(device_loss):
        wall = []
        for iterations in STEP_ITERS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mod.run(envs=STEP_ENVS, iterations=iterations, horizon=STEP_HORIZON, epochs=STEP_EPOCHS, batch=STEP_BATCH, device_sampling=True,
                    device_loss=device_loss, log=lambda line: None)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        return 1e3 * (wall[1] - wall[0]) / ((STEP_ITERS[1] - STEP_ITERS[0]) * per_iteration)
    calls = {"iteration share per minibatch with --device-loss": True, "iteration share per minibatch with the torch composition": False}
    for device_loss in calls.values():
        per_minibatch(device_loss)                                   # warm: allocator, kernels' code objects
    out = {k: [] for k in calls}
    for _ in range(GROUPS):
        for label, device_loss in calls.items():
            out[label].append(per_minibatch(device_loss))
    return {"%s, %d envs, batch %d" % (k, STEP_ENVS, STEP_BATCH): v for k, v in out.items()}


PARTS = dict(part1=part1, part2=part2)


def child(part):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", part], capture_output=True, text=True, timeout=LIMIT)
    if out.returncode != 0:                                          # nothing more is started on the device after a failure
        sys.stderr.write(out.stderr[-4000:])
        raise SystemExit("the worker for %s ended with status %d" % (part, out.returncode))
    return json.loads(out.stdout.strip().splitlines()[-1])


def resources(say=print):
    """VGPRs and scratch of the unit's kernels, from hipcc -Rpass-analysis=kernel-resource-usage."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-fno-strict-aliasing",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(_lib.CSRC, "k_ppo.hip")]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=600).stderr
    for name, body in re.findall(r"Function Name: (\S+)(.*?)LDS Size", text, flags=re.S):
        kernel = re.search(r"k_ppo_lossILi(\d)ELb(\d)", name)
        fields = dict(re.findall(r"remark: +(\w+)(?: \[[^\]]*\])?: (\d+)", body))
        label = "k_ppo_loss<%s, %s>" % (kernel.group(1), ("value not clipped", "value clipped")[int(kernel.group(2))]) if kernel else "k_ppo_reduce"
        say("    %-36s VGPRs %3s   scratch %s bytes/lane   occupancy %s waves/SIMD" % (label, fields.get("VGPRs"), fields.get("ScratchSize"), fields.get("Occupancy")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--resources", action="store_true", help="print the compiler's resource report of the unit's kernels and stop")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(PARTS[args.worker]()))
        return
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def show(rows):
        for label, t in rows.items():
            say("    %-84s median %9.4f   min %9.4f   max %9.4f" % (label, float(np.median(t)), min(t), max(t)))
        return {k: float(np.median(t)) for k, t in rows.items()}
    if args.resources:
        return resources()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    say("ms per call on the device, %d groups of back-to-back calls, the rows of a shape taking turns group by group" % GROUPS)
    say("  part 1: the loss with its statistics and its gradient")
    med = show(child("part1"))
    for B, A in SHAPES:
        what = "B = %d, A = %d" % (B, A)
        moved = B * (4 * (2 * A + 7) + 8)                            # logits, action and four scalars read; loss, both gradients written
        raw, new, ref = (med["%s, %s" % (k, what)] for k in (RAW, NEW, REF))
        say("    %s: composition / PPOLoss %.2f; composition / C ABI %.2f; the C ABI call moves %.2f MB, %.1f GB/s" % (
            what, ref / new, ref / raw, moved / 1e6, moved / raw / 1e6))
    say("  part 2: examples/ppo_batched.py, wall ms per update minibatch (the rollout's share included)")
    med = show(child("part2"))
    a, b = (med["iteration share per minibatch with %s, %d envs, batch %d" % (k, STEP_ENVS, STEP_BATCH)] for k in ("the torch composition", "--device-loss"))
    say("    composition / --device-loss  %.2f" % (a / b))
    say("  the compiler's resource report")
    resources(say)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
