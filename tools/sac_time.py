"""Discrete SAC's device calls (snac_soft_value in snac_amd/csrc/k_soft.hip; SoftValue): device time over back-to-back calls, the median
of five timed groups with min / max.  The reference of every comparison is the torch composition on the same tensors, in the same process,
its groups taking turns with the new call's: log_softmax, exp, minimum, products, sums and the TD combine; for the actor loss the same
through autograd.

  part 1      SoftValue.target(), SoftValue.policy_loss().mean().backward() and SoftValue.entropy() beside their compositions, at
              B = 2048, 4096 and 65 536 for A = 3, 5 and 8; and snac_soft_value itself through the C ABI with every output asked for
              (v, y, entropy and grad in one launch), which has no single counterpart.  The calls through SoftValue carry its argument
              checks and, for the loss, autograd's own nodes (neg, mean and their backward): the host's issue rate bounds them.
  part 2      one tick of examples/sac_batched.py (acting, the env step, the minibatch, the three losses, the optimiser step) with
              SoftValue and with --composition: wall time per tick, from the difference of a run of 40 ticks and one of 10.
  --resources the VGPRs and the scratch of the six kernels from the compiler's resource report (needs hipcc, no GPU).
Every part is a child process under its own time limit; the first child that fails ends the run.

    python tools/sac_time.py [--resources]
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

from snac_amd import SoftValue, _lib  # noqa: E402

SHAPES = tuple((B, A) for A in (3, 5, 8) for B in (2048, 4096, 65536))
GROUPS = 5
REPS = {2048: 500, 4096: 500, 65536: 200}                            # calls per timed window
STEP_ENVS, STEP_BATCH, STEP_TICKS = 4096, 2048, (10, 40)
LIMIT = 420                                                          # seconds per child process
RAW = "snac_soft_value, every output (C ABI)"
PAIRS = (("SoftValue.target", "torch composition of the target"), ("SoftValue.policy_loss().mean().backward()", "torch composition through autograd"),
         ("SoftValue.entropy", "torch -(pi * log pi).sum(1)"))


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
    spec = importlib.util.spec_from_file_location("sac_batched", os.path.join(ROOT, "examples", "sac_batched.py"))
    sac = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sac)
    return sac


def part1():
    sac = example()                                                  # the compositions are the example's
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {}
    for B, A in SHAPES:
        what = "B = %d, A = %d" % (B, A)
        g = torch.Generator(device=dev).manual_seed(B + A)
        logits = (3.0 * torch.randn((B, A), device=dev, generator=g)).requires_grad_()
        q1, q2 = 5.0 * torch.randn((B, A), device=dev, generator=g), 5.0 * torch.randn((B, A), device=dev, generator=g)
        ret = torch.rand(B, device=dev, generator=g) * 10.0 - 5.0
        discount = torch.tensor([0.0, 0.95, 0.95 ** 3, 1.0], device=dev)[torch.randint(0, 4, (B,), device=dev, generator=g)].contiguous()
        alpha = torch.tensor([0.2], device=dev)
        soft = SoftValue(A, device=dev)
        y, v, h, grad = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty((B, A), device=dev)
        data = logits.detach()
        vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        L, stream = _lib.lib(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def raw():
            _lib.check(L.snac_soft_value(B, A, vp(data), vp(q1), vp(q2), vp(alpha), vp(ret), vp(discount), 1.0 / B, vp(v), vp(y), vp(h), vp(grad), None, stream))

        def target():
            soft.target(data, q1, q2, alpha, ret, discount, out=y)

        def loss():
            logits.grad = None
            soft.policy_loss(logits, q1, q2, alpha).mean().backward()

        def loss_torch():
            logits.grad = None
            sac.torch_policy_loss(logits, q1, q2, alpha)[0].mean().backward()
        target()
        loss()
        mine = logits.grad.clone()
        loss_torch()
        if float((y - sac.torch_target(data, q1, q2, alpha, ret, discount)).abs().max()) > 1e-4 or float((mine - logits.grad).abs().max()) > 1e-6:
            raise SystemExit("the kernel and the composition disagree at %s" % what)
        rows = timed({PAIRS[0][0]: target, PAIRS[0][1]: lambda: sac.torch_target(data, q1, q2, alpha, ret, discount), PAIRS[1][0]: loss,
                      PAIRS[1][1]: loss_torch, PAIRS[2][0]: lambda: soft.entropy(data), PAIRS[2][1]: lambda: sac.torch_soft_value(data, q1, q2, alpha)[1],
                      RAW: raw},
                     REPS[B])
        out.update({"%s, %s" % (k, what): v for k, v in rows.items()})
    return out


def part2():
    sac = example()

    def per_tick(composition):
        wall = []
        for ticks in STEP_TICKS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sac.run(envs=STEP_ENVS, ticks=ticks, batch=STEP_BATCH, composition=composition, log=lambda line: None)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        return 1e3 * (wall[1] - wall[0]) / (STEP_TICKS[1] - STEP_TICKS[0])
    calls = {"tick with SoftValue": False, "tick with the torch composition": True}
    for composition in calls.values():
        per_tick(composition)                                        # warm: allocator, kernels' code objects
    out = {k: [] for k in calls}
    for _ in range(GROUPS):
        for label, composition in calls.items():
            out[label].append(per_tick(composition))
    return {"%s, %d envs, batch %d" % (k, STEP_ENVS, STEP_BATCH): v for k, v in out.items()}


PARTS = dict(part1=part1, part2=part2)


def child(part):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", part], capture_output=True, text=True, timeout=LIMIT)
    if out.returncode != 0:                                          # nothing more is started on the device after a failure
        sys.stderr.write(out.stderr[-4000:])
        raise SystemExit("the worker for %s ended with status %d" % (part, out.returncode))
    return json.loads(out.stdout.strip().splitlines()[-1])


def show(rows):
    for label, t in rows.items():
        print("    %-72s median %9.4f   min %9.4f   max %9.4f" % (label, float(np.median(t)), min(t), max(t)), flush=True)
    return {k: float(np.median(t)) for k, t in rows.items()}


def resources():
    """VGPRs and scratch of the unit's kernels, from hipcc -Rpass-analysis=kernel-resource-usage."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-fno-strict-aliasing",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(_lib.CSRC, "k_soft.hip")]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=600).stderr
    for name, body in re.findall(r"Function Name: (\S+)(.*?)LDS Size", text, flags=re.S):
        kernel = re.search(r"k_soft_valueILi(\d)ELb(\d)", name)
        fields = dict(re.findall(r"remark: +(\w+)(?: \[[^\]]*\])?: (\d+)", body))
        print("    %-28s VGPRs %3s   scratch %s bytes/lane   occupancy %s waves/SIMD" % (
            "k_soft_value<%s, %s>" % (kernel.group(1), ("one critic", "two critics")[int(kernel.group(2))]) if kernel else name, fields.get("VGPRs"),
            fields.get("ScratchSize"), fields.get("Occupancy")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--resources", action="store_true", help="print the compiler's resource report of the unit's kernels and stop")
    args = ap.parse_args()
    if args.resources:
        return resources()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    if args.worker:
        print(json.dumps(PARTS[args.worker]()))
        return
    print("ms per call on the device, %d groups of back-to-back calls, the rows of a shape taking turns group by group" % GROUPS)
    print("  part 1: the target, the actor loss with its backward pass, and the entropy")
    med = show(child("part1"))
    for B, A in SHAPES:
        what = "B = %d, A = %d" % (B, A)
        moved = B * (4 * (4 * A + 2) + 12)                          # logits, q1, q2, ret, discount read; grad, v, y, entropy written
        ms = med["%s, %s" % (RAW, what)]
        print("    %s: composition / SoftValue: target %.2f, actor loss and backward %.2f, entropy %.2f; every output at once moves %.2f MB, %.1f GB/s" % (
            (what,) + tuple(med["%s, %s" % (ref, what)] / med["%s, %s" % (new, what)] for new, ref in PAIRS) + (moved / 1e6, moved / ms / 1e6)))
    print("  part 2: one tick of examples/sac_batched.py, wall ms")
    med = show(child("part2"))
    a, b = (med["%s, %d envs, batch %d" % (k, STEP_ENVS, STEP_BATCH)] for k in ("tick with the torch composition", "tick with SoftValue"))
    print("    composition / SoftValue  %.2f" % (a / b))


if __name__ == "__main__":
    main()
