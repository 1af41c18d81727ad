"""The search loss on the device (snac_search_loss in snac_amd/csrc/k_search.hip; SearchLoss): device time over back-to-back calls, the
median of five timed groups with min / max.  The reference of every comparison is the torch composition of
examples/alphazero_selfplay.py on the same tensors, in the same process, its groups taking turns with the new call's.

  part 1      snac_search_loss through the C ABI with every output asked for (both launches), SearchLoss.loss().backward() with the
              priorities, and the composition of --prioritized (log_softmax, the product with pi, the sums, the squared value error,
              the weights, the two means, abs() for the priorities) with backward(), at B = 256 (the example's), 8192 and 65 536 for
              A = 3, 5 and 8.
  part 2      one training step of examples/alphazero_selfplay.py with and without --device-loss, plain and --prioritized: wall time per
              step, from the difference of runs of 12 steps and of 4.  With --parent-example FILE (examples/alphazero_selfplay.py of the
              parent commit) also that file's default step, twice, beside this tree's, on this tree's library: the spread of the two is
              what the default step is held against.
  --resources the VGPRs, LDS and scratch of the unit's kernels from the compiler's resource report (needs hipcc, no GPU).
Every part is a child process under its own time limit; the first child that fails ends the run.

    python tools/search_loss_time.py [--resources] [--parent-example FILE] [--out profiles/r29_search_loss.txt]
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

from snac_amd import SearchLoss, _lib  # noqa: E402

SHAPES = tuple((B, A) for A in (3, 5, 8) for B in (256, 8192, 65536))
GROUPS = 5
REPS = {256: 300, 8192: 300, 65536: 150}                             # calls per timed window
STEPS = (4, 12)
LIMIT = 420                                                          # seconds per child process
RAW, NEW, REF = "snac_search_loss, every output (C ABI)", "SearchLoss.loss().backward()", "torch composition of --prioritized, forward and backward"


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


def example(path=None):
    spec = importlib.util.spec_from_file_location("alphazero_selfplay", path or os.path.join(ROOT, "examples", "alphazero_selfplay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def vp(t):
    return C.c_void_p(t.data_ptr())


def part1():
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {}
    for B, A in SHAPES:
        what = "B = %d, A = %d" % (B, A)
        g = torch.Generator(device=dev).manual_seed(B + A)
        y = (1.5 * torch.randn((B, A + 1), device=dev, generator=g)).requires_grad_()      # the network's joint output, as the example's
        b = dict(pi=torch.softmax(torch.randn((B, A), device=dev, generator=g), dim=1).contiguous(), z=torch.randn(B, device=dev, generator=g),
                 weight=0.1 + 0.9 * torch.rand(B, device=dev, generator=g))
        sl = SearchLoss(A, device=dev)
        loss, prio, gv, gl = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty((B, A), device=dev)
        stats, partials = torch.empty(8, dtype=torch.float64, device=dev), torch.empty(((B + 63) // 64, 8), dtype=torch.float64, device=dev)
        mean = torch.empty((), device=dev)
        L, stream = _lib.lib(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ld, vd = y.detach()[:, :A].contiguous(), y.detach()[:, A].contiguous()
        keep = {}

        def raw():
            _lib.check(L.snac_search_loss(B, A, vp(ld), vp(vd), vp(b["pi"]), vp(b["z"]), vp(b["weight"]), 1.0, 0.0, 1.0 / B, vp(loss), vp(prio), vp(gl),
                                          vp(gv), vp(stats), vp(mean), vp(partials), None, stream))

        def new():                                                   # as the example's --device-loss: the two heads made contiguous
            y.grad = None
            m, _, keep["prio"] = sl.loss(y[:, :A].contiguous(), y[:, A].contiguous(), b, want_per_sample=True)
            m.backward()
            return m

        def ref():                                                   # the example's lines
            y.grad = None
            policy_loss = -(b["weight"] * (b["pi"] * torch.log_softmax(y[:, :A], 1)).sum(1)).mean()
            value_loss = (b["weight"] * (y[:, A] - b["z"]) ** 2).mean()
            keep["ref_prio"] = (y[:, A].detach() - b["z"]).abs() ** 1.0
            total = policy_loss + value_loss
            total.backward()
            return total
        mine, mine_g = float(new()), y.grad.clone()
        theirs = float(ref())
        if abs(mine - theirs) > 1e-4 * max(1.0, abs(theirs)) or float((mine_g - y.grad).abs().max()) > 1e-6 or \
                float((keep["prio"] - keep["ref_prio"]).abs().max()) > 1e-4:
            raise SystemExit("the kernel and the composition disagree at %s" % what)
        rows = timed({RAW: raw, NEW: new, REF: ref}, REPS[B])
        out.update({"%s, %s" % (k, what): v for k, v in rows.items()})
    return out


def part2(parent=None):
    mods = {"this tree": example()}
    if parent:
        mods["parent"] = example(parent)

    def per_step(mod, how):
        wall = []
        for steps in STEPS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mod.train(steps=steps, **how)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        return 1e3 * (wall[1] - wall[0]) / (STEPS[1] - STEPS[0])
    calls = {"plain, torch composition (the default step), this tree": ("this tree", {}),
             "plain, --device-loss": ("this tree", dict(device_loss=True)),
             "--prioritized, torch composition": ("this tree", dict(prioritized=True)),
             "--prioritized, --device-loss": ("this tree", dict(prioritized=True, device_loss=True))}
    if parent:
        calls["plain, torch composition (the default step), the parent's example, run 1"] = ("parent", {})
        calls["plain, torch composition (the default step), the parent's example, run 2"] = ("parent", {})
    for which, how in calls.values():
        per_step(mods[which], how)                                   # warm: allocator, kernels' code objects
    out = {k: [] for k in calls}
    for _ in range(GROUPS):
        for label, (which, how) in calls.items():
            out[label].append(per_step(mods[which], how))
    return {"%s, 64 envs, batch 256" % k: v for k, v in out.items()}


PARTS = dict(part1=part1, part2=part2)


def child(part, *args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", part] + list(args), capture_output=True, text=True, timeout=LIMIT)
    if out.returncode != 0:                                          # nothing more is started on the device after a failure
        sys.stderr.write(out.stderr[-4000:])
        raise SystemExit("the worker for %s ended with status %d" % (part, out.returncode))
    return json.loads(out.stdout.strip().splitlines()[-1])


def resources(say=print):
    """VGPRs, LDS and scratch of the unit's kernels, from hipcc -Rpass-analysis=kernel-resource-usage."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-fno-strict-aliasing",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(_lib.CSRC, "k_search.hip")]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=600).stderr
    for name, body in re.findall(r"Function Name: (\S+)(.*?LDS Size[^\n]*)", text, flags=re.S):
        loss = re.search(r"k_search_lossILi(\d)", name)
        fields = dict(re.findall(r"remark: +(\w+)(?: Size)?(?: \[[^\]]*\])?: (\d+)", body))      # (the "Spill" lines do not match)
        say("    %-28s VGPRs %3s   scratch %s bytes/lane   LDS %4s bytes/block   occupancy %s waves/SIMD" % (
            "k_search_loss<%s>" % loss.group(1) if loss else "k_search_reduce", fields.get("VGPRs"), fields.get("ScratchSize"), fields.get("LDS"),
            fields.get("Occupancy")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", nargs="+", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--resources", action="store_true", help="print the compiler's resource report of the unit's kernels and stop")
    ap.add_argument("--parent-example", default=None, help="examples/alphazero_selfplay.py of the parent commit, for part 2")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(PARTS[args.worker[0]](*args.worker[1:])))
        return
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def show(rows):
        for label, t in rows.items():
            say("    %-100s median %9.4f   min %9.4f   max %9.4f" % (label, float(np.median(t)), min(t), max(t)))
        return {k: float(np.median(t)) for k, t in rows.items()}
    if args.resources:
        return resources()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    say("ms per call on the device, %d groups of back-to-back calls, the rows of a shape taking turns group by group" % GROUPS)
    say("  part 1: snac_search_loss: the loss with its statistics, both gradients and the priorities")
    med = show(child("part1"))
    slower = []
    for B, A in SHAPES:
        what = "B = %d, A = %d" % (B, A)
        raw, new, ref = (med["%s, %s" % (k, what)] for k in (RAW, NEW, REF))
        moved = B * 4 * (3 * A + 6)                                  # logits, pi, value, z, weight read; three [B] and grad_logits written
        say("    %s: composition / wrapper %.2f; composition / C ABI %.2f; the C ABI call moves %.2f MB, %.1f GB/s" % (
            what, ref / new, ref / raw, moved / 1e6, moved / raw / 1e6))
        if new > ref:
            slower.append(what)
    say("    shapes at which the wrapper's median is above the composition's: %s" % (", ".join(slower) or "none"))
    say("  part 2: examples/alphazero_selfplay.py, wall ms per step (the search, the sample, the network and the update included)")
    rows = child("part2", *([args.parent_example] if args.parent_example else []))
    med = show(rows)
    tail = ", 64 envs, batch 256"
    say("    plain: composition / --device-loss  %.3f" % (med["plain, torch composition (the default step), this tree" + tail] / med["plain, --device-loss" + tail]))
    say("    --prioritized: composition / --device-loss  %.3f" % (med["--prioritized, torch composition" + tail] / med["--prioritized, --device-loss" + tail]))
    if args.parent_example:
        runs = [med["plain, torch composition (the default step), the parent's example, run %d" % n + tail] for n in (1, 2)]
        both = [t for n in (1, 2) for t in rows["plain, torch composition (the default step), the parent's example, run %d" % n + tail]]
        mine = med["plain, torch composition (the default step), this tree" + tail]
        say("    the default step: this tree %.4f; the parent's two runs %.4f and %.4f (their groups: %.4f .. %.4f): %s" % (
            mine, runs[0], runs[1], min(both), max(both), "inside their spread" if min(both) <= mine <= max(both) else "OUTSIDE their spread"))
    say("  the compiler's resource report")
    resources(say)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
