"""The Q-learning losses on the device (snac_td_loss, snac_c51_loss in snac_amd/csrc/k_qloss.hip; TDLoss, CategoricalSupport.loss): device
time over back-to-back calls, the median of five timed groups with min / max.  The reference of every comparison is the torch
composition of examples/dqn_batched.py on the same tensors, in the same process, its groups taking turns with the new call's.

  part 1      snac_td_loss through the C ABI with every output asked for (both launches), TDLoss.loss().backward() with the priorities,
              and the composition of --prioritized (max, the target arithmetic, gather, the difference, the square, the weight, the mean,
              abs() for the priorities) with backward(), at B = 2048, 8192 and 65 536 for A = 3, 5 and 8.
  part 2      the same for snac_c51_loss, CategoricalSupport.loss().backward() and the composition of --distributional --prioritized
              (log_softmax over [B, A, K], the advanced-index gather, the product, the sum, the weighting, the mean), K = 51.
  part 3      one tick of examples/dqn_batched.py with and without --device-loss, plain and --distributional --prioritized --n-step 3:
              wall time per tick, from the difference of runs of 24 ticks and of 8.  With --parent-example FILE (examples/dqn_batched.py
              of the parent commit) also that file's default tick beside this tree's, on this tree's library.
  --waves DIR part 2's C ABI row for every libsnac_hip_w<N>.so in DIR: the library built with -DSNAC_C51L_WAVES=N (waves per block of
              k_c51_loss; 64 / N samples per wave).
  --resources the VGPRs, LDS and scratch of the unit's kernels from the compiler's resource report (needs hipcc, no GPU).
Every part is a child process under its own time limit; the first child that fails ends the run.

    python tools/qloss_time.py [--resources] [--waves DIR] [--parent-example FILE] [--out profiles/r28_qloss.txt]
"""
import argparse
import ctypes as C
import glob
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

from snac_amd import CategoricalSupport, TDLoss, _lib  # noqa: E402

SHAPES = tuple((B, A) for A in (3, 5, 8) for B in (2048, 8192, 65536))
ATOMS = 51
GROUPS = 5
REPS = {2048: 300, 8192: 300, 65536: 150}                            # calls per timed window
TICK_ENVS, TICK_BATCH, TICKS = 4096, 2048, (8, 24)
LIMIT = 420                                                          # seconds per child process
RAW, NEW, REF = "%s, every output (C ABI)", "%s().backward()", "torch composition of %s, forward and backward"


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
    spec = importlib.util.spec_from_file_location("dqn_batched", path or os.path.join(ROOT, "examples", "dqn_batched.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def vp(t):
    return C.c_void_p(t.data_ptr())


def td_inputs(B, A, dev):
    g = torch.Generator(device=dev).manual_seed(B + A)
    q = (2.0 * torch.randn((B, A), device=dev, generator=g)).requires_grad_()
    q_next = 2.0 * torch.randn((B, A), device=dev, generator=g)
    action = torch.randint(0, A, (B,), device=dev, generator=g)
    ret, discount = torch.randn(B, device=dev, generator=g), torch.full((B,), 0.95, device=dev)
    weight = 0.1 + 0.9 * torch.rand(B, device=dev, generator=g)
    return q, q_next, action, ret, discount, weight


def part1():
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {}
    names = tuple(k % n for k, n in ((RAW, "snac_td_loss"), (NEW, "TDLoss.loss"), (REF, "--prioritized")))
    for B, A in SHAPES:
        what = "B = %d, A = %d" % (B, A)
        q, q_next, action, ret, discount, weight = td_inputs(B, A, dev)
        td = TDLoss(A, device=dev)
        loss, prio, y_out, gq = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty((B, A), device=dev)
        stats, partials = torch.empty(8, dtype=torch.float64, device=dev), torch.empty(((B + 63) // 64, 8), dtype=torch.float64, device=dev)
        mean = torch.empty((), device=dev)
        L, stream = _lib.lib(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        qd = q.detach()
        keep = {}

        def raw():
            _lib.check(L.snac_td_loss(B, A, vp(qd), vp(action), None, vp(q_next), None, vp(ret), vp(discount), vp(weight), 0.0, 1.0 / B, vp(loss),
                                      vp(prio), vp(y_out), vp(gq), vp(stats), vp(mean), vp(partials), None, stream))

        def new():
            q.grad = None
            m, _, keep["prio"] = td.loss(q, action, q_next=q_next, ret=ret, discount=discount, weight=weight, want_per_sample=True)
            m.backward()
            return m

        def ref():
            q.grad = None
            y = ret + discount * q_next.max(dim=1).values
            d = q.gather(1, action[:, None]).squeeze(1) - y
            total = (weight * d ** 2).mean()
            keep["ref_prio"] = d.detach().abs()
            total.backward()
            return total
        mine, mine_g = float(new()), q.grad.clone()
        theirs = float(ref())
        if abs(mine - theirs) > 1e-4 * max(1.0, abs(theirs)) or float((mine_g - q.grad).abs().max()) > 1e-6 or \
                float((keep["prio"] - keep["ref_prio"]).abs().max()) > 1e-4:
            raise SystemExit("the kernel and the composition disagree at %s" % what)
        rows = timed(dict(zip(names, (raw, new, ref))), REPS[B])
        out.update({"%s, %s" % (k, what): v for k, v in rows.items()})
    return out


def c51_inputs(B, A, dev):
    g = torch.Generator(device=dev).manual_seed(B + A)
    logits = (1.5 * torch.randn((B, A, ATOMS), device=dev, generator=g)).requires_grad_()
    m = torch.softmax(torch.randn((B, ATOMS), device=dev, generator=g), dim=1).contiguous()
    action = torch.randint(0, A, (B,), device=dev, generator=g)
    weight = 0.1 + 0.9 * torch.rand(B, device=dev, generator=g)
    return logits, m, action, weight


def part2():
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {}
    names = tuple(k % n for k, n in ((RAW, "snac_c51_loss"), (NEW, "CategoricalSupport.loss"), (REF, "--distributional --prioritized")))
    for B, A in SHAPES:
        what = "B = %d, A = %d, K = %d" % (B, A, ATOMS)
        logits, m, action, weight = c51_inputs(B, A, dev)
        sup = CategoricalSupport(A, atoms=ATOMS, device=dev)
        loss, grad = torch.empty(B, device=dev), torch.empty((B, A, ATOMS), device=dev)
        stats, partials = torch.empty(8, dtype=torch.float64, device=dev), torch.empty(((B + 63) // 64, 8), dtype=torch.float64, device=dev)
        mean = torch.empty((), device=dev)
        L, stream = _lib.lib(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ld, every = logits.detach(), torch.arange(B, device=dev)

        def raw():
            _lib.check(L.snac_c51_loss(B, A, ATOMS, vp(ld), vp(action), vp(m), vp(weight), 1.0 / B, vp(loss), vp(grad), vp(stats), vp(mean), vp(partials),
                                       None, stream))

        def new():
            logits.grad = None
            mean_loss, _ = sup.loss(logits, action, m, weight=weight, want_per_sample=True)
            mean_loss.backward()
            return mean_loss

        def ref():
            logits.grad = None
            ce = -(m * logits.log_softmax(-1)[every, action]).sum(1)
            total = (weight * ce).mean()
            total.backward()
            return total
        mine, mine_g = float(new()), logits.grad.clone()
        theirs = float(ref())
        if abs(mine - theirs) > 1e-4 * max(1.0, abs(theirs)) or float((mine_g - logits.grad).abs().max()) > 1e-6:
            raise SystemExit("the kernel and the composition disagree at %s" % what)
        rows = timed(dict(zip(names, (raw, new, ref))), REPS[B])
        out.update({"%s, %s" % (k, what): v for k, v in rows.items()})
    return out


def part3(parent=None):
    mods = {"this tree": example()}
    if parent:
        mods["the parent's example"] = example(parent)

    def per_tick(mod, how):
        wall = []
        for ticks in TICKS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mod.run(envs=TICK_ENVS, ticks=ticks, batch=TICK_BATCH, prefill=16, replace=1000, log=lambda line: None, **how)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        return 1e3 * (wall[1] - wall[0]) / (TICKS[1] - TICKS[0])
    rainbow = dict(distributional=True, prioritized=True, n_step=3)
    calls = {"plain, torch composition (the default tick), this tree": ("this tree", {}),
             "plain, --device-loss": ("this tree", dict(device_loss=True)),
             "--distributional --prioritized --n-step 3, torch composition": ("this tree", rainbow),
             "--distributional --prioritized --n-step 3, --device-loss": ("this tree", dict(rainbow, device_loss=True))}
    if parent:
        calls["plain, torch composition (the default tick), the parent's example"] = ("the parent's example", {})
    for which, how in calls.values():
        per_tick(mods[which], how)                                   # warm: allocator, kernels' code objects
    out = {k: [] for k in calls}
    for _ in range(GROUPS):
        for label, (which, how) in calls.items():
            out[label].append(per_tick(mods[which], how))
    return {"%s, %d envs, batch %d" % (k, TICK_ENVS, TICK_BATCH): v for k, v in out.items()}


def waves(directory):
    """snac_c51_loss through the C ABI of every variant library in `directory`, their groups taking turns."""
    dev = torch.device("cuda", torch.cuda.current_device())
    libs = {}
    for path in sorted(glob.glob(os.path.join(directory, "libsnac_hip_w*.so")), key=lambda p: int(re.search(r"_w(\d+)\.so", p).group(1))):
        L = C.CDLL(path)
        L.snac_c51_loss.restype, L.snac_c51_loss.argtypes = _lib.PROTOTYPES["snac_c51_loss"]
        libs[int(re.search(r"_w(\d+)\.so", path).group(1))] = L
    out = {}
    for B, A in ((2048, 5), (8192, 5), (65536, 5), (65536, 8)):
        logits, m, action, weight = c51_inputs(B, A, dev)
        loss, grad = torch.empty(B, device=dev), torch.empty((B, A, ATOMS), device=dev)
        stats, partials = torch.empty(8, dtype=torch.float64, device=dev), torch.empty(((B + 63) // 64, 8), dtype=torch.float64, device=dev)
        mean = torch.empty((), device=dev)
        stream, ld = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), logits.detach()

        def call(L):
            def raw():
                if L.snac_c51_loss(B, A, ATOMS, vp(ld), vp(action), vp(m), vp(weight), 1.0 / B, vp(loss), vp(grad), vp(stats), vp(mean), vp(partials),
                                   None, stream) != 0:
                    raise SystemExit("snac_c51_loss failed")
            return raw
        first = None
        for n, L in libs.items():                                    # every variant gives the same bytes
            call(L)()
            got = (loss.clone(), grad.clone(), stats.clone())
            if first is not None and not all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, got)):
                raise SystemExit("the variant with %d waves gives other bytes" % n)
            first = got
        rows = timed({"%2d waves a block, %2d samples a wave" % (n, 64 // n): call(L) for n, L in libs.items()}, REPS[B])
        out.update({"%s, B = %d, A = %d, K = %d" % (k, B, A, ATOMS): v for k, v in rows.items()})
    return out


PARTS = dict(part1=part1, part2=part2, part3=part3, waves=waves)


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
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(_lib.CSRC, "k_qloss.hip")]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=600).stderr
    for name, body in re.findall(r"Function Name: (\S+)(.*?LDS Size[^\n]*)", text, flags=re.S):
        td, c51 = re.search(r"k_td_lossILi(\d)ELi(\d)", name), re.search(r"k_c51_lossILi(\d)", name)
        fields = dict(re.findall(r"remark: +(\w+)(?: Size)?(?: \[[^\]]*\])?: (\d+)", body))      # (the "Spill" lines do not match)
        label = "k_td_loss<%s, %s>" % (td.group(1), ("y", "next", "double")[int(td.group(2))]) if td else "k_c51_loss<%s>" % c51.group(1) if c51 else "k_q_reduce"
        say("    %-28s VGPRs %3s   scratch %s bytes/lane   LDS %4s bytes/block   occupancy %s waves/SIMD" % (
            label, fields.get("VGPRs"), fields.get("ScratchSize"), fields.get("LDS"), fields.get("Occupancy")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", nargs="+", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--resources", action="store_true", help="print the compiler's resource report of the unit's kernels and stop")
    ap.add_argument("--waves", default=None, help="a directory of libsnac_hip_w<N>.so variants to compare")
    ap.add_argument("--parent-example", default=None, help="examples/dqn_batched.py of the parent commit, for part 3")
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
    for part, title, names, moved in (
            ("part1", "snac_td_loss: the loss with its statistics, its gradient and the priorities", ("snac_td_loss", "TDLoss.loss", "--prioritized"),
             lambda B, A: B * (4 * (3 * A + 6) + 8)),                 # q, q_next, action, ret, discount, weight read; three [B] and grad_q written
            ("part2", "snac_c51_loss: the cross-entropy with its statistics and its gradient",
             ("snac_c51_loss", "CategoricalSupport.loss", "--distributional --prioritized"),
             lambda B, A: B * (4 * ((A + 2) * ATOMS + 2) + 8))):      # one row of logits, m, action, weight read; loss and the block written
        say("  %s: %s" % (part.replace("part", "part "), title))
        med = show(child(part))
        for B, A in SHAPES:
            what = "B = %d, A = %d" % (B, A) + (", K = %d" % ATOMS if part == "part2" else "")
            raw, new, ref = (med["%s, %s" % (k % n, what)] for k, n in zip((RAW, NEW, REF), names))
            say("    %s: composition / wrapper %.2f; composition / C ABI %.2f; the C ABI call moves %.2f MB, %.1f GB/s" % (
                what, ref / new, ref / raw, moved(B, A) / 1e6, moved(B, A) / raw / 1e6))
    say("  part 3: examples/dqn_batched.py, wall ms per tick (acting, the env tick, the sample, the networks and the update included)")
    med = show(child("part3", *([args.parent_example] if args.parent_example else [])))
    tail = ", %d envs, batch %d" % (TICK_ENVS, TICK_BATCH)
    say("    plain: composition / --device-loss  %.2f" % (med["plain, torch composition (the default tick), this tree" + tail] / med["plain, --device-loss" + tail]))
    say("    --distributional --prioritized --n-step 3: composition / --device-loss  %.2f" % (
        med["--distributional --prioritized --n-step 3, torch composition" + tail] / med["--distributional --prioritized --n-step 3, --device-loss" + tail]))
    if args.parent_example:
        say("    the default tick: this tree / the parent's example  %.3f" % (
            med["plain, torch composition (the default tick), this tree" + tail] / med["plain, torch composition (the default tick), the parent's example" + tail]))
    if args.waves:
        say("  k_c51_loss by waves per block (the library built with -DSNAC_C51L_WAVES=N), snac_c51_loss through the C ABI, every output")
        show(child("waves", args.waves))
    say("  the compiler's resource report")
    resources(say)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
