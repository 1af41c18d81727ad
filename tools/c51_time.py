"""Distributional targets (snac_c51_project / snac_c51_expect in snac_amd/csrc/k_dist.hip; CategoricalSupport): device time over
back-to-back calls, the median of five timed groups with min / max.  The reference of every comparison is the textbook composition in
torch on the same tensors, in the same process, its groups taking turns with the new call's: expected values, arg-max, gather of the row,
clamp, floor / ceil with the usual repairs, two index_add_ (whose float atomics make its bits change from run to run).

  part 1      snac_c51_project (double DQN: p_select given; a_star and q_star written) and snac_c51_expect into reused outputs beside the
              composition, at B = 2048, 4096 and 65 536 for A = 5 and 8, K = 51 on [-10, 10]; with the bytes a call moves (the A rows of
              p_select, the chosen row of p_next, ret and discount read; m, a_star and q_star written) and the rate that makes.
  part 2      one tick of examples/dqn_batched.py --distributional --prioritized --n-step 3 (acting, the env step, the minibatch, the
              learner step) with CategoricalSupport.project and with the composition swapped in for it (run(projection=...)): wall time
              per tick, from the difference of a run of 40 ticks and one of 10.
  --resources the VGPRs and the scratch of the six kernels from the compiler's resource report (needs hipcc, no GPU).
Every part is a child process under its own time limit; the first child that fails ends the run.

    python tools/c51_time.py [--resources]
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

from snac_amd import CategoricalSupport, _lib  # noqa: E402

SHAPES = tuple((B, A) for A in (5, 8) for B in (2048, 4096, 65536))
K, VMIN, VMAX = 51, -10.0, 10.0
GROUPS = 5
REPS = {2048: 1000, 4096: 1000, 65536: 200}                          # calls per timed window
STEP_ENVS, STEP_BATCH, STEP_TICKS = 4096, 2048, (10, 40)
LIMIT = 420                                                          # seconds per child process


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


def torch_expected(z, p):
    return (p * z).sum(-1)


def torch_project(z, vmin, vmax, p_next, ret, discount, p_select=None):
    """The textbook composition, float32: (m [B, K], a_star [B]).  b, l and u are held inside the support: index_add_ checks no index."""
    B, A, K = p_next.shape
    dz = (vmax - vmin) / (K - 1)
    a_star = torch_expected(z, p_next if p_select is None else p_select).argmax(dim=1)
    p = p_next[torch.arange(B, device=p_next.device), a_star]
    tz = (ret[:, None] + discount[:, None] * z[None, :]).clamp(vmin, vmax)
    b = ((tz - vmin) / dz).clamp(0.0, float(K - 1))
    l, u = b.floor().long(), b.ceil().long()
    l[(u > 0) & (l == u)] -= 1
    u[(l < K - 1) & (l == u)] += 1
    l, u = l.clamp(0, K - 1), u.clamp(0, K - 1)
    off = (torch.arange(B, device=p_next.device) * K)[:, None]
    m = torch.zeros(B * K, dtype=torch.float32, device=p_next.device)
    m.index_add_(0, (l + off).view(-1), (p * (u.float() - b)).view(-1))
    m.index_add_(0, (u + off).view(-1), (p * (b - l.float())).view(-1))
    return m.view(B, K), a_star


def part1():
    dev = torch.device("cuda", torch.cuda.current_device())
    L = _lib.lib()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    for B, A in SHAPES:
        what = "B = %d, A = %d" % (B, A)
        g = torch.Generator(device=dev).manual_seed(B + A)
        p_next = torch.randn((B, A, K), device=dev, generator=g).softmax(-1).contiguous()
        p_select = torch.randn((B, A, K), device=dev, generator=g).softmax(-1).contiguous()
        ret = (torch.rand(B, device=dev, generator=g) * 12.0 - 6.0).contiguous()
        discount = torch.tensor([0.0, 0.95, 0.95 ** 3, 1.0], device=dev)[torch.randint(0, 4, (B,), device=dev, generator=g)].contiguous()
        cs = CategoricalSupport(A, atoms=K, vmin=VMIN, vmax=VMAX, device=dev)
        z = cs.z
        m, a_star, q_star = torch.empty((B, K), device=dev), torch.empty(B, dtype=torch.int8, device=dev), torch.empty(B, device=dev)
        q = torch.empty((B, A), device=dev)

        def project():
            _lib.check(L.snac_c51_project(B, A, K, VMIN, VMAX, vp(p_next), vp(p_select), vp(ret), vp(discount), vp(m), vp(a_star), vp(q_star), None, stream))

        def expect():
            _lib.check(L.snac_c51_expect(B, A, K, VMIN, VMAX, vp(p_select), vp(q), stream))
        project()
        m_t, a_t = torch_project(z, VMIN, VMAX, p_next, ret, discount, p_select)
        same = a_t == a_star.long()                                  # a float32 dot product may order two close values the other way
        if float(same.float().mean()) < 0.999 or float((m - m_t)[same].abs().max()) > 1e-5:
            raise SystemExit("the kernel and the composition disagree at %s" % what)
        rows = timed({"snac_c51_project": project, "torch composition of the projection": lambda: torch_project(z, VMIN, VMAX, p_next, ret, discount, p_select),
                      "snac_c51_expect": expect, "torch (p * z).sum(-1)": lambda: torch_expected(z, p_select)}, REPS[B])
        out.update({"%s, %s" % (k, what): v for k, v in rows.items()})
    return out


def part2():
    spec = importlib.util.spec_from_file_location("dqn_batched", os.path.join(ROOT, "examples", "dqn_batched.py"))
    dqn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dqn)
    dev = torch.device("cuda", torch.cuda.current_device())
    z = CategoricalSupport(5, atoms=K, vmin=0.0, vmax=100.0, device=dev).z

    def composition(p_next, ret, discount, p_select=None):
        return torch_project(z, 0.0, 100.0, p_next, ret, discount, p_select)[0]

    def per_tick(projection):
        wall = []
        for ticks in STEP_TICKS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dqn.run(envs=STEP_ENVS, ticks=ticks, batch=STEP_BATCH, distributional=True, prioritized=True, n_step=3, vmin=0.0, vmax=100.0,
                    projection=projection, log=lambda line: None)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        return 1e3 * (wall[1] - wall[0]) / (STEP_TICKS[1] - STEP_TICKS[0])
    calls = {"tick with CategoricalSupport.project": None, "tick with the torch composition": composition}
    for projection in calls.values():
        per_tick(projection)                                         # warm: allocator, kernels' code objects
    out = {k: [] for k in calls}
    for _ in range(GROUPS):
        for label, projection in calls.items():
            out[label].append(per_tick(projection))
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
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(_lib.CSRC, "k_dist.hip")]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=600).stderr
    for name, body in re.findall(r"Function Name: (\S+)(.*?)LDS Size", text, flags=re.S):
        kernel = re.search(r"k_c51_[a-z]+ILi\d", name)
        fields = dict(re.findall(r"remark: +(\w+)(?: \[[^\]]*\])?: (\d+)", body))
        print("    %-16s VGPRs %3s   scratch %s bytes/lane   occupancy %s waves/SIMD" % (
            kernel.group().replace("ILi", "<") + ">" if kernel else name, fields.get("VGPRs"), fields.get("ScratchSize"), fields.get("Occupancy")))


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
    print("  part 1: the projected target and the expected values, K = %d on [%g, %g]" % (K, VMIN, VMAX))
    med = show(child("part1"))
    for B, A in SHAPES:
        what = "B = %d, A = %d" % (B, A)
        moved = B * (4 * K * (A + 2) + 8 + 5)                        # p_select, the chosen row and m; ret, discount; a_star, q_star
        ms = med["snac_c51_project, " + what]
        print("    %s: composition / snac_c51_project %.2f; dot product / snac_c51_expect %.2f; the projection moves %.2f MB, %.1f GB/s" % (
            what, med["torch composition of the projection, " + what] / ms, med["torch (p * z).sum(-1), " + what] / med["snac_c51_expect, " + what],
            moved / 1e6, moved / ms / 1e6))
    print("  part 2: one tick of examples/dqn_batched.py --distributional --prioritized --n-step 3, wall ms")
    med = show(child("part2"))
    a, b = (med["%s, %d envs, batch %d" % (k, STEP_ENVS, STEP_BATCH)] for k in ("tick with the torch composition", "tick with CategoricalSupport.project"))
    print("    composition / CategoricalSupport.project  %.2f" % (a / b))


if __name__ == "__main__":
    main()
