"""GPU: the tie between tests/golden/dispatch_table.txt and the real launchers.  The table is produced on the host with stubs in the
launchers' place (tests/test_dispatch_host.py); here one real call per entry point, kind and N in {4, 256, 1024} must report, through
snac_last_kernel(), the kernel the table names for that call -- the sizes at which the arms differ: the tile kernels and k_step3dq
from 4 envs, the fast reset / AUX / k_iou / k_step1d forms from 256, 1024 below the 8-env blocks of k_rollout2dt.  Static classes,
float64 canonical rows, torch's allocations (aligned); the table's lines are for 400 plans, these envs have one: the dispatch asks only
whether they pass TB_MAX."""
import os
import re

import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

SIZES = (4, 256, 1024)


def _table():
    """{(entry, kind): [(first N, kernel), ...]} of the aligned, static, float64, canonical lines for whole groups of four envs."""
    ids, out = {}, {}
    with open(os.path.join(helpers.TESTS, "golden", "dispatch_table.txt")) as f:
        for line in f:
            m = re.match(r"(\S+) +([123])D sta f64 canonical obs0 plans0 grid0 P=400 +N%4=0 +\[(=?)(\d+)\] ?(.*)$", line)
            if not line.startswith("#"):
                lm = re.search(r"\[(\d+)\] (.*)$", line)
                if lm:
                    ids[lm.group(1)] = lm.group(2)
            if m:
                out[(m.group(1), int(m.group(2)))] = m.group(4)
    return {key: [(int(n), rest.split()[0]) for n, rest in (item.split(": ", 1) for item in ids[i].split("  |  "))] for key, i in out.items()}


def _expected(table, entry, kind, n):
    return [k for first, k in table[(entry, kind)] if first <= n][-1]


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_real_calls_run_on_the_kernels_of_the_golden_table(kind):
    from snac_amd import BatchedDMPEnv, _lib

    table, got, want = _table(), {}, {}
    for n in SIZES:
        env = BatchedDMPEnv(kind, False, n, seed=3)
        calls = [("reset", lambda: env.reset()), ("rollout/ALL", lambda: env.rollout(2)), ("step/obs", lambda: env.step(auto_reset=True)),
                 ("reset(m)", lambda: env.reset(mask=(torch.arange(n, device="cuda") % 3 == 0).to(torch.uint8))), ("observe", lambda: env.observe()),
                 ("iou", lambda: env.iou())]
        if n >= 8:
            m = n // 2
            src = torch.arange(m, device="cuda", dtype=torch.int32)
            calls.append(("trans/sd/obs", lambda: env.transition(torch.zeros(m, dtype=torch.int8, device="cuda"), None, src, src + m, t=0)))
        for entry, call in calls:
            call()
            size = n // 2 if entry.startswith("trans") else n         # (the table's batch size of a transition: its edges)
            got[(entry, n)] = _lib.lib().snac_last_kernel().decode()
            want[(entry, n)] = _expected(table, entry, kind, size)
        torch.cuda.synchronize()
    assert got == want
