"""CPU: the dispatch of the env-batch entry points, pinned as a table.  tests/native/dispatch_table.cpp is built by
`hipcc --offload-host-only` together with snac_amd/csrc/snac_hip.hip as it is, with stubs for every launch function, and calls the real
C ABI over a grid of batch sizes round every threshold, for every kind, row type, layout, alignment and observation mode; one process
per set of knob overrides (the library reads its environment once).  Every run's output must have the sha256 that
tests/golden/dispatch_overrides.sha256 holds for its override set ("none": the full table, 6390 lines).  Of the full table the part a
person reads is committed as text, tests/golden/dispatch_table.txt, and must be equal byte for byte: the header, every line that
carries a list of changes (each distinct list is printed once) and the lines of the static float64 canonical aligned calls; the
other lines only say which list they share ([=id]) and are held by the digest.  The goldens were produced from the
library BEFORE choose() existed (the cascade in launch() and the knob reads in the launchers; profiles/dispatch_refactor.txt): a changed
comparison or a dropped condition shows here, without a GPU.  After a deliberate retune: `python tests/test_dispatch_host.py regenerate`."""
import hashlib
import os
import subprocess
import sys

import helpers

GOLDEN = os.path.join(helpers.TESTS, "golden")
TABLE, DIGESTS = os.path.join(GOLDEN, "dispatch_table.txt"), os.path.join(GOLDEN, "dispatch_overrides.sha256")
CSRC = os.path.join(helpers.ROOT, "snac_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# every 0/1 switch of the env dispatch flipped on its own
SWITCHES = ["SNAC_3D_BLOCK", "SNAC_2D_STAGE", "SNAC_2D_TP", "SNAC_1D_TP", "SNAC_STEP_STAGE", "SNAC_STEP3D_SPAN", "SNAC_EDGES3D", "SNAC_EDGES2D", "SNAC_3D_BLOCK_VAR",
            "SNAC_2D_BLOCK", "SNAC_STEP3D_QUARTER", "SNAC_1D_LANE", "SNAC_STEP1D", "SNAC_EDGES1D", "SNAC_RESET_FAST", "SNAC_IOU_FAST", "SNAC_AUX_STEP"]
# the override sets, one process each; the first (none) is the full table, the others run the reduced layout and alignment set
OVERRIDES = ([{}, {"SNAC_3D_PIPELINE": 0}] + [{s: 0} for s in SWITCHES] + [{"SNAC_1D_LANE_NT": 1}, {"SNAC_STEP3D_QUARTER": 0, "SNAC_STEP3D_SPAN": 0}] +
             [{"SNAC_TILE": e} for e in (8, 16, 32, 64)] +
             # each umbrella override at a value inside the grid
             [{"SNAC_3D_BLOCK_MIN": 1024}, {"SNAC_2D_STAGE_MIN": 8192}, {"SNAC_2D_TP_MAX": 4096}, {"SNAC_2D_TP_VAR_MAX": 12288}, {"SNAC_1D_TP_MAX": 16384},
              {"SNAC_STEP_VAR_MIN": 2048}] +
             [{"SNAC_STEP_VAR_HALF": v} for v in (0, 1)] +
             [{k: v} for k in ("SNAC_STEP2D_FORM", "SNAC_STEP3D_FORM", "SNAC_STEP1D_FORM") for v in (0, 1, 2, 3)] +
             [{"SNAC_T2D_E": e} for e in (16, 32, 64)])


def label(ov):
    return " ".join("%s=%d" % kv for kv in sorted(ov.items())) or "none"


def build(out_dir):
    exe = os.path.join(str(out_dir), "dispatch_table")
    cmd = [HIPCC, "--offload-host-only", "-O1", "-std=c++17", "-fno-strict-aliasing", "-I", CSRC, "-I", os.path.join(helpers.ROOT, "include"),
           "-x", "hip", os.path.join(helpers.TESTS, "native", "dispatch_table.cpp"), os.path.join(CSRC, "snac_hip.hip"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def run(exe, ov):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SNAC_")}
    env.update({k: str(v) for k, v in ov.items()})
    r = subprocess.run([exe] + (["reduced"] if ov else []), capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, (label(ov), r.stderr[-3000:])
    return r.stdout


def excerpt(out):
    """The committed part of the full table: comments, the lines that define a list, the static float64 canonical aligned calls."""
    return b"".join(line for line in out.splitlines(True)
                    if line.startswith(b"#") or b"[=" not in line or b" sta f64 canonical obs0 plans0 grid0 P=400 " in line)


def regenerate(exe):
    """Rewrite both goldens from the program `exe` (after a deliberate retune: from the library as it is)."""
    with open(TABLE, "wb") as f:
        f.write(excerpt(run(exe, {})))
    with open(DIGESTS, "w") as f:
        for ov in OVERRIDES:
            f.write("%s  %s\n" % (hashlib.sha256(run(exe, ov)).hexdigest(), label(ov)))


def test_dispatch_equals_the_golden_table_under_every_override_set(tmp_path):
    exe = build(tmp_path)
    with open(DIGESTS) as f:
        want = {lab: dig for dig, lab in (line.rstrip("\n").split("  ", 1) for line in f)}
    assert sorted(want) == sorted(label(ov) for ov in OVERRIDES)
    with open(TABLE, "rb") as f:
        golden = f.read()
    bad = []
    for ov in OVERRIDES:
        out = run(exe, ov)
        if hashlib.sha256(out).hexdigest() == want[label(ov)] and (ov or excerpt(out) == golden):
            continue
        path = tmp_path / ("dispatch_table_%s.txt" % label(ov).replace(" ", "_"))
        path.write_bytes(out)                                        # left behind for a diff (excerpt() of the no-override one against the golden)
        bad.append("%s: %s" % (label(ov), path))
    assert not bad, "the dispatch differs from tests/golden under these overrides (produced tables): " + "; ".join(bad)


if __name__ == "__main__":
    import tempfile

    assert sys.argv[1:] == ["regenerate"], "usage: python tests/test_dispatch_host.py regenerate"
    with tempfile.TemporaryDirectory() as tmp:
        regenerate(build(tmp))
