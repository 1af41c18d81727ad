"""GPU: the two ends of a k_rollout2d launch and its tile order.  The launch loads its state in two trips (header, episode counter, the
env's three episodic sums and the grid words together, then the plan rows) and leaves by stores alone: an env that finished episodes
gets sums-as-loaded + its own, every other env's sums are not written.  SNAC_2D_STAGE_XCD picks which block of 256 envs a workgroup
takes (0: launch order; 1: a contiguous eighth of the env range per XCD with a grid padded to a multiple of 8; the default 2 is one or
the other by batch size, so both are run here).

The knobs are read once per process, so the cases run in a child pytest with SNAC_2D_BLOCK=0 SNAC_2D_TP=0 SNAC_2D_STAGE_MIN=4 (every
2D rollout of whole groups of four envs on k_rollout2d), once per tile order.  Batches: 4 envs (one ragged tile), 64 (one full tile),
68 (two tiles, one block), 2048 (8 blocks: one per XCD label), 2340 (10 blocks: a grid of 16 with empty blocks, a ragged last tile),
4352 (17 blocks).  Time limit 5 and launches of 1, 2 and 7 ticks in turn: in the 1-tick launches (nearly) no env finishes anything, in
the 7-tick launches every env does.  Against the CPU oracle: rows, rewards, done flags, the PER-ENV sums element for element,
episodic_stats(), iou(); against a twin on the tile kernel (an output that is not 16-byte aligned selects it): headers, grids, sums."""
import os
import subprocess
import sys

import numpy as np
import pytest

from devmem import _kernel
import helpers

pytestmark = pytest.mark.gpu

INNER = os.environ.get("SNAC_TEST_ENDS2D_INNER") == "1"
inner = pytest.mark.skipif(not INNER, reason="runs in the child processes of test_both_tile_orders_in_child_processes")
SIZES = [4, 64, 68, 2048, 2304 + 36, 4352]
LAUNCHES = (1, 2, 7, 1, 2, 7)


def _pair(dyn, n, f32, seed=5, kw=None):
    import torch
    from snac_amd import BatchedDMPEnv

    kw = kw or {}
    table = helpers.plan_table(2, dyn, "dense_train" if dyn else "p0")
    env = BatchedDMPEnv(2, dyn, n, plans=table.reshape(len(table), 26, 26), seed=seed, env_id_base=7, total_step=5,
                        obs_dtype=torch.float32 if f32 else torch.float64, **kw)
    orc = helpers.oracle().OracleBatch(2, dyn, n, table, seed=seed, env_id_base=7)
    orc.set_total_step(5)
    if kw:
        norm = {None: dyn, "raw": False, "norm": True}[env.obs_scalars]
        orc.configure(obs_norm=norm, frame=env.frame_value, tail=env.obs_tail)
        assert orc.obs_dim == env.obs_dim
    o = orc.reset()
    assert env.reset().cpu().numpy().tobytes() == (o.astype(np.float32) if f32 else o).tobytes()
    return env, orc


def _per_env_sums(env, orc):
    s = orc.stats()
    got = env._stats.cpu().numpy()
    assert np.array_equal(got[0], s["episodes"].astype(np.int64)), "per-env episode counts"
    assert np.array_equal(got[1], s["ret"].astype(np.int64)), "per-env return sums"
    assert np.array_equal(got[2], s["iou_fx"].astype(np.int64)), "per-env IoU sums"
    e = env.episodic_stats()
    assert (e["episodes"], e["return_sum"], e["iou_fx_sum"]) == (int(s["episodes"].sum()), int(s["ret"].sum()), int(s["iou_fx"].sum()))


def _run(dyn, n, f32, kw=None, explicit=False):
    import torch

    env, orc = _pair(dyn, n, f32, kw=kw)
    twin = env.fork(torch.arange(n, device=env.device))
    D = env.obs_dim
    rng = np.random.default_rng(n)
    t0 = 0
    for T in LAUNCHES:
        acts = rng.integers(0, 5, size=(T, n)).astype(np.int8) if explicit else None
        ks = rng.integers(1, 4, size=(T, n)).astype(np.int8) if explicit else None
        ta = None if acts is None else torch.from_numpy(acts).to(env.device)
        tk = None if ks is None else torch.from_numpy(ks).to(env.device)
        before = env._stats.clone()
        og, rg, dg = env.rollout(T, actions=ta, step_size=tk)
        assert _kernel() == "k_rollout2d"
        oc, rc, dc = orc.rollout(T, t0=t0, actions=acts, step_size=ks)
        assert og.cpu().numpy().tobytes() == (oc.astype(np.float32) if f32 else oc).tobytes(), "observations"
        assert rg.cpu().numpy().tobytes() == rc.tobytes(), "rewards"
        assert np.array_equal(dg.cpu().numpy().view(np.uint8), dc), "done flags"
        _per_env_sums(env, orc)
        finished = torch.from_numpy(dc.astype(bool).any(axis=0)).to(env.device)
        assert torch.equal(env._stats[:, ~finished], before[:, ~finished])      # an env that finished nothing keeps its sums as they were
        if T == 1:
            assert int(finished.sum()) * 2 < n                       # most envs finish nothing in a launch of one tick
        if T == 7:
            assert bool(finished.all())
        raw = torch.empty(T * n * D + 1, dtype=env.obs_dtype, device=env.device)
        ob, rb, db = twin.rollout(T, out=raw[1:].view(T, n, D), actions=ta, step_size=tk)
        assert ob.data_ptr() % 16 != 0 and _kernel() == "k_rollout"
        assert torch.equal(og, ob) and torch.equal(rg, rb) and torch.equal(dg, db)
        t0 += T
    assert env.iou().cpu().numpy().tobytes() == orc.iou().tobytes()
    assert torch.equal(env._hdr, twin._hdr) and torch.equal(env._grid, twin._grid) and torch.equal(env._stats, twin._stats)
    assert torch.equal(env._episode, twin._episode)


@inner
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("dyn", [False, True], ids=["sta", "dyn"])
@pytest.mark.parametrize("n", SIZES)
def test_inner_ends_of_a_launch(n, dyn, f32):
    _run(dyn, n, f32)


@inner
@pytest.mark.parametrize("n", [68, 2304 + 36])
def test_inner_explicit_actions_and_step_sizes(n):
    _run(True, n, False, explicit=True)


@inner
@pytest.mark.parametrize("n", [68, 2304 + 36])
def test_inner_rows_with_the_record_tail(n):
    _run(True, n, False, kw=dict(obs_tail=("record",)))


@inner
def test_inner_the_knob_is_what_the_child_was_given():
    from snac_amd import _lib

    t = _lib.tuning()
    assert t["SNAC_2D_STAGE_XCD"][0] == int(os.environ["SNAC_2D_STAGE_XCD"]) and t["SNAC_2D_STAGE_MIN"][0] == 4


@pytest.mark.parametrize("xcd", [0, 1])
def test_both_tile_orders_in_child_processes(xcd):
    if INNER:
        pytest.skip("the child itself")
    env = dict(os.environ, SNAC_TEST_ENDS2D_INNER="1", SNAC_2D_BLOCK="0", SNAC_2D_TP="0", SNAC_2D_STAGE_MIN="4", SNAC_2D_STAGE_XCD=str(xcd))
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "inner", "-p", "no:cacheprovider"],
                         cwd=helpers.ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "skipped" not in out.stdout.splitlines()[-1], out.stdout[-500:]
