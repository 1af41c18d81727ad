"""GPU: no node-pool kernel and no kernel with a flat output writes outside its outputs (tests/guard.py, as tests/test_gpu_footprint.py does
for the env-batch calls; default knobs, in this process).  Every output is carved from an arena with 64 KiB of 0xA5 on both sides, at a
512-byte boundary and one element past it (plan_out: 16 bytes past -- the header wants it 16-byte aligned); a node pool lies in the arena
itself, 128 bytes past a 512-byte boundary (the header wants records on 128).  After each call: the bytes inside the outputs equal the
reference's, arena.check(), and the pool's records outside the dst rows are what they were.

References: the CPU oracle for iou and the exported grid, numpy for obs_equal, torch's sum for the episodic sums; for every other call the
SAME call into plain torch tensors (a twin pool / ring / tree) -- those paths are pinned against the oracle by their own tests
(test_gpu_nodes2d.py, test_gpu_nodes1d3d.py, test_gpu_nodes_observe.py, test_gpu_nodes_eval.py, test_gpu_replay.py, test_gpu_prio.py)."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

import guard
import helpers

pytestmark = pytest.mark.gpu

EDGES = [1, 3, 4, 31, 32, 33, 63, 64, 65, 129]                         # edges / rows / leaves per call
POOL_ENVS = 132                                                        # the lower half of the pool: sources; the upper half: dst rows
_REPORT = []


def _note(entry, sizes, offsets, seconds):
    _REPORT.append(dict(entry=entry, n=sorted(set(sizes)), off=sorted(set(offsets))))
    d = os.environ.get("SNAC_FOOTPRINT_TABLE_DIR")
    line = "%-34s sizes %-44s offsets %-24s %.2f s" % (entry, " ".join(str(n) for n in sorted(set(sizes))), " ".join(str(o) for o in sorted(set(offsets))), seconds)
    print(line)
    if d:
        with open(os.path.join(d, "footprint_nodes.txt"), "a") as f:
            f.write(line + "\n")
        with open(os.path.join(d, "footprint_nodes.json"), "w") as f:
            json.dump(_REPORT, f)


def _same(got, want, what):
    assert got.cpu().numpy().tobytes() == (want.cpu().numpy() if hasattr(want, "cpu") else np.ascontiguousarray(want)).tobytes(), what


def _env(kind, dyn, n, f32, seed=3, with_oracle=False, ticks=9):
    import torch
    from snac_amd import BatchedDMPEnv

    table = helpers.plan_table(kind, dyn, ("sin_train" if kind == 1 else "dense_train") if dyn else "p0")[:16]
    shaped = table if kind == 1 else table.reshape(len(table), 26, 26)
    env = BatchedDMPEnv(kind, dyn, n, plans=shaped, seed=seed, total_step=12, obs_dtype=torch.float32 if f32 else torch.float64)
    env.reset()
    env.rollout(ticks, obs=None)                                       # states of every age, some of them terminal
    if not with_oracle:
        return env
    orc = helpers.oracle().OracleBatch(kind, dyn, n, table, seed=seed)
    orc.set_total_step(12)
    orc.reset()
    orc.rollout(ticks, obs=None)
    return env, orc


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_node_pool_edges_rows_and_leaves(kind, f32):
    """snac_transition_nodes*, snac_observe_nodes* and snac_evaluate_nodes* on a pool carved from the arena.  Reference: a twin pool in a
    plain torch tensor that takes the same calls."""
    import torch
    from snac_amd import NodePool, nodes

    t0 = time.time()
    env = _env(kind, True, POOL_ENVS, f32)
    rows = 2 * POOL_ENVS
    twin = NodePool(env, rows)
    twin.load(rows=torch.arange(rows) % POOL_ENVS, node_rows=torch.arange(rows))
    master = twin.records.clone()
    pool = NodePool(env, rows)
    rng = np.random.default_rng(kind)
    el = 4 if f32 else 8
    D, dt, dev = env.obs_dim, env.obs_dtype, env.device
    for m in EDGES:
        for off in (0, 1):                                             # the outputs: on a 512-byte boundary, and one element past it
            A = guard.Arena(rows * pool.WORDS * 4 + 3 * m * (D * el + 32) + 12 * (guard.BAND + 1024), dev)
            pool.records = A.carve((rows, pool.WORDS), torch.int32, offset=128, name="node records").copy_(master)
            assert pool.records.data_ptr() % 512 == 128
            twin.records.copy_(master)
            src = rng.integers(0, POOL_ENVS, m).astype(np.int32)
            dst = (POOL_ENVS + rng.permutation(POOL_ENVS)[:m]).astype(np.int32)
            acts = torch.from_numpy(rng.integers(0, env.num_actions, m).astype(np.int8)).to(dev)
            ks = torch.from_numpy(rng.integers(1, 4, m).astype(np.int8)).to(dev)
            # edges
            o = A.carve((m, D), dt, offset=off * el, name="obs")
            r = A.carve((m,), torch.float32, offset=off * 4, name="reward")
            d = A.carve((m,), torch.uint8, offset=off, name="done")
            with guard.allocations(nodes, [o, r, d]):
                go, gr, gd = pool.transition(acts, ks, src=src, dst=dst, t=m)
            assert go is o and gr is r and gd.data_ptr() == d.data_ptr()
            wo, wr, wd = twin.transition(acts, ks, src=src, dst=dst, t=m)
            _same(o, wo, "edge rows"), _same(r, wr, "edge rewards"), _same(d, wd.view(torch.uint8), "edge done flags")
            A.check()
            keep = torch.ones(rows, dtype=torch.bool, device=dev)
            keep[torch.from_numpy(dst).long().to(dev)] = False
            assert torch.equal(pool.records[keep], master[keep]), "records outside the dst rows"
            assert torch.equal(pool.records, twin.records)
            # rows of records: several i may name one record
            before = pool.records.clone()
            idx = rng.integers(0, rows, m).astype(np.int32)
            o2 = A.carve((m, D), dt, offset=off * el, name="observed rows")
            assert pool.observe(idx, out=o2) is o2
            _same(o2, twin.observe(idx), "observed rows")
            A.check()
            assert torch.equal(pool.records, before)
            # leaves
            est = A.carve((m,), torch.float64, offset=off * 8, name="estimate")
            steps = A.carve((m,), torch.int64, offset=off * 8, name="steps")
            with guard.allocations(nodes, [est, steps]):
                ge, gs = pool.evaluate(idx, 5, 0.9, t0=1)
            assert ge is est and gs is steps
            we, ws = twin.evaluate(idx, 5, 0.9, t0=1)
            _same(est, we, "estimates"), _same(steps, ws, "steps")
            A.check()
            assert torch.equal(pool.records, before)
    for entry in ("snac_transition_nodes%dd", "snac_observe_nodes%dd", "snac_evaluate_nodes%dd"):
        _note(entry % kind + (" f32" if f32 else " f64"), EDGES, ["+0", "+1 element"], (time.time() - t0) / 3)


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_flat_outputs_of_a_batch(kind):
    """iou and export_grid against the oracle, obs_equal against numpy, episodic sums against torch's sum of the per-env arrays (and the
    ticket of the scratch back at zero, as the header promises)."""
    import torch
    from snac_amd import _lib, batched

    t0 = time.time()
    sizes = (5, 252, 256, 257, 260)                                    # both sides of the 256-env threshold of k_iou
    for n in sizes:
        for off in (0, 1):
            env, orc = _env(kind, True, n, False, with_oracle=True, ticks=15)
            dev, sz = env.device, env.sizes
            A = guard.Arena(n * (8 + 1 + sz.env_height * sz.env_width * 8) + 256 * 8 + 12 * (guard.BAND + 1024), dev)
            out = A.carve((n,), torch.float64, offset=8 * off, name="iou")
            with guard.allocations(batched, [out]):
                assert env.iou() is out
            assert (_lib.lib().snac_last_kernel().decode() == "k_iou") == (n >= 256)
            _same(out, orc.iou(), "iou")
            A.check()
            mem = A.carve((n, sz.env_height, sz.env_width), torch.float64, offset=8 * off, name="exported grid")
            with guard.allocations(batched, [mem]):
                assert env.environment_memory() is mem
            assert np.array_equal(mem.cpu().numpy().reshape(n, -1), orc.state()["grid"])
            A.check()
            oa = env.observe()
            ob = oa.clone()
            ob[::3, -1] += 1.0
            eq = A.carve((n,), torch.uint8, offset=off, name="equal")
            with guard.allocations(batched, [eq]):
                got = env.obs_equal(oa, ob)
            assert got.data_ptr() == eq.data_ptr()
            _same(eq, (np.arange(n) % 3 != 0).astype(np.uint8), "obs_equal")
            A.check()
            out3 = A.carve((3,), torch.int64, offset=8 * off, name="out3")
            env._sums_scratch = A.carve((_lib.SUMS_SCRATCH_WORDS,), torch.int64, offset=8 * off, name="sums scratch").zero_()
            assert env.stats_tensor(out=out3) is out3
            _same(out3, env._stats.sum(dim=1), "episodic sums")
            assert int(out3[0]) > 0
            # the state the header promises: the ticket (the last word) is back at 0 -- the partials are stored, never added to, so they
            # may stay -- and the next call on the same scratch, without a fill, gives the same sums
            assert int(env._sums_scratch[-1]) == 0, "the ticket of snac_episodic_sums is 0 again after the call"
            again = A.carve((3,), torch.int64, offset=8 * off, name="out3 of the second call")
            assert env.stats_tensor(out=again) is again
            _same(again, out3, "episodic sums of a second call on the used scratch")
            assert int(env._sums_scratch[-1]) == 0
            A.check()
    _note("snac_iou %dD" % kind, sizes, ["+0", "+8"], 0)
    _note("snac_export_grid %dD" % kind, sizes, ["+0", "+8"], 0)
    _note("snac_obs_equal %dD" % kind, sizes, ["+0", "+1"], 0)
    _note("snac_episodic_sums %dD" % kind, sizes, ["+0", "+8"], time.time() - t0)


def test_discounted_return():
    """The same call into plain torch tensors is the reference (pinned by test_gpu_mcts.py / test_gpu_nodes_eval.py)."""
    import torch
    from snac_amd import _lib

    t0 = time.time()
    L, dev, H = _lib.lib(), torch.device("cuda", torch.cuda.current_device()), 6
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(1)
    for m in EDGES:
        for off in (0, 1):
            reward = torch.rand((H, m), generator=g).to(dev)
            done = (torch.rand((H, m), generator=g) < 0.2).to(torch.uint8).to(dev)
            term = (torch.rand((m,), generator=g) < 0.2).to(torch.uint8).to(dev)
            gpow = torch.tensor([0.9 ** t for t in range(H)], dtype=torch.float64).to(dev)
            first = torch.rand((m,), generator=g, dtype=torch.float64).to(dev)
            A = guard.Arena(16 * m + 4 * (guard.BAND + 1024), dev)
            est = A.carve((m,), torch.float64, offset=8 * off, name="est").copy_(first)
            steps = A.carve((m,), torch.int64, offset=8 * off, name="steps")
            west, wsteps = first.clone(), torch.empty(m, dtype=torch.int64, device=dev)
            _lib.check(L.snac_discounted_return(H, m, vp(reward), vp(done), vp(term), vp(gpow), vp(est), vp(steps), stream))
            _lib.check(L.snac_discounted_return(H, m, vp(reward), vp(done), vp(term), vp(gpow), vp(west), vp(wsteps), stream))
            _same(est, west, "estimates"), _same(steps, wsteps, "steps")
            A.check()
    _note("snac_discounted_return", EDGES, ["+0", "+8"], time.time() - t0)


@pytest.mark.parametrize("layout", ["ticks", "tiled"])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_replay_gather(kind, layout):
    """snac_replay_gather / snac_replay_gather_tiled: s_out, s_next_out one element past a 512-byte boundary too, plan_out 16 bytes past.
    Reference: the same gather of the same ring into plain torch tensors (pinned by test_gpu_replay.py)."""
    import torch
    from snac_amd import ReplayRing, replay

    t0 = time.time()
    batches = (1, 3, 4, 5, 64, 67)
    for f32 in (False, True):
        env = _env(kind, True, 67, f32, ticks=3)
        ring = ReplayRing(env, 8, layout=layout)
        ring.collect(6)
        rng = np.random.default_rng(kind)
        slots = ring.slots().cpu().numpy()
        for B in batches:
            for off in (0, 1):
                slot, idx = rng.choice(slots, B).astype(np.int32), rng.integers(0, 67, B).astype(np.int32)
                A = guard.Arena(B * (2 * env.obs_dim + ring.plan_cells) * 4 + 6 * (guard.BAND + 1024), env.device)
                s = A.carve((B, env.obs_dim), torch.float32, offset=4 * off, name="s_out")
                s_next = A.carve((B, env.obs_dim), torch.float32, offset=4 * off, name="s_next_out")
                plan = A.carve((B, ring.plan_cells), torch.float32, offset=16 * off, name="plan_out")
                with guard.allocations(replay, [s, s_next, plan]):
                    got = ring.gather(slot, idx)
                assert got["s"] is s and got["s_next"] is s_next and got["plan"].data_ptr() == plan.data_ptr()
                want = ring.gather(slot, idx)
                _same(s, want["s"], "s"), _same(s_next, want["s_next"], "s_next"), _same(plan, want["plan"], "plan")
                A.check()
    _note("snac_replay_gather%s %dD" % ("_tiled" if layout == "tiled" else "", kind), batches, ["s +0 / +4", "plan +0 / +16"], time.time() - t0)


def test_prio_sample():
    """snac_prio_sample: index and prob.  Reference: a twin tree with the same seed, updates and draw counter, sampled into plain tensors."""
    import torch
    from snac_amd import priority

    t0 = time.time()
    dev = torch.device("cuda", torch.cuda.current_device())
    trees = [priority.PriorityTree(1000, dev, seed=3, sampler_id=5) for _ in range(2)]
    g = torch.Generator().manual_seed(2)
    index, pri = torch.randperm(1000, generator=g)[:300].to(torch.int32).to(dev), torch.rand(300, generator=g).to(dev)
    for t in trees:
        t.update(index, pri)
    sizes = (1, 63, 64, 65)
    for n in sizes:
        for stratified in (True, False):
            for off in (0, 1):
                A = guard.Arena(8 * n + 4 * (guard.BAND + 1024), dev)
                idx = A.carve((n,), torch.int32, offset=4 * off, name="index")
                prob = A.carve((n,), torch.float32, offset=4 * off, name="prob")
                with guard.allocations(priority, [idx, prob]):
                    gi, gp = trees[0].sample(n, stratified=stratified)
                assert gp is prob
                wi, wp = trees[1].sample(n, stratified=stratified)
                assert torch.equal(idx.long(), wi) and torch.equal(gi, wi)
                _same(prob, wp, "prob")
                assert bool((wi >= 0).all())
                A.check()
    _note("snac_prio_sample", sizes, ["+0", "+4"], time.time() - t0)
