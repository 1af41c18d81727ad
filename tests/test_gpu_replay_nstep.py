"""GPU: ReplayRing.gather_nstep / gather_windows (snac_replay_gather_nstep / snac_replay_gather_windows) and the sampling calls on them.

Constructed rings: a small real ReplayRing whose arrays are overwritten with the generated contents of tests/test_replay_nstep_host.py
(make_ring), compared byte for byte with the numpy rules of that file for EVERY addressable (slot, env), over both layouts, both ring
dtypes, the three kinds, rings that wrapped and rings not yet full, ragged batches, with and without plan_out, and the position tail.  That
the rings meet each stop of both walks is asserted there, on the host.

Real data: 3D dynamic envs through a wrapped ring; the reference is the EXISTING gather() -- five calls composed in numpy for the 5-step
transition, the flattened steps for the windows.  Then the sampling calls against the gathers of their own slot / env, the footprint of
both entry points (tests/guard.py), and the example with --n-step."""
import importlib.util
import os

import numpy as np
import pytest

from devmem import short_env
import guard
import helpers
from test_replay_nstep_host import FILLS, GAMMA, LENGTHS, NSTEPS, addressable, make_ring, nstep_rule, ring_seed, window_rule

pytestmark = pytest.mark.gpu

NSTEP_KEYS = ("s", "s_next", "action", "return", "discount", "done", "steps")
WINDOW_KEYS = ("s", "s_next", "action", "reward", "done", "mask", "length")


def constructed_ring(env, cells, layout, cap, head, ticks, seed):
    """A real ring with generated contents, and the same contents for the numpy rules."""
    import torch
    from snac_amd import ReplayRing

    reset = env.observe()[0].float().cpu().numpy()                   # the envs were just reset: the reset observation
    ring = ReplayRing(env, cap, layout=layout)
    R = make_ring(np.random.default_rng(seed), cap, env.num_envs, env.obs_dim, head, ticks, np.float32 if env.obs_dtype == torch.float32 else np.float64)
    R["reset"], R["plans"] = reset, cells
    for slot in range(cap):
        ring._put(slot, torch.from_numpy(R["obs"][slot]).to(env.device))
    for name in ("reward", "done", "first", "action", "plan_idx"):
        getattr(ring, name).copy_(torch.from_numpy(R[name]))
    ring.head, ring.ticks = head, ticks
    return ring, R


def stack_rows(rows, keys):
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in keys}


def equal_gather(got, want, keys, what):
    for k in keys:
        g = got[k].cpu().numpy()
        g = g.reshape(len(g), -1) if k == "plan" else g
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, want[k].dtype, g.shape, want[k].shape)
        assert g.tobytes() == want[k].tobytes(), (what, k)


def _check_ring(ring, R, rng):
    """Every addressable entry at once (with the plan), then batches of 1, 5 and 67 drawn from them, with and without the plan."""
    pairs = addressable(R)
    assert len(pairs) == len(ring)
    slot, env = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    cap = ring.cap
    for n in NSTEPS(cap):
        rows = [nstep_rule(R, t, i, n, GAMMA) for t, i in pairs]
        equal_gather(ring.gather_nstep(slot, env, n, GAMMA), stack_rows(rows, NSTEP_KEYS + ("plan",)), NSTEP_KEYS + ("plan",), "n = %d" % n)
        for B, with_plan in ((1, False), (5, True), (67, False)):
            pick = rng.integers(0, len(pairs), B)
            got = ring.gather_nstep(slot[pick], env[pick], n, GAMMA, with_plan=with_plan)
            keys = NSTEP_KEYS + (("plan",) if with_plan else ())
            assert ("plan" in got) == with_plan
            equal_gather(got, stack_rows([rows[j] for j in pick], keys), keys, "n = %d, batch %d" % (n, B))
    for L in LENGTHS:
        rows = [window_rule(R, t, i, L) for t, i in pairs]
        equal_gather(ring.gather_windows(slot, env, L), stack_rows(rows, WINDOW_KEYS + ("plan",)), WINDOW_KEYS + ("plan",), "L = %d" % L)
        for B, with_plan in ((1, True), (5, False), (67, True)):
            pick = rng.integers(0, len(pairs), B)
            got = ring.gather_windows(slot[pick], env[pick], L, with_plan=with_plan)
            keys = WINDOW_KEYS + (("plan",) if with_plan else ())
            assert ("plan" in got) == with_plan
            equal_gather(got, stack_rows([rows[j] for j in pick], keys), keys, "L = %d, batch %d" % (L, B))


@pytest.mark.parametrize("N,layout", [(5, "ticks"), (70, "ticks"), (70, "tiled")])
@pytest.mark.parametrize("f32", [False, True], ids=["f64ring", "f32ring"])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_constructed_rings_equal_the_numpy_rules_at_every_addressable_entry(kind, f32, N, layout):
    env, cells = short_env(kind, N, f32)
    rng = np.random.default_rng(kind)
    for cap, head, ticks in FILLS:
        ring, R = constructed_ring(env, cells, layout, cap, head, ticks, ring_seed(kind, f32, N, cap, head))
        _check_ring(ring, R, rng)


@pytest.mark.parametrize("kind,layout", [(1, "ticks"), (2, "tiled")])
def test_constructed_rings_with_the_position_tail(kind, layout):
    env, cells = short_env(kind, 70, False, obs_tail=("position",))
    assert env.obs_dim == (8 if kind == 1 else 53)
    ring, R = constructed_ring(env, cells, layout, 7, 3, 10, 41 + kind)
    assert R["reset"][-1] == (2.0 if kind == 1 else 3.0)             # the tail of the reset observation: the start position
    _check_ring(ring, R, np.random.default_rng(9))


# ---- real data against the existing gather ------------------------------------------------------------------------------------------
def _real_ring(layout, prioritized=False):
    from snac_amd import BatchedDMPEnv, ReplayRing

    table = helpers.plan_table(3, True, "dense_train")
    env = BatchedDMPEnv(3, True, 64, plans=table.reshape(len(table), 26, 26), seed=12)
    env.reset()
    ring = ReplayRing(env, 96, layout=layout, prioritized=prioritized)
    ring.collect(96)
    ring.collect(40)                                                 # wrapped: head = 40, 95 addressable slots
    return ring


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.mark.parametrize("layout", ["ticks", "tiled"])
def test_real_data_equals_compositions_of_the_existing_gather(layout):
    import torch

    ring = _real_ring(layout)
    cap, N, n, L, gamma = 96, 64, 5, 8, 0.97
    assert ring.valid_ticks() == 95 and ring.head == 40
    slot = ring.slots().cpu().numpy().repeat(N)
    env = np.tile(np.arange(N), 95)
    B = len(slot)
    newest, oldest = (ring.head - 1) % cap, (ring.head - 95) % cap
    first, done = ring.first.cpu().numpy(), ring.done.cpu().numpy()
    # n-step: five gather() calls, put together in numpy
    steps = [_np(ring.gather((slot + k) % cap, env, with_plan=k == 0)) for k in range(n)]
    m, alive = np.zeros(B, np.int32), np.ones(B, bool)
    by_done, by_newest = np.zeros(B, bool), np.zeros(B, bool)
    for k in range(n):
        sk = (slot + k) % cap
        stop = steps[k]["done"] | (k + 1 == n) | (sk == newest) | (first[(sk + 1) % cap, env] != 0)
        m[alive & stop] = k + 1
        by_done |= alive & steps[k]["done"] & (k + 1 < n)
        by_newest |= alive & ~steps[k]["done"] & (sk == newest) & (k + 1 < n)
        alive &= ~stop
    assert not alive.any() and m.min() >= 1
    g, d = np.zeros(B, np.float64), np.ones(B, np.float64)
    for k in range(n - 1, -1, -1):
        g = np.where(k < m, steps[k]["reward"].astype(np.float64) + np.float64(gamma) * g, g)
        d = np.where(k < m, d * np.float64(gamma), d)
    last = {key: np.stack([steps[k][key] for k in range(n)])[m - 1, np.arange(B)] for key in ("s_next", "done")}
    want = {"s": steps[0]["s"], "action": steps[0]["action"], "plan": steps[0]["plan"].reshape(B, -1), "s_next": last["s_next"], "done": last["done"],
            "steps": m, "return": g.astype(np.float32), "discount": np.where(last["done"], 0.0, d).astype(np.float32)}
    equal_gather(ring.gather_nstep(slot, env, n, gamma), want, NSTEP_KEYS + ("plan",), "5-step")
    # the conditions of this setup (from the CPU oracle: 16.9 % and 3.3 %)
    assert by_done.mean() >= 0.05 and by_newest.mean() >= 0.01, (by_done.mean(), by_newest.mean())
    # windows: gather() of the flattened steps, zeros and the mask outside
    length = np.ones(B, np.int32)
    for it in range(L - 1):
        e = (slot - length + 1) % cap                                 # the earliest step; a window that stopped (length < it + 1) stays
        grow = (length == it + 1) & (e != oldest) & (first[e, env] == 0) & (done[(e - 1) % cap, env] == 0)
        length += grow
    j = np.arange(L)[None, :]
    inside = j < length[:, None]
    wslot = np.where(inside, slot[:, None] - length[:, None] + 1 + j, slot[:, None]) % cap
    flat = _np(ring.gather(wslot.reshape(-1), np.repeat(env, L), with_plan=False))
    wwant = {k: np.where(inside.reshape(B, L, *([1] * (v.ndim - 1))), v.reshape(B, L, *v.shape[1:]), np.zeros((), v.dtype)) for k, v in flat.items()}
    wwant.update(mask=inside, length=length, plan=steps[0]["plan"].reshape(B, -1))
    got = ring.gather_windows(slot, env, L)
    equal_gather(got, wwant, WINDOW_KEYS + ("plan",), "windows")
    assert (length < L).mean() >= 0.10, (length < L).mean()           # about a third
    assert torch.equal(got["s"][:, 1:][got["mask"][:, 1:]], got["s_next"][:, :-1][got["mask"][:, 1:]])   # consecutive tuples chain


# ---- sampling -----------------------------------------------------------------------------------------------------------------------
def _same_dicts(a, b, keys):
    import torch

    for k in keys:
        assert torch.equal(a[k], b[k]), k


def test_sampling_returns_the_gathers_of_its_own_slots():
    import torch

    ring = _real_ring("ticks", prioritized=True)
    dev = ring.env.device
    nkeys, wkeys = NSTEP_KEYS + ("plan",), WINDOW_KEYS + ("plan",)
    for how in (dict(generator=torch.Generator(device=dev).manual_seed(4)), dict(prioritized=True, beta=0.5)):
        out = ring.sample(200, n_step=3, gamma=0.9, **how)
        assert set(nkeys) | {"slot", "env"} <= set(out) and "reward" not in out and out["s"].shape == (200, 51)
        assert ("index" in out and "prob" in out and "weight" in out) == ("prioritized" in how)
        _same_dicts(out, ring.gather_nstep(out["slot"], out["env"], 3, 0.9), nkeys)
        assert int(out["steps"].min()) >= 1 and int(out["steps"].max()) == 3
        win = ring.sample_windows(200, 6, **how)
        assert win["s"].shape == (200, 6, 51) and win["mask"].shape == (200, 6) and win["length"].shape == (200,) and win["plan"].shape == (200, 20, 20)
        assert ("index" in win and "prob" in win and "weight" in win) == ("prioritized" in how)
        _same_dicts(win, ring.gather_windows(win["slot"], win["env"], 6), wkeys)
        assert bool(((win["slot"] - (ring.head - 95)) % 96 < 95).all())      # only addressable ends
        if "prioritized" in how:
            assert torch.equal(out["index"], out["slot"] * 64 + out["env"]) and torch.equal(win["index"], win["slot"] * 64 + win["env"])
    plain = ring.sample_windows(50, 4, generator=torch.Generator(device=dev).manual_seed(4), with_plan=False)
    assert "plan" not in plain


def test_the_default_sample_is_what_it_was():
    """sample(batch) without n_step: the draw and the gather of before, restated here."""
    import torch

    ring = _real_ring("ticks")
    dev = ring.env.device
    g = torch.Generator(device=dev).manual_seed(7)
    out = ring.sample(300, generator=g)
    g = torch.Generator(device=dev).manual_seed(7)
    age = torch.randint(0, ring.valid_ticks(), (300,), device=dev, generator=g)
    slot = (ring.head - 1 - age) % ring.cap
    env = torch.randint(0, 64, (300,), device=dev, generator=g)
    want = ring.gather(slot, env)
    assert set(out) == set(want) == {"s", "s_next", "action", "reward", "done", "plan"}
    _same_dicts(out, want, want.keys())


# ---- footprint ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ticks", "tiled"])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_neither_entry_point_writes_outside_its_outputs(kind, layout):
    """Every output of both entry points carved from an arena, on a 512-byte boundary and one element past it (plan_out: 16 bytes past);
    ragged batches.  Reference: the same call into plain torch tensors (pinned above)."""
    import torch
    from snac_amd import ReplayRing, replay

    n, L = 3, 5
    for f32 in (False, True):
        env, _ = short_env(kind, 67, f32)
        env.rollout(3, obs=None)
        ring = ReplayRing(env, 8, layout=layout)
        ring.collect(6)
        rng = np.random.default_rng(kind)
        slots = ring.slots().cpu().numpy()
        D, PC, dev = env.obs_dim, ring.plan_cells, env.device
        for B in (1, 3, 4, 5, 64, 67):
            for off in (0, 1):
                slot, idx = rng.choice(slots, B).astype(np.int32), rng.integers(0, 67, B).astype(np.int32)
                A = guard.Arena(B * ((2 * D + 6) * 4 * (L + 1) + 2 * PC * 4 + 64) + 20 * (guard.BAND + 1024), dev)
                outs = [A.carve((B, D), torch.float32, offset=4 * off, name="s_out"), A.carve((B, D), torch.float32, offset=4 * off, name="s_next_out"),
                        A.carve((B, PC), torch.float32, offset=16 * off, name="plan_out"), A.carve((B,), torch.int64, offset=8 * off, name="action_out"),
                        A.carve((B,), torch.float32, offset=4 * off, name="return_out"), A.carve((B,), torch.float32, offset=4 * off, name="discount_out"),
                        A.carve((B,), torch.bool, offset=off, name="done_out"), A.carve((B,), torch.int32, offset=4 * off, name="steps_out")]
                with guard.allocations(replay, outs):
                    got = ring.gather_nstep(slot, idx, n, GAMMA)
                assert got["s"] is outs[0] and got["return"] is outs[4] and got["steps"] is outs[7] and got["plan"].data_ptr() == outs[2].data_ptr()
                _same_dicts(got, ring.gather_nstep(slot, idx, n, GAMMA), NSTEP_KEYS + ("plan",))
                A.check()
                outs = [A.carve((B, L, D), torch.float32, offset=4 * off, name="s_out"), A.carve((B, L, D), torch.float32, offset=4 * off, name="s_next_out"),
                        A.carve((B, PC), torch.float32, offset=16 * off, name="plan_out"), A.carve((B, L), torch.int64, offset=8 * off, name="action_out"),
                        A.carve((B, L), torch.float32, offset=4 * off, name="reward_out"), A.carve((B, L), torch.bool, offset=off, name="done_out"),
                        A.carve((B, L), torch.bool, offset=off, name="mask_out"), A.carve((B,), torch.int32, offset=4 * off, name="length_out")]
                with guard.allocations(replay, outs):
                    got = ring.gather_windows(slot, idx, L)
                assert got["s"] is outs[0] and got["mask"] is outs[6] and got["length"] is outs[7] and got["plan"].data_ptr() == outs[2].data_ptr()
                _same_dicts(got, ring.gather_windows(slot, idx, L), WINDOW_KEYS + ("plan",))
                A.check()


# ---- the example --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prioritized", [False, True], ids=["uniform", "prioritized"])
def test_the_dqn_example_runs_with_n_step_targets(prioritized):
    spec = importlib.util.spec_from_file_location("dqn_batched", os.path.join(helpers.ROOT, "examples", "dqn_batched.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses, _ = mod.run(envs=256, ticks=20, batch=128, prefill=16, n_step=3, log=lambda line: None, prioritized=prioritized)
    assert len(losses) == 20 and all(np.isfinite(losses))
