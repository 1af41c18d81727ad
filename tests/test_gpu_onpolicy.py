"""GPU: snac_gae, snac_replay_gather_onpolicy and RolloutBuffer (snac_amd/onpolicy.py).

snac_gae through the C ABI on the generated spans of tests/test_onpolicy_host.py (make_span; that they contain every case that can go
wrong is asserted there, on the host), byte for byte against gae_rule, with adv and ret carved from a guard arena: slots outside the span
keep their bytes and nothing lands outside the two arrays.  The gather on constructed rings as tests/test_gpu_replay_nstep.py builds them:
s and plan byte for byte against the EXISTING ReplayRing.gather() of the same pairs, everything against onpolicy_rule with the downloaded
norm pair.  Then its footprint (tests/guard.py), RolloutBuffer on real envs whose episodes end inside the span and whose ring wraps, and
the PPO example."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from devmem import _vp, short_env
import guard
import helpers
from test_gpu_replay_nstep import constructed_ring, equal_gather, stack_rows
from test_onpolicy_host import GAMMA, LAM, SIZES, gae_rule, make_span, onpolicy_rule, span_cases, span_seed, span_slots
from test_replay_nstep_host import FILLS, addressable, ring_seed

pytestmark = pytest.mark.gpu

KEYS = ("s", "action", "value", "logp", "adv", "ret")


# ---- snac_gae -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_gae_equals_the_rule_byte_for_byte_and_writes_the_span_only(N):
    import torch
    from snac_amd import _lib

    L, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    for cap, first, count in span_cases():
        S = make_span(np.random.default_rng(span_seed(N, cap, first, count)), cap, N, first, count)
        reward, done, value, boot = (torch.from_numpy(S[k]).to(dev) for k in ("reward", "done", "value", "bootstrap"))
        slots = span_slots(S)
        outside = torch.from_numpy(np.setdiff1d(np.arange(cap), slots)).to(dev)
        for with_boot in (True, False):
            A = guard.Arena(2 * cap * N * 4 + 4 * (guard.BAND + 1024), dev)
            adv, ret = A.carve((cap, N), torch.float32, offset=4, name="adv"), A.carve((cap, N), torch.float32, name="ret")
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(L.snac_gae(N, cap, first, count, GAMMA, LAM, _vp(reward), _vp(done), _vp(value), _vp(boot if with_boot else None),
                                  _vp(adv), _vp(ret), stream))
            want_adv, want_ret = gae_rule(S, GAMMA, LAM, bootstrap=with_boot)
            what = (N, cap, first, count, with_boot)
            assert adv.cpu().numpy()[slots].tobytes() == want_adv[slots].tobytes(), what
            assert ret.cpu().numpy()[slots].tobytes() == want_ret[slots].tobytes(), what
            if len(outside):
                guard.view_untouched(adv[outside], "adv outside the span")
                guard.view_untouched(ret[outside], "ret outside the span")
            A.check()


# ---- the gather on constructed rings ------------------------------------------------------------------------------------------------
def _buffer(env, cells, layout, cap, head, ticks, seed):
    """A RolloutBuffer of horizon cap - 1 over a constructed ring, its four arrays generated too, and the same contents for the rule."""
    import torch
    from snac_amd import RolloutBuffer

    buf = RolloutBuffer(env, cap - 1, GAMMA, LAM, layout=layout)
    buf.ring, R = constructed_ring(env, cells, layout, cap, head, ticks, seed)
    rng = np.random.default_rng(seed + 1)
    V = {k: (10.0 * rng.normal(size=(cap, env.num_envs))).astype(np.float32) for k in ("value", "logp", "adv", "ret")}
    for k, v in V.items():
        getattr(buf, k).copy_(torch.from_numpy(v))
    buf.first = (head - (cap - 1)) % cap
    norm = buf.update_norm().cpu().numpy()
    span = V["adv"][(buf.first + np.arange(cap - 1)) % cap].astype(np.float64)
    assert abs(norm[0] - span.mean()) <= span.size * 2.0 ** -23 * np.abs(span).mean()      # a float32 sum of span.size terms, any order
    assert abs(norm[1] * (span.std() + 1e-8) - 1.0) <= 1e-4
    return buf, R, V, norm


def _check_buffer(buf, R, V, norm, rng):
    """Every addressable entry at once, then batches of 1, 5 and 67 drawn from them, with and without plan_out and norm."""
    pairs = addressable(R)
    assert len(pairs) == len(buf.ring)
    slot, env = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    rows = {n: [onpolicy_rule(R, V, t, i, norm if n else None) for t, i in pairs] for n in (True, False)}
    old = buf.ring.gather(slot, env)
    for normalise in (True, False):
        got = buf.gather(slot, env, normalise=normalise)
        assert "s_next" not in got
        assert got["s"].cpu().numpy().tobytes() == old["s"].cpu().numpy().tobytes() and got["plan"].cpu().numpy().tobytes() == old["plan"].cpu().numpy().tobytes()
        equal_gather(got, stack_rows(rows[normalise], KEYS + ("plan",)), KEYS + ("plan",), "all, normalise %s" % normalise)
    for B, with_plan, normalise in ((1, False, True), (5, True, False), (67, False, False), (67, True, True)):
        pick = rng.integers(0, len(pairs), B)
        got = buf.gather(slot[pick], env[pick], normalise=normalise, with_plan=with_plan)
        keys = KEYS + (("plan",) if with_plan else ())
        assert ("plan" in got) == with_plan
        equal_gather(got, stack_rows([rows[normalise][j] for j in pick], keys), keys, "batch %d" % B)


@pytest.mark.parametrize("N,layout", [(5, "ticks"), (70, "ticks"), (70, "tiled")])
@pytest.mark.parametrize("f32", [False, True], ids=["f64ring", "f32ring"])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_constructed_rings_equal_the_rule_and_the_existing_gather(kind, f32, N, layout):
    env, cells = short_env(kind, N, f32)
    rng = np.random.default_rng(kind)
    for cap, head, ticks in FILLS:
        _check_buffer(*_buffer(env, cells, layout, cap, head, ticks, ring_seed(kind, f32, N, cap, head)), rng)


@pytest.mark.parametrize("kind,layout", [(1, "ticks"), (2, "tiled")])
def test_constructed_rings_with_the_position_tail(kind, layout):
    env, cells = short_env(kind, 70, False, obs_tail=("position",))
    assert env.obs_dim == (8 if kind == 1 else 53)
    _check_buffer(*_buffer(env, cells, layout, 7, 3, 10, 41 + kind), np.random.default_rng(9))


# ---- footprint ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ticks", "tiled"])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_the_gather_writes_nothing_outside_its_outputs(kind, layout):
    """Every output carved from an arena, on a 512-byte boundary and one element past it (plan_out: 16 bytes past); ragged batches.
    Reference: the same call into plain torch tensors (pinned above)."""
    import torch
    from snac_amd import RolloutBuffer, onpolicy

    for f32 in (False, True):
        env, _ = short_env(kind, 67, f32)
        buf = RolloutBuffer(env, 7, GAMMA, LAM, layout=layout)
        gen = torch.Generator().manual_seed(kind)
        for _ in range(7):
            buf.act(torch.randint(0, env.num_actions, (67,), generator=gen).to(torch.int8), torch.randn(67, generator=gen), torch.randn(67, generator=gen))
        buf.finish(torch.randn(67, generator=gen))
        buf.update_norm()
        rng = np.random.default_rng(kind)
        slots = buf.span_slots().cpu().numpy()
        D, PC, dev = env.obs_dim, buf.ring.plan_cells, env.device
        for B in (1, 3, 4, 5, 64, 67):
            for off in (0, 1):
                slot, idx = rng.choice(slots, B).astype(np.int32), rng.integers(0, 67, B).astype(np.int32)
                A = guard.Arena(B * ((D + PC) * 4 + 64) + 16 * (guard.BAND + 1024), dev)
                outs = [A.carve((B, D), torch.float32, offset=4 * off, name="s_out"), A.carve((B, PC), torch.float32, offset=16 * off, name="plan_out"),
                        A.carve((B,), torch.int64, offset=8 * off, name="action_out"), A.carve((B,), torch.float32, offset=4 * off, name="value_out"),
                        A.carve((B,), torch.float32, offset=4 * off, name="logp_out"), A.carve((B,), torch.float32, offset=4 * off, name="adv_out"),
                        A.carve((B,), torch.float32, offset=4 * off, name="ret_out")]
                with guard.allocations(onpolicy, outs):
                    got = buf.gather(slot, idx, normalise=bool(off))
                assert got["s"] is outs[0] and got["adv"] is outs[5] and got["ret"] is outs[6] and got["plan"].data_ptr() == outs[1].data_ptr()
                want = buf.gather(slot, idx, normalise=bool(off))
                for k in KEYS + ("plan",):
                    assert torch.equal(got[k], want[k]), k
                A.check()


# ---- RolloutBuffer on real envs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ticks", "tiled"])
@pytest.mark.parametrize("kind", [2, 3])
def test_rollout_buffer_on_real_envs(kind, layout):
    """N = 200, total_step = 12, horizon 29: episodes end inside the span, and the ring of 30 slots wraps in the second round."""
    import torch
    from snac_amd import RolloutBuffer

    N, H = 200, 29
    env, _ = short_env(kind, N, True)
    buf = RolloutBuffer(env, H, GAMMA, LAM, layout=layout)
    gen = torch.Generator().manual_seed(kind)
    with pytest.raises(ValueError, match="needs 29 ticks"):
        buf.finish(None)
    for rnd in range(2):
        for _ in range(H):
            buf.act(torch.randint(0, env.num_actions, (N,), generator=gen).to(torch.int8), 20.0 * torch.randn(N, generator=gen), -torch.rand(N, generator=gen))
        boot = 20.0 * torch.randn(N, generator=gen)
        buf.finish(boot)
        first, count = buf.first, H
        assert first == (rnd * H) % (H + 1) and (first + count > H + 1) == (rnd == 1) and buf.ring.ticks == (rnd + 1) * H
        S = dict(reward=buf.ring.reward.cpu().numpy(), done=buf.ring.done.cpu().numpy(), value=buf.value.cpu().numpy(), bootstrap=boot.numpy(),
                 first=first, count=count)
        slots = span_slots(S)
        dn = S["done"][slots] != 0
        assert dn.any(axis=0).all() and dn[:-1].any()                # every env's episode ends inside the span
        want_adv, want_ret = gae_rule(S, GAMMA, LAM)
        adv, ret = buf.adv.cpu().numpy(), buf.ret.cpu().numpy()
        assert adv[slots].tobytes() == want_adv[slots].tobytes() and ret[slots].tobytes() == want_ret[slots].tobytes(), rnd
        with pytest.raises(ValueError, match="needs 29 ticks"):
            buf.finish(boot)
    # one epoch: every (slot, env) of the span exactly once, a ragged last batch, the rows of gather()
    seen, sizes = [], []
    V = dict(value=S["value"], logp=buf.logp.cpu().numpy(), adv=adv, ret=ret)
    for mb in buf.minibatches(64, generator=torch.Generator(device=env.device).manual_seed(5)):
        sl, en = mb["slot"].cpu().numpy(), mb["env"].cpu().numpy()
        sizes.append(len(sl))
        seen.append(sl.astype(np.int64) * N + en)
        norm = buf.norm.cpu().numpy()
        assert torch.equal(mb["s"], buf.ring.gather(mb["slot"], mb["env"], with_plan=False)["s"]) and mb["plan"].shape == (len(sl), 20, 20)
        for k in ("value", "logp", "ret"):
            assert mb[k].cpu().numpy().tobytes() == V[k][sl, en].tobytes(), k
        assert mb["adv"].cpu().numpy().tobytes() == ((V["adv"][sl, en] - norm[0]) * norm[1]).astype(np.float32).tobytes()
        assert mb["action"].cpu().numpy().tolist() == buf.ring.action.cpu().numpy()[sl, en].tolist()
    assert sizes == [64] * (H * N // 64) + [H * N % 64] and H * N % 64
    want = (slots[:, None].astype(np.int64) * N + np.arange(N)[None, :]).reshape(-1)
    assert np.array_equal(np.sort(np.concatenate(seen)), np.sort(want))
    assert sum(1 for _ in buf.minibatches(4096, epochs=3, normalise=False)) == 3 * 2


# ---- the example --------------------------------------------------------------------------------------------------------------------
def test_the_ppo_example_runs():
    spec = importlib.util.spec_from_file_location("ppo_batched", os.path.join(helpers.ROOT, "examples", "ppo_batched.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses, returns = mod.run(envs=256, iterations=2, horizon=16, epochs=2, batch=1024, log=lambda line: None)
    assert len(losses) == 2 * 2 * 4 and all(np.isfinite(losses)) and len(returns) == 2 and all(np.isfinite(returns))
