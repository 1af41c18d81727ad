"""GPU: no env-batch kernel writes outside its outputs.  Every output of a call (rows, rewards, done flags, the four record arrays) and,
in the state test, every state array is carved from one arena of the test's own (tests/guard.py: 64 KiB of 0xA5 on both sides of each,
the interior pre-filled with 0x5A).  After each call, in this order: snac_last_kernel() is the kernel the case is meant to reach; the
bytes inside the outputs equal the CPU oracle's byte for byte (the record arrays, observe() and the final records: a shadow batch that
makes the same calls into plain torch tensors); arena.check() -- no byte outside the outputs changed; the regions the ABI documents as
NOT written still hold 0x5A:
  * rollout(obs="tiled"): rows [g_last, :, N % 64 :, :] of a ragged last tile            (test_inner_calls, call "roll_tiled" / "roll_ring")
  * rollout(ring=): every tick of the ring outside first_tick .. first_tick + T - 1, for first_tick 0, 3 and ring_ticks - T
                                                                                         (test_inner_calls, call "roll_ring")
  * k_rollout2d: the three sums words of an env that finished nothing in the launch      (test_inner_state_arrays, child "lane_*")
The state test binds the C ABI directly and runs every case twice: all eight arrays of snac_state on 512-byte boundaries, and ("weak")
each at the alignment include/snac_hip.h asks for past such a boundary and no better -- hdr, grid and plans 16 bytes past, episode and
plan_tb 4, the sums 8 (below that the library refuses the call: tests/test_cabi_host.py, on the host).  plans and plan_tb are inputs
there: after every call they hold what the test put in.  Its per-element inputs sit at their natural alignment: plan_idx_in 2 bytes
past a boundary, a mask 1, src_index / dst_index 4.  The 2D dynamic leg adds a table of 15 plan rows, where the 32-bit word that
k_rollout2d / k_rollout2db fetch for the last row ends two bytes past plan_tb.
Outputs are carved at the alignments of OFFSETS (never below the natural alignment of the element type): obs on a 512-byte boundary
and one element past it; done 0 / 1 / 4 / 8 bytes past (8 breaks the kernels' `& 15` test and keeps `& 3`), reward 0 / 4, the byte
records 0 / 1, the plan_idx record 0 / 2; explicit actions and step sizes -- inputs -- at the byte records' offsets.  Batch sizes: SIZES,
the smallest at which each tiling can go wrong (one lane group, a ragged tile, a full tile, full + ragged, either side of the 128- and
256-env blocks and of the 256-env thresholds).  Time limit 5 and launches of 1, 2 and 7 ticks in turn, so auto-reset runs inside a launch.

The dispatch knobs are read once per process: the cases run in child pytest processes of this file, one per entry of CHILDREN, one after
another.  Every child runs the same inner tests; a call runs in a child only where expect() -- the kernel-name table, checked on the host
against the dispatch of snac_hip.hip -- names one of the kernels the child is there for (CHILDREN[..]["targets"]).  The parent asserts that
the child reached every kernel of its "reach" list (so a changed knob default that takes a kernel out of reach fails
test_children[<child>]) and prints the table kernel x call x batch sizes x offsets that the inner runs recorded."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from devmem import _kernel
import guard
import helpers

pytestmark = pytest.mark.gpu

CHILD = os.environ.get("SNAC_TEST_FOOTPRINT_INNER", "")
inner = pytest.mark.skipif(not CHILD, reason="runs in the child processes of test_children")

ANY_N = [1, 3, 5, 63, 64, 65, 67, 257]                                 # the kernels that take any N
P16_N = [4, 8, 12, 60, 64, 68, 128, 132, 252, 256, 260, 516]           # the kernels behind pieces16 (N % 4 == 0)
SIZES = sorted(set(ANY_N + P16_N))
LAUNCHES = (1, 2, 7)
RING = 12                                                              # ticks of the tile-major ring; first_tick 0, 3 and RING - T
# byte offsets past a 512-byte boundary: (obs in ELEMENTS, done, reward, byte records and explicit inputs, plan_idx record)
OFFSETS = [(0, 0, 0, 0, 0), (0, 1, 4, 1, 2), (0, 4, 0, 0, 2), (0, 8, 4, 1, 0), (1, 0, 0, 0, 0), (1, 1, 4, 1, 2)]

AUXK = {1: "k_step1d", 2: "k_step2d", 3: "k_step3dq"}                 # the step kernels' AUX forms: masked resets and observe
_LANE = {"SNAC_1D_LANE_MIN_F64": 4, "SNAC_1D_LANE_MIN_F32": 4, "SNAC_2D_BLOCK": 0, "SNAC_2D_TP": 0, "SNAC_2D_STAGE_MIN": 4, "SNAC_3D_BLOCK_MIN": 4}
_BLOCK = {"SNAC_2D_BLOCK_MIN_F64": 4, "SNAC_2D_BLOCK_MIN_F32": 4}
# knobs: the overrides of the child; targets: the kernels whose calls it runs (None: every call); reach: what it must reach, by name;
# state: the kernels (without the envs of a block) it must reach in test_inner_state_arrays, with the state arrays at their weakest alignment
_STEPS = ["k_reset", "k_iou", "k_step1d", "k_step2d", "k_step3dq", "k_edges1d", "k_edges2d", "k_edges3d"]
CHILDREN = {
    "default": dict(knobs={}, targets=None, timeout=240,
                    reach=["k_rollout", "k_transition", "k_aux", "k_reset", "k_iou", "k_step1d", "k_step2d", "k_step3dq", "k_edges1d", "k_edges2d", "k_edges3d",
                           "k_transition2d", "k_transition3d", "k_rollout1dt/E4", "k_rollout2dt/E4", "k_rollout3d"],
                    state=_STEPS + ["k_aux", "k_transition", "k_transition2d", "k_transition3d", "k_rollout1dt", "k_rollout2dt", "k_rollout3d"]),
    "lane_xcd0": dict(knobs=dict(_LANE, SNAC_2D_STAGE_XCD=0), targets=["k_rollout1dl", "k_rollout2d", "k_rollout3db"], timeout=150,
                      reach=["k_rollout1dl", "k_rollout2d", "k_rollout3db"], state=_STEPS + ["k_rollout1dl", "k_rollout2d", "k_rollout3db"]),
    "lane_xcd1": dict(knobs=dict(_LANE, SNAC_2D_STAGE_XCD=1), targets=["k_rollout1dl", "k_rollout2d", "k_rollout3db"], timeout=150,
                      reach=["k_rollout1dl", "k_rollout2d", "k_rollout3db"], state=_STEPS + ["k_rollout1dl", "k_rollout2d", "k_rollout3db"]),
    "block128": dict(knobs=dict(_BLOCK, SNAC_2D_BLOCK_TWO_F64=128, SNAC_2D_BLOCK_TWO_F32=128), targets=["k_rollout2db"], timeout=120,
                     reach=["k_rollout2db/E64", "k_rollout2db/E128"], state=["k_rollout2db"]),
    "block256": dict(knobs=dict(_BLOCK, SNAC_2D_BLOCK_MAX_F64=255, SNAC_2D_BLOCK_MAX_F32=255, SNAC_2D_BLOCK_FOUR_MAX_F64=38912, SNAC_2D_BLOCK_FOUR_MAX_F32=45056),
                     targets=["k_rollout2db"], timeout=120, reach=["k_rollout2db/E64", "k_rollout2db/E256"]),
    "tp": dict(knobs={"SNAC_2D_TP_EB8": 8, "SNAC_1D_TP_EB8_MIN": 1073741824, "SNAC_1D_TP_EB16": 16}, targets=["k_rollout1dt", "k_rollout2dt"], timeout=150,
               reach=["k_rollout1dt/E4", "k_rollout1dt/E16", "k_rollout2dt/E4", "k_rollout2dt/E8"], state=["k_rollout1dt", "k_rollout2dt"]),
    "tile": dict(knobs={"SNAC_3D_PIPELINE": 0}, targets=None, timeout=240, reach=["k_rollout", "k_transition", "k_aux"],
                 state=["k_rollout", "k_transition", "k_aux"]),
    "step3d": dict(knobs={"SNAC_STEP3D_QUARTER": 0}, targets=["k_step3d"], timeout=120, reach=["k_step3d"]),
}
STATE_CHILDREN = tuple(c for c, spec in CHILDREN.items() if "state" in spec)   # test_inner_state_arrays runs in these
WEAK = " (state arrays), weak"                      # the call names of its weak variant in the report
ROLLS = ("roll_all", "roll_tiled", "roll_ring", "roll_last", "roll_none")


def expect(child, call, kind, n, aligned):
    """The kernel (with the envs of a block where a knob decides them) that `call` on n envs (edges: n edges) of `kind` reaches in `child`;
    aligned: the observation pointer is 16-byte aligned (or there is none).  Literal thresholds: a changed default shows as a failure."""
    k = CHILDREN[child]["knobs"]
    p16 = n % 4 == 0 and aligned
    if "SNAC_3D_PIPELINE" in k:
        return "k_rollout" if call in ROLLS else ("k_transition" if call in ("step", "edges") else "k_aux")
    if call in ("reset", "reset_scalar"):
        return "k_reset" if p16 and n >= 256 else "k_aux"
    if call in ("reset_mask", "observe"):
        return AUXK[kind] if p16 and n >= 256 else "k_aux"
    if call == "iou":
        return "k_iou" if n >= 256 else "k_aux"
    if call == "step":
        if kind == 1:
            return "k_step1d" if p16 and n >= 256 else "k_transition"
        if kind == 2:
            return "k_step2d" if p16 else "k_transition2d"
        return ("k_step3d" if "SNAC_STEP3D_QUARTER" in k else "k_step3dq") if p16 else "k_transition3d"
    if call == "edges":
        if kind == 1:
            return "k_edges1d" if n >= 64 else "k_transition"
        return ("k_edges2d" if kind == 2 else "k_edges3d") if p16 else ("k_transition2d" if kind == 2 else "k_transition3d")
    assert call in ROLLS, call
    if call in ("roll_last", "roll_none"):
        return "k_rollout"
    lane = "SNAC_2D_STAGE_MIN" in k
    if kind == 1:
        if lane and p16:
            return "k_rollout1dl"
        return "k_rollout1dt/E%d" % (16 if "SNAC_1D_TP_EB16" in k and n >= 16 else 4)
    if kind == 3:
        return "k_rollout3db" if lane and p16 else "k_rollout3d"
    if "SNAC_2D_BLOCK_MIN_F64" in k and p16:
        return "k_rollout2db/E%d" % (256 if "SNAC_2D_BLOCK_MAX_F64" in k and n > 255 else (128 if "SNAC_2D_BLOCK_TWO_F64" in k and n >= 128 else 64))
    if lane:
        return "k_rollout2d" if p16 else "k_rollout"
    return "k_rollout2dt/E%d" % (8 if "SNAC_2D_TP_EB8" in k and n >= 8 else 4)


def wanted(label):
    t = CHILDREN[CHILD]["targets"]
    return t is None or label.split("/")[0] in t


_REPORT = {}                                                           # (kernel label, call) -> {"n": set, "off": set}


def _note(label, call, n, off):
    e = _REPORT.setdefault((label, call), {"n": set(), "off": set()})
    e["n"].add(n)
    e["off"].add(off)


def _flush_report(name, seconds):
    d = os.environ.get("SNAC_TEST_FOOTPRINT_REPORT")
    if d:
        rows = [dict(kernel=k, call=c, n=sorted(v["n"]), off=sorted(v["off"])) for (k, c), v in sorted(_REPORT.items())]
        with open(os.path.join(d, "%s.json" % name), "w") as f:
            json.dump(dict(test=name, seconds=round(seconds, 2), rows=rows), f)
    _REPORT.clear()


def _allocations(views):
    """The outputs that a call of BatchedDMPEnv allocates itself (reset, observe, iou, transition, step without out=) come from the arena."""
    from snac_amd import batched

    return guard.allocations(batched, views)


def plan_tables(kind, dyn):
    table = helpers.plan_table(kind, dyn, ("sin_train" if kind == 1 else "dense_train") if dyn else "p0")[:16]
    return table, (table if kind == 1 else table.reshape(len(table), 26, 26))


class Case:
    """One batch, its oracle and its shadow (the same calls into plain torch tensors), and the arena of the current offset tuple."""

    def __init__(self, kind, dyn, n, f32, seed=5):
        import torch
        from snac_amd import BatchedDMPEnv

        table, shaped = plan_tables(kind, dyn)
        mk = lambda: BatchedDMPEnv(kind, dyn, n, plans=shaped, seed=seed, env_id_base=7, total_step=5, obs_dtype=torch.float32 if f32 else torch.float64)  # noqa: E731
        self.env, self.sh = mk(), mk()
        self.orc = helpers.oracle().OracleBatch(kind, dyn, n, table, seed=seed, env_id_base=7)
        self.orc.set_total_step(5)
        self.kind, self.dyn, self.n, self.f32, self.P = kind, dyn, n, f32, len(table)
        self.D, self.dt, self.dev = self.env.obs_dim, self.env.obs_dtype, self.env.device
        self.el = 4 if f32 else 8
        self.rng = np.random.default_rng(1000 * kind + n)
        want = self.orc.reset()
        assert self.rows(self.env.reset()) == self.cast(want).tobytes() and self.rows(self.sh.reset()) == self.cast(want).tobytes()

    def cast(self, o):
        return np.ascontiguousarray(o.astype(np.float32) if self.f32 else o)

    @staticmethod
    def rows(t):
        return t.cpu().numpy().tobytes()

    def begin(self, rows):
        """A fresh arena for one call whose largest output holds `rows` observation rows (9 views at the most: rows, rewards, done flags,
        four record arrays, two inputs; 16 bytes per env-step cover the small ones)."""
        self.A = guard.Arena(rows * (self.D * self.el + 16) + 12 * (guard.BAND + 1024), self.dev)

    # -- carving, by the offset tuple
    def obs(self, *lead):
        return self.A.carve(tuple(lead) + (self.n, self.D), self.dt, offset=self.off[0] * self.el, name="obs")

    def rd(self, *lead):
        import torch

        return (self.A.carve(tuple(lead) + (self.n,), torch.float32, offset=self.off[2], name="reward"),
                self.A.carve(tuple(lead) + (self.n,), torch.uint8, offset=self.off[1], name="done"))

    def record(self, T):
        import torch

        return {"actions": self.A.carve((T, self.n), torch.int8, offset=self.off[3], name="record actions"),
                "step_size": self.A.carve((T, self.n), torch.int8, offset=self.off[3], name="record step_size"),
                "plan_idx": self.A.carve((T, self.n), torch.int16, offset=self.off[4], name="record plan_idx"),
                "first": self.A.carve((T, self.n), torch.uint8, offset=self.off[3], name="record first")}

    def inputs(self, *lead):
        """Explicit actions and step sizes, carved at the byte records' offset: inputs, which the call must leave as they are."""
        import torch

        A = self.env.num_actions
        a = self.rng.integers(0, A, size=tuple(lead) + (self.n,)).astype(np.int8)
        k = self.rng.integers(1, 4, size=tuple(lead) + (self.n,)).astype(np.int8)
        ta = self.A.carve(a.shape, torch.int8, offset=self.off[3], name="actions (input)").copy_(torch.from_numpy(a))
        tk = self.A.carve(k.shape, torch.int8, offset=self.off[3], name="step_size (input)").copy_(torch.from_numpy(k))
        return a, k, ta, tk

    def label(self, call, n=None, has_obs=True):
        return expect(CHILD, call, self.kind, self.n if n is None else n, (not has_obs) or self.off[0] == 0)

    def reached(self, call, label, n=None):
        assert _kernel() == label.split("/")[0], (call, self.kind, self.n, self.off, _kernel(), label)
        _note(label, call, self.n if n is None else n, self.off)

    def same(self, got, want, what):
        assert self.rows(got) == np.ascontiguousarray(want).tobytes(), (what, self.kind, self.dyn, self.n, self.f32, self.off, _kernel())

    # -- the calls
    def reset(self, mode):
        import torch

        call = {"all": "reset", "mask": "reset_mask", "scalar": "reset_scalar"}[mode]
        label = self.label(call)
        if not wanted(label):
            return
        self.begin(self.n)
        o = self.obs()
        if mode == "scalar":
            p = min(3, self.P - 1)
            got = self.env.reset_scalar(p, out=o)
            self.reached(call, label)
            want = self.orc.reset(plan_idx=np.full(self.n, p))
            self.sh.reset_scalar(p)
        else:
            mask = None if mode == "all" else (np.arange(self.n) % 3 == 0).astype(np.uint8)
            tm = None if mask is None else torch.from_numpy(mask).to(self.dev)
            with _allocations([o]):
                got = self.env.reset(mask=tm)
            self.reached(call, label)
            want = self.orc.reset(mask=mask)
            self.sh.reset(mask=tm)
        assert got is o
        self.same(o, self.cast(want), call)
        self.A.check()

    def step(self, how):
        """how: "out" (preallocated outputs, counter RNG), "explicit" (preallocated outputs, explicit inputs), "alloc" (the call allocates),
        "noobs" (want_obs=False)."""
        has_obs = how != "noobs"
        label = self.label("step", has_obs=has_obs)
        if not wanted(label):
            return
        self.begin(self.n)
        a = k = ta = tk = None
        if how == "explicit":
            a, k, ta, tk = self.inputs()
        o = self.obs() if has_obs else None
        r, d = self.rd()
        t = self.env.t
        if how == "alloc":
            with _allocations([o, r, d]):
                go, gr, gd = self.env.step(auto_reset=True)
        else:
            go, gr, gd = self.env.step(ta, tk, auto_reset=True, want_obs=has_obs, out=(o, r, d))
        self.reached("step", label)
        assert go is o and gr is r and gd.data_ptr() == d.data_ptr()
        oc, rc, dc = self.orc.step(t, a, k, auto_reset=True)
        self.sh.step(ta, tk, auto_reset=True)
        if has_obs:
            self.same(o, self.cast(oc), "step rows")
        self.same(r, rc, "step rewards")
        self.same(d, dc, "step done flags")
        if ta is not None:
            self.same(ta, a, "actions (input)")
            self.same(tk, k, "step_size (input)")
        self.A.check()

    def rollout(self, mode, T, explicit=False, first=0):
        import torch

        call = {"all": "roll_all", "tiled": "roll_tiled", "ring": "roll_ring", "last": "roll_last", None: "roll_none"}[mode]
        label = self.label(call, has_obs=mode is not None)
        if not wanted(label):
            return
        n, D, G = self.n, self.D, (self.n + 63) // 64
        self.begin(max(T * n, G * 64 * (RING if mode == "ring" else T)))
        a = k = ta = tk = None
        if explicit:
            a, k, ta, tk = self.inputs(T)
        ticks = RING if mode == "ring" else T
        if mode == "all":
            o = self.obs(T)
        elif mode == "last":
            o = self.obs()
        elif mode is None:
            o = None
        else:
            o = self.A.carve((G, ticks, 64, D), self.dt, offset=self.off[0] * self.el, name="obs (tile-major)")
        r, d = self.rd(T)
        rec = self.record(T) if mode in ("all", "ring") else None
        t0 = self.env.t
        go, gr, gd = self.env.rollout(T, actions=ta, step_size=tk, obs="tiled" if mode == "ring" else mode, out=o, reward_out=r, done_out=d, record=rec,
                                      ring=(RING, first) if mode == "ring" else None)
        self.reached(call, label)
        assert go is o and gr is r and gd.data_ptr() == d.data_ptr()
        oc, rc, dc = self.orc.rollout(T, t0=t0, actions=a, step_size=k, obs="last" if mode == "last" else ("all" if mode is not None else None))
        ref = {name: torch.empty_like(v) for name, v in rec.items()} if rec else None
        self.sh.rollout(T, actions=ta, step_size=tk, obs=None, record=ref)
        if mode in ("all", "last"):
            self.same(o, self.cast(oc), call + " rows")
        elif mode is not None:
            # the whole tile-major tensor, byte for byte: the oracle's rows where the ABI puts them, 0x5A everywhere else
            want = np.full((G, ticks, 64, D * self.el), guard.FRESH_BYTE, np.uint8)
            rows = self.cast(oc).view(np.uint8).reshape(T, n, D * self.el)
            for g in range(G):
                m = min(64, n - 64 * g)
                want[g, first:first + T, :m] = rows[:, 64 * g:64 * g + m]
            self.same(o, want, call + " rows (tile-major)")
        self.same(r, rc, call + " rewards")
        self.same(d, dc, call + " done flags")
        if rec:
            for name in rec:
                self.same(rec[name], ref[name].cpu().numpy(), call + " record " + name)
            if explicit:
                self.same(rec["actions"], a, "recorded actions = the explicit ones")
                self.same(rec["step_size"], k, "recorded step sizes = the explicit ones")
        if ta is not None:
            self.same(ta, a, "actions (input)")
            self.same(tk, k, "step_size (input)")
        self.A.check()
        if mode in ("tiled", "ring"):
            if n % 64:
                guard.view_untouched(o[G - 1, :, n % 64:, :], "the envs of the ragged last tile beyond N")
            if mode == "ring":
                guard.view_untouched(o[:, :first], "ring ticks before first_tick")
                guard.view_untouched(o[:, first + T:], "ring ticks from first_tick + T")

    def edges(self):
        """snac_transition with src and dst: every row of the pool stepped in place, through a permutation (m = N edges)."""
        label = self.label("edges")
        if not wanted(label):
            return
        import torch

        self.begin(self.n)
        a, k, ta, tk = self.inputs()
        perm = self.rng.permutation(self.n).astype(np.int32)
        o = self.A.carve((self.n, self.D), self.dt, offset=self.off[0] * self.el, name="obs")
        r, d = self.rd()
        with _allocations([o, r, d]):
            go, gr, gd = self.env.transition(ta, tk, src=torch.from_numpy(perm), dst=torch.from_numpy(perm), t=3)
        self.reached("edges", label)
        assert go is o and gr is r and gd.data_ptr() == d.data_ptr()
        oc, rc, dc = self.orc.transition(a, k, src=perm, dst=perm, t=3)
        self.sh.transition(ta, tk, src=torch.from_numpy(perm), dst=torch.from_numpy(perm), t=3)
        self.same(o, self.cast(oc), "edge rows")
        self.same(r, rc, "edge rewards")
        self.same(d, dc, "edge done flags")
        self.same(ta, a, "actions (input)")
        self.A.check()

    def observe(self):
        label = self.label("observe")
        if not wanted(label):
            return
        self.begin(self.n)
        o = self.obs()
        with _allocations([o]):
            assert self.env.observe() is o
        self.reached("observe", label)
        self.same(o, self.sh.observe().cpu().numpy(), "observe rows (the shadow's)")
        self.A.check()

    def iou(self):
        import torch

        label = self.label("iou", has_obs=False)
        if not wanted(label):
            return
        self.begin(self.n)
        out = self.A.carve((self.n,), torch.float64, offset=8 * self.off[0], name="iou")
        with _allocations([out]):
            assert self.env.iou() is out
        self.reached("iou", label)
        self.same(out, self.orc.iou(), "iou")
        self.A.check()

    def records_equal_shadow(self):
        import torch

        e, s = self.env, self.sh
        assert torch.equal(e._hdr, s._hdr) and torch.equal(e._grid, s._grid) and torch.equal(e._episode, s._episode) and torch.equal(e._stats, s._stats)
        st = self.orc.stats()
        got = e._stats.cpu().numpy()
        assert np.array_equal(got[0], st["episodes"]) and np.array_equal(got[1], st["ret"]) and np.array_equal(got[2], st["iou_fx"])


def _sequence(c, off):
    """Every call of the issue's list once, at one offset tuple.  The tuples that differ only in done / reward / records leave out the
    calls that have none of those (resets, observe, iou): their first byte would lie where tuple 0 or 4 put it."""
    c.off = off
    full = off[1:] == (0, 0, 0, 0)
    if full:
        c.reset("all")
        c.reset("mask")
        c.reset("scalar")
    for how in ("out", "explicit", "alloc", "noobs"):
        c.step(how)
    for T in LAUNCHES:
        c.rollout("all", T)
    c.rollout("all", 2, explicit=True)
    for T in LAUNCHES:
        c.rollout("tiled", T)
    for T, first in zip(LAUNCHES, (0, 3, RING - 7)):
        c.rollout("ring", T, first=first)
    c.rollout("ring", 2, explicit=True, first=RING - 2)
    for T in LAUNCHES:
        c.rollout("last", T)
        c.rollout(None, T)
    c.edges()
    if full:
        c.observe()
        c.iou()


@inner
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("dyn", [False, True], ids=["sta", "dyn"])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_inner_calls(kind, dyn, f32, request):
    t0 = time.time()
    for n in SIZES:
        c = Case(kind, dyn, n, f32)
        for off in OFFSETS:
            _sequence(c, off)
        c.records_equal_shadow()
    _flush_report(request.node.name, time.time() - t0)


# ---- the state arrays: the C ABI bound directly, every array of snac_state carved from the arena
# the odd plan table of the 2D dynamic leg and its seed, picked on the host with the oracle alone: of the seeds 0 .. 39, 25 give what
# _state_case asserts of _rehearse() at every n of the case (5 envs: ten resets over 15 rows); 11, the other cases' seed, is one of them
ODD_ROWS, ODD_SEED = 15, 11


def _rehearse(kind, dyn, n, table, seed):
    """The oracle alone, before anything runs on the GPU: the state case's calls up to the end of its two rollout launches, the launches
    one tick at a time.  -> [(the env's previous plan row, the row it was reset onto)] of every reset inside those launches, and the
    oracle's state behind them (the case compares it with its own oracle's: the launches as a whole did what the single ticks did)."""
    orc = helpers.oracle().OracleBatch(kind, dyn, n, table, seed=seed, env_id_base=7)
    orc.set_total_step(5)
    orc.reset()
    for t in range(3):
        orc.step(t, auto_reset=True, want_obs=False)
    resets = []
    for t in range(3, 3 + 1 + 7):
        before = orc.state()
        orc.rollout(1, t0=t, obs=None)
        after = orc.state()
        for i in np.nonzero(after["episode"] != before["episode"])[0]:
            resets.append((int(before["plan_idx"][i]), int(after["plan_idx"][i])))
    return resets, orc.state()


def _state_case(kind, dyn, n, f32, weak=False, rows=16, seed=11):
    """weak: every array of snac_state at the alignment include/snac_hip.h asks for ("Alignment of the state arrays") past a 512-byte
    boundary, and no better.  rows: the plan rows of the table (ODD_ROWS: the 32-bit word of plan_tb's last row ends two bytes past the
    array, inside the band)."""
    import torch
    from snac_amd import _lib, plans

    L = _lib.lib()
    sz = _lib.env_sizes(kind, dyn)
    table, shaped = plan_tables(kind, dyn)
    table, shaped = table[:rows], shaped[:rows]
    packed, tb = plans.pack_plans(kind, np.array(shaped, np.float64))
    P = len(packed)
    assert P == (rows if dyn else 1)                                   # (the static classes: their one plan)
    rehearsed = None
    if rows % 2:
        # what the odd table is there for, from the oracle alone: the launches of k_rollout2d / k_rollout2db fetch total_brick as the
        # 32-bit word that holds the row -- the low half for an even row, the high half for an odd one, the last word for row P - 1
        resets, rehearsed = _rehearse(kind, dyn, n, table, seed)
        fresh = [new for old, new in resets if new != old]
        assert any(new % 2 == 0 for new in fresh), "no env is reset onto another, even plan row"
        assert any(new % 2 == 1 for new in fresh), "no env is reset onto another, odd plan row"
        assert P - 1 in fresh, "no env is reset onto the last row of the odd table from another row"
    dev = torch.device("cuda", torch.cuda.current_device())
    gdt = {1: torch.int16, 2: torch.int32, 3: torch.int16}[kind]
    pdt = torch.int32 if kind == 2 else torch.int16
    assert sz.grid_elem_bytes == torch.empty((), dtype=gdt).element_size() and sz.plan_elem_bytes == torch.empty((), dtype=pdt).element_size()
    A = guard.Arena(n * (16 + 4 + 24 + sz.grid_elems * sz.grid_elem_bytes + 1 + 2 + 8) + P * (sz.plan_elems * sz.plan_elem_bytes + 2)
                    + 14 * (guard.BAND + 512) + 4096, dev)
    w = (lambda need: need) if weak else (lambda need: 0)              # the offset past a 512-byte boundary: the requirement itself, or none
    hdr = A.carve((n, 4), torch.int32, offset=w(16), name="hdr").zero_()
    epi = A.carve((n,), torch.int32, offset=w(4), name="episode").fill_(-1)
    grid = A.carve((n, sz.grid_elems), gdt, offset=w(16), name="grid").zero_()
    sums = [A.carve((n,), torch.int64, offset=w(8), name=nm).zero_() for nm in ("stat_episodes", "stat_return", "stat_iou_fx")]
    d_plans = A.carve((P, sz.plan_elems), pdt, offset=w(16), name="plans").copy_(torch.from_numpy(packed.view(np.int32) if kind == 2 else packed))
    d_tb = A.carve((P,), torch.int16, offset=w(4), name="plan_tb").copy_(torch.from_numpy(tb))
    for arr, need in [(hdr, 16), (epi, 4), (grid, 16), (d_plans, 16), (d_tb, 4)] + [(s, 8) for s in sums]:
        assert arr.data_ptr() % 512 == w(need)
    keep_plans, keep_tb = d_plans.clone(), d_tb.clone()
    desc = _lib.EnvDesc(kind, int(dyn), n, P, _lib.OBS_F32 if f32 else _lib.OBS_F64, 0, seed, 7, 5, 0, -1, _lib.SCALARS_DEFAULT, 0, 0)
    st = _lib.State(hdr.data_ptr(), epi.data_ptr(), grid.data_ptr(), d_plans.data_ptr(), d_tb.data_ptr(), *[s.data_ptr() for s in sums])
    dref, sref = C.byref(desc), C.byref(st)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    D = L.snac_obs_dim(dref)
    odt = torch.float32 if f32 else torch.float64
    cast = lambda o: np.ascontiguousarray(o.astype(np.float32) if f32 else o)  # noqa: E731
    same = lambda got, want, what: Case.same(_Where(kind, dyn, n, f32, weak, rows), got, want, what)  # noqa: E731
    ok = lambda rc: _lib.check(rc)  # noqa: E731
    aligned = True

    orc = helpers.oracle().OracleBatch(kind, dyn, n, table, seed=seed, env_id_base=7)
    orc.set_total_step(5)

    def reach(call, m=None):
        label = expect(CHILD, call, kind, n if m is None else m, aligned)
        assert _kernel() == label.split("/")[0], (call, kind, n, _kernel(), label)
        _note(label, call + (WEAK if weak else " (state arrays)"), n, (0, 0, 0, 0, 0))
        return label

    def settled():
        """No byte outside the carved arrays changed, and the plans and their total_brick -- inputs of every call here -- are as they were."""
        A.check()
        assert torch.equal(d_plans, keep_plans) and torch.equal(d_tb, keep_tb), ("a call wrote the plan table", kind, dyn, n, f32, weak, rows, _kernel())

    obs = torch.empty((n, D), dtype=odt, device=dev)
    rew, done = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    ok(L.snac_reset(dref, sref, None, None, vp(obs), stream))
    reach("reset")
    same(obs, cast(orc.reset()), "reset rows")
    settled()
    t = 0
    for _ in range(3):
        ok(L.snac_step(dref, sref, t, None, None, 1, vp(obs), vp(rew), vp(done), stream))
        reach("step")
        oc, rc, dc = orc.step(t, auto_reset=True)
        same(obs, cast(oc), "step rows"), same(rew, rc, "step rewards"), same(done, dc, "step done flags")
        settled()
        t += 1
    for T in (1, 7):
        # the sums words pre-filled with the fresh pattern: an env that finishes nothing in the launch keeps the pattern (k_rollout2d does
        # not write its words at all; a kernel that adds zero to what it loaded stores the pattern back), the others hold pattern + their
        # own, which goes back on top of the saved sums afterwards
        saved = [s.clone() for s in sums]
        for s in sums:
            guard.fresh(s)
        pattern = int.from_bytes(bytes([guard.FRESH_BYTE]) * 8, "little")
        traj = torch.empty((T, n, D), dtype=odt, device=dev)
        r2, d2 = torch.empty((T, n), dtype=torch.float32, device=dev), torch.empty((T, n), dtype=torch.uint8, device=dev)
        ok(L.snac_rollout(dref, sref, T, t, None, None, _lib.OBS_ALL, vp(traj), vp(r2), vp(d2), stream))
        label = reach("roll_all")
        oc, rc, dc = orc.rollout(T, t0=t)
        same(traj, cast(oc), "rollout rows"), same(r2, rc, "rollout rewards"), same(d2, dc, "rollout done flags")
        settled()
        idle = torch.from_numpy(~dc.astype(bool).any(axis=0)).to(dev)
        if T == 1 and n >= 64:
            assert bool(idle.any()), "some env finishes nothing in a launch of one tick"
        for s in sums:
            guard.view_untouched(s[idle], "the sums words of the envs that finished nothing (%s)" % label)
        for s, keep in zip(sums, saved):
            s.copy_(keep + (s - pattern))
        t += T
    if rehearsed is not None:                                          # the launches did what _rehearse()'s single ticks did
        so = orc.state()
        assert all(np.array_equal(so[f], rehearsed[f]) for f in ("episode", "plan_idx", "tb", "cs"))
    out = torch.empty(n, dtype=torch.float64, device=dev)
    ok(L.snac_iou(dref, sref, vp(out), stream))
    reach("iou")
    same(out, orc.iou(), "iou")
    settled()
    # the per-element inputs at their natural alignment and no better: plan rows (int16) 2 bytes past a 512-byte boundary, a mask 1 byte
    # past, edge indices (int32) 4 bytes past; inputs, which a call leaves as they are
    rng = np.random.default_rng(n)
    rows_in = rng.integers(0, P, n).astype(np.int16)
    t_rows = A.carve((n,), torch.int16, offset=2, name="plan_idx_in").copy_(torch.from_numpy(rows_in))
    ok(L.snac_reset(dref, sref, None, vp(t_rows), vp(obs), stream))
    reach("reset")
    same(obs, cast(orc.reset(plan_idx=rows_in)), "rows of the reset onto given plan rows")
    same(t_rows, rows_in, "plan_idx_in (input)")
    settled()
    ok(L.snac_step(dref, sref, t, None, None, 1, vp(obs), vp(rew), vp(done), stream))   # the masked reset then finds envs in mid-episode
    reach("step")
    oc, rc, dc = orc.step(t, auto_reset=True)
    same(obs, cast(oc), "step rows"), same(rew, rc, "step rewards"), same(done, dc, "step done flags")
    settled()
    t += 1
    mask_in = (np.arange(n) % 3 == 0).astype(np.uint8)
    mask = A.carve((n,), torch.uint8, offset=1, name="mask").copy_(torch.from_numpy(mask_in))
    ok(L.snac_reset(dref, sref, vp(mask), None, vp(obs), stream))
    reach("reset_mask")
    same(obs, cast(orc.reset(mask=mask_in)), "masked reset rows")
    same(mask, mask_in, "mask (input)")
    settled()
    # two waves of edges: rows of the lower half stepped into the upper half, with dst alone and with src and dst
    m = n // 2
    if m:
        src = rng.permutation(n - m)[:m].astype(np.int32)
        t_src = A.carve((m,), torch.int32, offset=4, name="src_index").copy_(torch.from_numpy(src))
        t_dst = A.carve((m,), torch.int32, offset=4, name="dst_index")
        for tick, with_src in ((9, False), (10, True)):
            a, k = rng.integers(0, sz.num_actions, m).astype(np.int8), rng.integers(1, 4, m).astype(np.int8)
            dst = (n - m + rng.permutation(m)).astype(np.int32)
            t_dst.copy_(torch.from_numpy(dst))
            ta, tk = (torch.from_numpy(x).to(dev) for x in (a, k))
            ok(L.snac_transition(dref, sref, m, vp(t_src) if with_src else None, vp(t_dst), tick, vp(ta), vp(tk), vp(obs), vp(rew), vp(done), stream))
            aligned = True
            reach("edges", m)
            oc, rc, dc = orc.transition(a, k, src=src if with_src else None, dst=dst, t=tick)
            same(obs[:m], cast(oc), "edge rows"), same(rew[:m], rc, "edge rewards"), same(done[:m], dc, "edge done flags")
            same(t_src, src, "src_index (input)"), same(t_dst, dst, "dst_index (input)")
            settled()
    # the state, against the oracle's
    so, ss = orc.state(), orc.stats()
    h8, h16 = hdr.view(torch.int8).cpu().numpy(), hdr.view(torch.int16).cpu().numpy()
    pos = h8[:, 0:2].astype(np.int64)
    assert np.array_equal(pos[:, 0], so["pos"][:, 0]) and (kind == 1 or np.array_equal(pos[:, 1], so["pos"][:, 1]))
    assert np.array_equal((h8[:, 2] & _lib.FLAG_NEED_RESET) != 0, so["need_reset"] != 0)
    for col, name in ((2, "cb"), (3, "cs"), (4, "tb"), (5, "plan_idx"), (6, "ep_return")):
        assert np.array_equal(h16[:, col].astype(np.int64), so[name].astype(np.int64)), name
    assert np.array_equal(epi.cpu().numpy(), so["episode"])
    mem = torch.empty((n, sz.env_height, sz.env_width), dtype=torch.float64, device=dev)
    ok(L.snac_export_grid(dref, sref, vp(mem), stream))
    assert np.array_equal(mem.cpu().numpy().reshape(n, -1), so["grid"])
    for s, name in zip(sums, ("episodes", "ret", "iou_fx")):
        assert np.array_equal(s.cpu().numpy(), ss[name]), name
    A.check()


class _Where:
    def __init__(self, kind, dyn, n, f32, weak, rows):
        self.kind, self.dyn, self.n, self.f32, self.off = kind, dyn, n, f32, "state arrays%s, %d plan rows" % (" at their weakest alignment" if weak else "", rows)

    rows = staticmethod(Case.rows)


@inner
@pytest.mark.parametrize("dyn", [False, True], ids=["sta", "dyn"])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_inner_state_arrays(kind, dyn, request):
    if CHILD not in STATE_CHILDREN:
        return
    t0 = time.time()
    for n in (5, 64, 68, 260):
        for f32 in (False, True):
            for weak in (False, True):
                _state_case(kind, dyn, n, f32, weak=weak)
            if kind == 2 and dyn:
                _state_case(kind, dyn, n, f32, weak=True, rows=ODD_ROWS, seed=ODD_SEED)
    _flush_report(request.node.name, time.time() - t0)


@inner
def test_inner_the_knobs_are_what_the_child_was_given():
    from snac_amd import _lib

    t = _lib.tuning()
    for name, value in CHILDREN[CHILD]["knobs"].items():
        assert t[name][0] == value == int(os.environ[name]), name
    # the defaults that expect() states as literals
    for name, value in (("SNAC_RESET_FAST_MIN", 256), ("SNAC_STEP1D_MIN", 256), ("SNAC_EDGES1D_MIN", 64), ("SNAC_EDGES2D_MIN", 4), ("SNAC_STEP3D_QUARTER_MIN", 4)):
        assert t[name][0] == value, name


def _table(rows):
    """kernel x call x batch sizes x offsets, as text."""
    out = ["%-18s %-34s %-62s %s" % ("kernel", "call", "batch sizes (edges: edges per call)", "offsets (obs elements, done, reward, byte records, plan_idx)")]
    for r in rows:
        out.append("%-18s %-34s %-62s %s" % (r["kernel"], r["call"], " ".join(str(n) for n in r["n"]), " ".join("/".join(str(x) for x in o) for o in r["off"])))
    return "\n".join(out)


_STOPPED = []                                                          # the first child that did not return 0


@pytest.mark.parametrize("child", list(CHILDREN))
def test_children(child, tmp_path):
    if CHILD:
        pytest.skip("the child itself")
    assert not _STOPPED, "not run: child %s did not return 0 (the children stop at the first that fails)" % _STOPPED[0]
    spec = CHILDREN[child]
    env = {k: v for k, v in os.environ.items() if not k.startswith("SNAC_") or k.startswith("SNAC_FOOTPRINT")}
    env.update({k: str(v) for k, v in spec["knobs"].items()})
    env.update(SNAC_TEST_FOOTPRINT_INNER=child, SNAC_TEST_FOOTPRINT_REPORT=str(tmp_path))
    _STOPPED.append(child)                                             # until it has returned 0: a time limit or a crash stops the rest too
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "inner", "-p", "no:cacheprovider"],
                         cwd=helpers.ROOT, env=env, capture_output=True, text=True, timeout=spec["timeout"])
    if out.returncode == 0:
        _STOPPED.remove(child)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "skipped" not in out.stdout.splitlines()[-1], out.stdout[-500:]
    rows, seconds = [], {}
    for name in sorted(os.listdir(str(tmp_path))):
        with open(os.path.join(str(tmp_path), name)) as f:
            rep = json.load(f)
        rows += rep["rows"]
        seconds[rep["test"]] = rep["seconds"]
    merged = {}
    for r in rows:
        e = merged.setdefault((r["kernel"], r["call"]), {"n": set(), "off": set()})
        e["n"].update(r["n"])
        e["off"].update(tuple(o) for o in r["off"])
    rows = [dict(kernel=k, call=c, n=sorted(v["n"]), off=sorted(v["off"])) for (k, c), v in sorted(merged.items())]
    reached = {r["kernel"] for r in rows}
    missing = [k for k in spec["reach"] if k not in reached]
    assert not missing, "child %s no longer reaches %s (reached: %s)" % (child, missing, sorted(reached))
    weak = {r["kernel"].split("/")[0] for r in rows if r["call"].endswith(WEAK)}
    missing = [k for k in spec.get("state", []) if k not in weak]
    assert not missing, "child %s no longer reaches %s with the state arrays at their weakest alignment (reached: %s)" % (child, missing, sorted(weak))
    text = "child %s  knobs: %s\n%s\nseconds per inner test: %s" % (child, spec["knobs"] or "none", _table(rows), json.dumps(seconds))
    print(text)
    dump = os.environ.get("SNAC_FOOTPRINT_TABLE_DIR")                   # a directory that receives the tables as text files
    if dump:
        with open(os.path.join(dump, "footprint_%s.txt" % child), "w") as f:
            f.write(text + "\n")
