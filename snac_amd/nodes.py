"""2D tree-search node pools with ONE record per node (snac_node2d, include/snac_hip.h; snac_amd/csrc/k_nodes.hip; the record's map: snac_amd/csrc/nodes_dev.h).

`BatchedDMPEnv.transition()` uses the batch itself as the node pool: a tree edge then reads its parent's header, episode counter and
board from three arrays at a random row -- three lines of memory for 100 bytes.  A NodePool2D keeps the three in one 128-byte record,
so an edge reads one line and writes one (524 288 random-parent edges: see bench.py `transition_2d_nodes_524288_edges`).  The rules
are the batch's: Env/2D/DMP_ENV_2D_dynamic_MCTS.py:117-175 `transition(state, action)`, one call per tree edge in
script/MCTS/utils/mcts_Qvalue_dynamic.py:88,118 -- here m edges per launch.

    env = BatchedDMPEnv(2, True, 4096, seed=1); env.reset()            # the roots (or import_states(...))
    pool = NodePool2D(env, 1 << 20)
    pool.load(rows=root_rows, node_rows=root_nodes)                     # batch rows -> node records
    obs, reward, done = pool.transition(actions, step_size, src=parents, dst=children)
    pool.store(node_rows=leaves, rows=leaf_rows)                        # node records -> batch rows (observe(), ...)
    est, steps = pool.evaluate(leaves, H, gamma, first_reward=reward)  # default-policy evaluation in place (script/MCTS/utils/mcts.py:100-110)

NodePool1D (snac_node1d: one 128-byte line per node) and NodePool3D (snac_node3d: seven whole lines) do the same for the other two
kinds (transition(state, action): Env/1D/DMP_Env_1D_dynamic_MCTS.py:82-139, Env/3D/DMP_simulator_3d_dynamic_triangle_MCTS.py:195-277);
NodePool(env, rows) picks the class of env.kind, so a search written against one pool runs unchanged on the others.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import ptr as _ptr


def _words(struct):
    """int32 words of a record of include/snac_hip.h."""
    return C.sizeof(_lib.STRUCTS[struct]) // 4


class _NodePool:
    """What the pools of the three kinds share; a subclass names its kind, its record's int32 words and its three entry points."""
    KIND, WORDS, CANONICAL_OBS, PACK, UNPACK, TRANSITION, EVALUATE, OBSERVE = None, None, None, None, None, None, None, None

    def __init__(self, env, rows):
        """env: a BatchedDMPEnv of the pool's kind -- its rules, plan table, observation dtype and device are the pool's; rows: node records."""
        if env.kind != self.KIND:
            raise ValueError("node records exist for the %dD kinds" % self.KIND)
        if env.obs_dim != self.CANONICAL_OBS:
            raise ValueError("a node pool writes the canonical observation rows")
        self.env, self.rows = env, int(rows)
        if self.rows < 1:
            raise ValueError("rows must be >= 1")
        # torch allocations are at least 512-byte aligned: every record starts a 128-byte line
        self.records = torch.zeros((self.rows, self.WORDS), dtype=torch.int32, device=env.device)
        assert self.records.data_ptr() % 128 == 0
        self._lib = env._lib
        self._gpow = {}                                              # (gamma, H) -> gamma**t on the device, for evaluate()

    # ---- records <-> batch rows ---------------------------------------------------------------------------------
    def _idx(self, x, m, limit, what):
        if x is None:
            if m > limit:
                raise ValueError("%s: %d rows, %d given" % (what, limit, m))
            return None
        t = torch.as_tensor(x, device=self.env.device).reshape(-1)
        if int(t.numel()) != m:
            raise ValueError("%s must have %d entries" % (what, m))
        if m and (int(t.min()) < 0 or int(t.max()) >= limit):
            raise ValueError("%s out of range" % what)
        return t.to(torch.int32).contiguous()

    def _count(self, a, b, default):
        for x in (a, b):
            if x is not None:
                return int(torch.as_tensor(x).numel())
        return int(default)

    def load(self, rows=None, node_rows=None, env=None):
        """Node record node_rows[i] <- batch row rows[i] of `env` (default: the pool's own batch); None = row i."""
        env = env or self.env
        m = self._count(rows, node_rows, min(env.num_envs, self.rows))
        ri, ni = self._idx(rows, m, env.num_envs, "rows"), self._idx(node_rows, m, self.rows, "node_rows")
        with torch.cuda.device(env.device):
            _lib.check(getattr(self._lib, self.PACK)(C.byref(env._desc), C.byref(env._state), _ptr(ri), m, _ptr(self.records), self.rows, _ptr(ni),
                                                   env._stream()))
        return m

    def store(self, node_rows=None, rows=None, env=None):
        """Batch row rows[i] of `env` <- node record node_rows[i]; None = row i."""
        env = env or self.env
        m = self._count(rows, node_rows, min(env.num_envs, self.rows))
        ri, ni = self._idx(rows, m, env.num_envs, "rows"), self._idx(node_rows, m, self.rows, "node_rows")
        with torch.cuda.device(env.device):
            _lib.check(getattr(self._lib, self.UNPACK)(C.byref(env._desc), _ptr(self.records), self.rows, _ptr(ni), m, C.byref(env._state), _ptr(ri),
                                                     env._stream()))
        env._was_reset = True
        return m

    # ---- the edges ------------------------------------------------------------------------------------------------
    def transition(self, actions, step_size=None, src=None, dst=None, t=0, want_obs=True, check=True):
        """m tree edges in one launch: record dst[i] <- step(record src[i], actions[i], step_size[i]); src / dst None = record i.
        Same rules and outputs as BatchedDMPEnv.transition(): no auto-reset, a dst record must not be the src record of another
        edge of the same call (check=False skips that test: a host round trip per wave).  Returns (obs [m, obs_dim], reward [m], done [m])."""
        env = self.env
        a = torch.as_tensor(actions, device=env.device) if not torch.is_tensor(actions) else actions.to(env.device)
        m = int(a.numel())
        a = env._i8(a.reshape(-1), (m,), "actions")
        k = env._i8(step_size, (m,), "step_size")
        si, di = self._idx(src, m, self.rows, "src"), self._idx(dst, m, self.rows, "dst")
        if check and m and (si is not None or di is not None):
            s_ = si if si is not None else torch.arange(m, device=env.device, dtype=torch.int32)
            d_ = di if di is not None else torch.arange(m, device=env.device, dtype=torch.int32)
            if bool(torch.isin(d_, s_[s_ != d_]).any()) or int(torch.unique(d_).numel()) != m:
                raise ValueError("dst records must be distinct and must not be the src record of another edge")
        obs = torch.empty((m, env.obs_dim), dtype=env.obs_dtype, device=env.device) if want_obs else None
        reward = torch.empty((m,), dtype=torch.float32, device=env.device)
        done = torch.empty((m,), dtype=torch.uint8, device=env.device)
        with torch.cuda.device(env.device):
            _lib.check(getattr(self._lib, self.TRANSITION)(C.byref(env._desc), C.byref(env._state), _ptr(self.records), self.rows, m, _ptr(si), _ptr(di),
                                                         int(t) & 0xFFFFFFFF, _ptr(a), _ptr(k), _ptr(obs), _ptr(reward), _ptr(done), env._stream()))
        return obs, reward, done.view(torch.bool)

    # ---- leaf evaluation --------------------------------------------------------------------------------------------
    def evaluate(self, node_rows, horizon, gamma, first_reward=None, t0=0, check=True):
        """Default-policy evaluation of tree leaves in place (script/MCTS/utils/mcts.py:100-110), one launch on the records: from each
        record node_rows[i] (None: record i, m = len(first_reward) or every record), up to `horizon` random steps (the env's action_probs, else uniform) that stop
        at the first `done`, estimate = first_reward + sum_t reward_t * gamma**t in float64 -- what BatchedDMPEnv.evaluate() computes
        for the same states, bit for bit.  Actions come from the counter RNG keyed by (env_id_base + i, t0 + t): t0 = 0 draws those of
        BatchedDMPEnv.evaluate(), another t0 fresh ones.  A terminal leaf is not rolled out.  The records are not changed.  check=False
        skips the range test of node_rows (a host round trip).  Enqueued on the env's stream.
        Returns (estimate float64 [m], steps int64 [m]: the number of steps actually taken)."""
        env = self.env
        m, H = self._count(node_rows, first_reward, self.rows), int(horizon)
        if check or node_rows is None:
            ni = self._idx(node_rows, m, self.rows, "node_rows")
        else:
            ni = torch.as_tensor(node_rows, device=env.device).reshape(-1)
            if int(ni.numel()) != m:
                raise ValueError("node_rows must have %d entries" % m)
            ni = ni.to(torch.int32).contiguous()
        if first_reward is None:
            est = torch.zeros(m, dtype=torch.float64, device=env.device)
        else:
            est = torch.as_tensor(first_reward, device=env.device).to(torch.float64).reshape(-1).clone()
            if int(est.numel()) != m:
                raise ValueError("first_reward must have %d entries" % m)
        steps = torch.zeros(m, dtype=torch.int64, device=env.device)
        if m == 0 or H <= 0:
            return est, steps
        key = (float(gamma), H)
        gpow = self._gpow.get(key)
        if gpow is None:                                             # gamma**t as python computes it (BatchedDMPEnv.evaluate)
            gpow = torch.tensor([float(gamma) ** t for t in range(H)], dtype=torch.float64).to(env.device)
            self._gpow[key] = gpow
        with torch.cuda.device(env.device):
            _lib.check(getattr(self._lib, self.EVALUATE)(C.byref(env._desc), C.byref(env._state), _ptr(self.records), self.rows, m, _ptr(ni), H,
                                                       int(t0) & 0xFFFFFFFF, _ptr(gpow), _ptr(est), _ptr(steps), env._stream()))
        return est, steps

    # ---- observation rows of records ---------------------------------------------------------------------------------
    def observe(self, node_rows=None, out=None, check=True):
        """The canonical observation rows of records (snac_observe_nodes*): row i = what env.observe() shows for a batch row holding record
        node_rows[i] (None: record i; m = out's rows, else every record), for every record, a terminal one (NEED_RESET) included.  One
        launch, the records are not changed, several i may name one record.  out: a contiguous [m, obs_dim] tensor of the env's obs_dtype
        on its device to write into.  check=False skips the range test of node_rows (a host round trip; the kernel clamps).  Enqueued on
        the env's stream.  Returns the rows [m, obs_dim]."""
        env = self.env
        if node_rows is None:
            m = self.rows if out is None else int(out.shape[0])
            ni = self._idx(None, m, self.rows, "node_rows")
        elif check:
            m = int(torch.as_tensor(node_rows).numel())
            ni = self._idx(node_rows, m, self.rows, "node_rows")
        else:
            ni = torch.as_tensor(node_rows, device=env.device).reshape(-1).to(torch.int32).contiguous()
            m = int(ni.numel())
        if out is None:
            out = torch.empty((m, env.obs_dim), dtype=env.obs_dtype, device=env.device)
        elif tuple(out.shape) != (m, env.obs_dim) or out.dtype != env.obs_dtype or out.device != env.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous [%d, %d] %s tensor on %s" % (m, env.obs_dim, env.obs_dtype, env.device))
        with torch.cuda.device(env.device):
            _lib.check(getattr(self._lib, self.OBSERVE)(C.byref(env._desc), C.byref(env._state), _ptr(self.records), self.rows, m, _ptr(ni), _ptr(out),
                                                      env._stream()))
        return out

    # ---- what a search reads of its nodes (decoded from the records: snac_env_hdr) -----------------------------------
    def _hdr16(self):
        return self.records[:, :4].contiguous().view(torch.int16).view(self.rows, 8)

    @property
    def position(self):
        h = self.records[:, 0]
        r = ((h & 0xFF) << 24) >> 24
        c = (((h >> 8) & 0xFF) << 24) >> 24
        return torch.stack([r, c], dim=1)

    @property
    def need_reset(self):
        return ((self.records[:, 0] >> 16) & _lib.FLAG_NEED_RESET) != 0

    @property
    def count_brick(self):
        return self._hdr16()[:, 2].to(torch.int32)

    @property
    def count_step(self):
        return self._hdr16()[:, 3].to(torch.int32)

    @property
    def total_brick(self):
        return self._hdr16()[:, 4].to(torch.int32)

    @property
    def plan_idx(self):
        return self._hdr16()[:, 5].to(torch.int32)


class NodePool2D(_NodePool):
    """2D node records (snac_node2d: 32 int32 words, one line)."""
    KIND, WORDS, CANONICAL_OBS = 2, _words("snac_node2d"), 51
    PACK, UNPACK, TRANSITION = "snac_nodes2d_pack", "snac_nodes2d_unpack", "snac_transition_nodes2d"
    EVALUATE, OBSERVE = "snac_evaluate_nodes2d", "snac_observe_nodes2d"

    @property
    def boards(self):
        """[rows, 20] row words of the bit boards (bit j of word q = interior cell (q, j))."""
        return self.records[:, 8:28]


class NodePool1D(_NodePool):
    """1D node records (snac_node1d: 32 int32 words, one line)."""
    KIND, WORDS, CANONICAL_OBS = 1, _words("snac_node1d"), 7
    PACK, UNPACK, TRANSITION = "snac_nodes1d_pack", "snac_nodes1d_unpack", "snac_transition_nodes1d"
    EVALUATE, OBSERVE = "snac_evaluate_nodes1d", "snac_observe_nodes1d"

    @property
    def heights(self):
        """[rows, 30] int16 heights of the interior cells (a view of the records)."""
        return self.records[:, 8:24].view(torch.int16)[:, :30]


class NodePool3D(_NodePool):
    """3D node records (snac_node3d: 224 int32 words, seven lines)."""
    KIND, WORDS, CANONICAL_OBS = 3, _words("snac_node3d"), 51
    PACK, UNPACK, TRANSITION = "snac_nodes3d_pack", "snac_nodes3d_unpack", "snac_transition_nodes3d"
    EVALUATE, OBSERVE = "snac_evaluate_nodes3d", "snac_observe_nodes3d"

    @property
    def heights(self):
        """[rows, 20, 20] int16 heights of the interior, row-major (a view of the records)."""
        return self.records[:, 8:208].view(torch.int16).view(self.rows, 20, 20)


_POOLS = {1: NodePool1D, 2: NodePool2D, 3: NodePool3D}


def NodePool(env, rows):
    """The node pool of env.kind (NodePool1D / NodePool2D / NodePool3D) with `rows` records."""
    if env.kind not in _POOLS:
        raise ValueError("unknown env kind %r" % (env.kind,))
    return _POOLS[env.kind](env, rows)
