"""Host: the prioritised-replay entry points (snac_prio_layout, snac_prio_init, snac_prio_update, snac_prio_fill, snac_prio_sample) are
exported, snac_prio_layout gives the layout include/snac_hip.h states ("Prioritised replay"), and every entry point checks every argument
before any HIP call -- each failing call below fails its checks first, so the placeholder pointers are never dereferenced, and an empty
job returns 0 although no device exists to launch on.  PriorityTree, SelfPlay(prioritized=), ReplayRing(prioritized=),
sample(prioritized=True) and update_priorities() reject bad arguments before they touch a device.  Last, the numpy reference the GPU tests
compare with (tests/test_gpu_prio.py): quant, the sums level by level, and the draw -- the segment arithmetic in python ints and
searchsorted over the cumulative sum -- checked here on cases computed by hand."""
import ctypes as C

import numpy as np
import pytest

from cabi_checks import ODD, PH, _err, _NoDevice
import rng_spec
from snac_amd import _lib
from test_uct_reanalyse_host import hostless_play
from test_uct_selfplay_host import hostless_search

STREAM_PRIO = 4
LIMIT = (1 << 31) - 64


# ---- the layout, restated -------------------------------------------------------------------------------------------------------------
def layout(entries):
    """(bytes, levels, offsets [0 .. levels], counts [0 .. levels]) as the header states them."""
    e64 = -(-entries // 64) * 64
    off, count = [128], [entries]
    at, n = 128 + 4 * e64, e64 // 64
    while True:
        off.append(at)
        count.append(n)
        at += 8 * (-(-n // 64) * 64)
        if n == 1:
            break
        n = -(-n // 64)
    return at, len(off) - 1, off, count


def _layout(L, entries, bytes_=True, levels=True, off=True):
    b, lv, o = C.c_int64(-1), C.c_int32(-1), (C.c_int64 * 8)(*([-1] * 8))
    rc = L.snac_prio_layout(entries, C.byref(b) if bytes_ else None, C.byref(lv) if levels else None, C.byref(o) if off else None)
    return rc, b.value, lv.value, list(o)


def _init(L, tree=PH, entries=100, s=16):
    return L.snac_prio_init(tree, entries, s, None)


def _update(L, tree=PH, entries=100, s=16, index=PH, priority=PH, n=4):
    return L.snac_prio_update(tree, entries, s, index, priority, n, None)


def _fill(L, tree=PH, entries=100, s=16, first=0, count=4, priority=1.0):
    return L.snac_prio_fill(tree, entries, s, first, count, priority, None)


def _sample(L, tree=PH, entries=100, seed=1, sampler_id=0, draw=0, n=4, stratified=1, index=PH, prob=PH, weight=PH):
    return L.snac_prio_sample(tree, entries, seed, sampler_id, draw, n, stratified, index, prob, weight, None)


def test_the_library_exports_the_prioritised_replay_entry_points():
    L = _lib.lib()
    assert L.snac_version() == _lib.ABI_VERSION == 12                # additions only
    for n, k in (("snac_prio_layout", 4), ("snac_prio_init", 4), ("snac_prio_update", 7), ("snac_prio_fill", 7), ("snac_prio_sample", 11)):
        assert n in _lib.EXPORTS
        assert getattr(L, n) is not None
        assert len(getattr(L, n).argtypes) == k


@pytest.mark.parametrize("entries,levels", [(1, 1), (63, 1), (64, 1), (65, 2), (4096, 2), (4097, 3), (262144, 3), (262145, 4), (LIMIT, 6)])
def test_the_layout_is_the_headers(entries, levels):
    L = _lib.lib()
    rc, b, lv, off = _layout(L, entries)
    want_bytes, want_levels, want_off, count = layout(entries)
    assert rc == 0 and lv == levels == want_levels
    assert off == want_off + [0] * (7 - levels) and b == want_bytes
    assert all(o % 128 == 0 for o in off) and b % 128 == 0
    assert off[0] == 128 and off[1] == 128 + 4 * (-(-entries // 64) * 64)
    assert count[levels] == 1 and all(count[l + 1] == -(-count[l] // 64) for l in range(1, levels))
    assert b == off[levels] + 8 * 64                                 # the total, padded to a group


def test_layout_validates_its_arguments():
    L = _lib.lib()
    for e in (0, -1, -(1 << 31), LIMIT + 1, (1 << 31) - 1):
        rc, b, lv, off = _layout(L, e)
        _err(L, rc, b"entries must be")
        assert (b, lv, off) == (-1, -1, [-1] * 8)                    # nothing written
    _err(L, _layout(L, 100, bytes_=False)[0], b"null output")
    _err(L, _layout(L, 100, levels=False)[0], b"null output")
    _err(L, _layout(L, 100, off=False)[0], b"null output")


def _tree_checks(L, call, scale=True):
    _err(L, call(L, tree=None), b"null tree")
    _err(L, call(L, tree=ODD), b"tree must be 128-byte")
    for e in (0, -1, -(1 << 31), LIMIT + 1, (1 << 31) - 1):
        _err(L, call(L, entries=e), b"entries must be")
    if scale:
        for s in (-1, 32, 64, -(1 << 31)):
            _err(L, call(L, s=s), b"scale_log2")


def test_init_validates_its_arguments_before_any_hip_call():
    _tree_checks(_lib.lib(), _init)


def test_update_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _tree_checks(L, _update)
    _err(L, _update(L, n=-1), b"n must be")
    _err(L, _update(L, n=-(1 << 31)), b"n must be")
    _err(L, _update(L, index=None), b"null index")
    _err(L, _update(L, priority=None), b"null priority")
    assert _update(L, n=0) == 0                                      # no entry to update: no launch
    _err(L, _update(L, n=0, index=None), b"null index")              # the checks come first
    _err(L, _update(L, n=0, priority=None), b"null priority")
    _err(L, _update(L, n=0, s=32), b"scale_log2")
    _err(L, _update(L, n=0, tree=ODD), b"128-byte")


def test_fill_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _tree_checks(L, _fill)
    _err(L, _fill(L, first=-1), b"first must be")
    _err(L, _fill(L, first=100, count=0), b"first must be")
    _err(L, _fill(L, count=-1), b"count must be")
    _err(L, _fill(L, first=97, count=4), b"count must be")           # it does not wrap
    _err(L, _fill(L, count=101), b"count must be")
    _err(L, _fill(L, entries=LIMIT, first=LIMIT - 1, count=2), b"count must be")
    _err(L, _fill(L, priority=float("nan")), b"NaN")
    for p in (1.0, 0.0, -1.0, float("inf")):
        assert _fill(L, count=0, priority=p) == 0                    # no entry to set: no launch
    assert _fill(L, first=99, count=0) == 0
    _err(L, _fill(L, count=0, priority=float("nan")), b"NaN")        # the checks come first
    _err(L, _fill(L, count=0, first=100), b"first must be")
    _err(L, _fill(L, count=0, s=-1), b"scale_log2")


def test_sample_validates_its_arguments_before_any_hip_call():
    L = _lib.lib()
    _tree_checks(L, _sample, scale=False)
    _err(L, _sample(L, draw=-1), b"draw must be")
    _err(L, _sample(L, draw=-(1 << 31)), b"draw must be")
    _err(L, _sample(L, n=-1), b"n must be")
    _err(L, _sample(L, index=None), b"null index")
    _err(L, _sample(L, prob=None), b"null prob")
    assert _sample(L, n=0) == 0                                      # no sample to draw: no launch
    assert _sample(L, n=0, weight=None, draw=0x7FFFFFFF, stratified=0, seed=(1 << 64) - 1) == 0
    _err(L, _sample(L, n=0, prob=None), b"null prob")                # the checks come first
    _err(L, _sample(L, n=0, draw=-1), b"draw must be")


# ---- the python layer -----------------------------------------------------------------------------------------------------------------
def _tree(entries=100, draw=0):
    """A PriorityTree that was never constructed on a device: the attributes its methods check, nothing else."""
    import torch

    from snac_amd.priority import PriorityTree

    t = object.__new__(PriorityTree)
    t.entries, t.scale_log2, t.seed, t.sampler_id, t.draw, t.levels = entries, 16, 1, 0, draw, 2
    t.device = torch.device("cuda", 0)
    return t


def test_priority_tree_rejects_bad_arguments_before_touching_a_device():
    import torch

    from snac_amd.priority import PriorityTree

    for e in (0, -1, LIMIT + 1, 2.0, "8", True, None):
        with pytest.raises(ValueError, match="entries"):
            PriorityTree(e, "cuda:0")
    for s in (-1, 32, 1.5, True, None):
        with pytest.raises(ValueError, match="scale_log2"):
            PriorityTree(8, "cuda:0", scale_log2=s)
    for seed in (1 << 64, 0.5, None):
        with pytest.raises(ValueError, match="seed"):
            PriorityTree(8, "cuda:0", seed=seed)
    for sid in (-1, 1 << 62, 0.5):
        with pytest.raises(ValueError, match="sampler_id"):
            PriorityTree(8, "cuda:0", sampler_id=sid)
    with pytest.raises(ValueError, match="cuda device"):
        PriorityTree(8, "cpu")
    t = _tree()
    ok_i, ok_p = torch.zeros(4, dtype=torch.int64), torch.zeros(4)   # on the host: the right shapes on the wrong device
    for idx in ([0, 1], np.zeros(4, np.int64), torch.zeros((2, 2), dtype=torch.int64), torch.zeros(4), torch.zeros(4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="index"):
            t.update(idx, ok_p)
    with pytest.raises(ValueError, match="index must be on"):
        t.update(ok_i, ok_p)
    t.device = torch.device("cpu")                                   # so that the placeholders pass the device check
    for pri in ([0.0] * 4, torch.zeros(3), torch.zeros((4, 1)), torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="priority"):
            t.update(ok_i, pri)
    t = _tree()
    for first in (-1, 100, 1.0, None):
        with pytest.raises(ValueError, match="first"):
            t.fill(first, 1)
    for first, count in ((0, -1), (0, 101), (97, 4), (0, 2.0)):
        with pytest.raises(ValueError, match="count"):
            t.fill(first, count)
    for p in (-1.0, -1e-30, float("nan")):
        with pytest.raises(ValueError, match="priority"):
            t.fill(0, 4, p)
    for n in (-1, 1 << 31, 2.5, None):
        with pytest.raises(ValueError, match="n must be"):
            t.sample(n)
    for st in (1, 0, None):
        with pytest.raises(ValueError, match="stratified"):
            t.sample(4, stratified=st)
    with pytest.raises(ValueError, match="2\\^31 times"):
        _tree(draw=1 << 31).sample(4)                                # draw would reach 2^31
    with pytest.raises(ValueError, match="l must be"):
        t.level(3)


def test_selfplay_rejects_bad_priority_arguments_before_touching_a_device():
    import torch

    from snac_amd import SelfPlay

    for p in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="prioritized"):
            SelfPlay(hostless_search(), 8, prioritized=p)
    for s in (-1, 32, 1.5, True):
        with pytest.raises(ValueError, match="priority_scale_log2"):
            SelfPlay(hostless_search(), 8, prioritized=True, priority_scale_log2=s)
    p = hostless_play()
    p.tree = None                                                    # a ring built without a tree
    with pytest.raises(ValueError, match="prioritized=True needs the priority tree"):
        p.sample(4, prioritized=True)
    with pytest.raises(ValueError, match="prioritized must be a bool"):
        p.sample(4, prioritized=1)
    with pytest.raises(ValueError, match="needs the priority tree"):
        p.update_priorities(torch.zeros(4, dtype=torch.int64), torch.zeros(4))
    with pytest.raises(ValueError, match="prioritized=True needs the priority tree"):
        p.reanalyse(p.search, 4, prioritized=True)
    with pytest.raises(ValueError, match="prioritized must be a bool"):
        p.reanalyse(p.search, 4, prioritized=None)
    p.tree = _tree(32)
    with pytest.raises(ValueError, match="index must be None"):
        p.reanalyse(p.search, 4, index=torch.zeros(4, dtype=torch.int64), prioritized=True)
    with pytest.raises(ValueError, match="generator"):
        p.sample(4, prioritized=True, generator=torch.Generator())
    for beta in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta"):
            p.sample(4, prioritized=True, beta=beta)
    with pytest.raises(ValueError, match="index"):
        p.update_priorities([0, 1], torch.zeros(2))
    with pytest.raises(ValueError, match="must be on"):
        p.update_priorities(torch.zeros(2, dtype=torch.int64), torch.zeros(2))


def _ring(tree, ticks=8, cap=4, head=0):
    """A ReplayRing that was never constructed on a device: the attributes sample() and update_priorities() check."""
    from snac_amd import ReplayRing

    r = object.__new__(ReplayRing)
    r.env, r.cap, r.ticks, r.head, r.tree = _NoDevice(num_envs=4), cap, ticks, head, tree
    return r


def test_replay_ring_rejects_bad_priority_arguments_before_touching_a_device():
    import torch

    from snac_amd import ReplayRing

    for p in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="prioritized"):
            ReplayRing(_NoDevice(num_envs=4), 8, prioritized=p)
    for s in (-1, 32, 1.5, True):
        with pytest.raises(ValueError, match="priority_scale_log2"):
            ReplayRing(_NoDevice(num_envs=4), 8, prioritized=True, priority_scale_log2=s)
    r = _ring(None)
    with pytest.raises(ValueError, match="prioritized=True needs the priority tree"):
        r.sample(4, prioritized=True)
    with pytest.raises(ValueError, match="prioritized must be a bool"):
        r.sample(4, prioritized="yes")
    with pytest.raises(ValueError, match="needs the priority tree"):
        r.update_priorities(torch.zeros(4, dtype=torch.int64), torch.zeros(4))
    r = _ring(_tree(16))
    with pytest.raises(ValueError, match="generator"):
        r.sample(4, prioritized=True, generator=torch.Generator())
    for beta in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta"):
            r.sample(4, prioritized=True, beta=beta)
    for idx in ([0, 1], torch.zeros(2), torch.zeros(2, dtype=torch.bool)):
        with pytest.raises(ValueError, match="index"):
            r.update_priorities(idx, torch.zeros(2))
    with pytest.raises(ValueError, match="must be on"):
        r.update_priorities(torch.zeros(2, dtype=torch.int64), torch.zeros(2))


# ---- the reference, in numpy ----------------------------------------------------------------------------------------------------------
def quant(p, s):
    """quant(p, s) of the header for a float32 array -> uint32 weights."""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.rint(p.astype(np.float64) * np.float64(2.0 ** s))     # exact multiply, round half to even
        w = np.clip(x, 1.0, 4294967295.0)
    w = np.where(np.isnan(p) | (p < 0), 1.0, w)
    w = np.where(p == 0, 0.0, w)
    return w.astype(np.uint32)


def apply_update(w, index, priority, s):
    """snac_prio_update on the leaves w (uint32 [entries], in place): out-of-range indices skipped, the largest duplicate wins.
    Returns the largest weight stored (0: none)."""
    q = quant(priority, s)
    ok = (index >= 0) & (index < len(w))
    w[index[ok]] = 0
    np.maximum.at(w, index[ok], q[ok])
    return int(q[ok].max()) if ok.any() else 0


def level_sums(w):
    """The sum levels of leaves w, each padded to whole groups of 64: [level 1, ..., the total] as uint64 arrays."""
    cur = np.zeros(-(-len(w) // 64) * 64, np.uint64)
    cur[:len(w)] = w
    out = []
    while True:
        n = len(cur) // 64
        nxt = np.zeros(-(-n // 64) * 64, np.uint64)
        nxt[:n] = cur.reshape(n, 64).sum(axis=1, dtype=np.uint64)
        out.append(nxt)
        if n == 1:
            return out
        cur = nxt


def positions(T, n, seed, sampler_id, draw, stratified):
    """u of samples 0 .. n - 1, in python ints: the header's segment arithmetic on stream 4's words."""
    j = np.arange(n, dtype=np.uint64) + np.uint64(sampler_id)
    hi = rng_spec.words(seed, STREAM_PRIO, j, np.uint64(2 * draw))
    lo = rng_spec.words(seed, STREAM_PRIO, j, np.uint64(2 * draw + 1))
    q, rem = divmod(T, n)
    out = []
    for k in range(n):
        r = (int(hi[k]) << 32) | int(lo[k])
        if stratified and q >= 1:
            out.append(k * q + min(k, rem) + ((r * (q + (1 if k < rem else 0))) >> 64))
        else:
            out.append((r * T) >> 64)
    return out


def draw_at(w, u):
    """(index, prob, weight) of the positions u: the lowest i with w_0 + ... + w_i > u."""
    c = np.cumsum(w, dtype=np.uint64)
    T = int(c[-1])
    if T == 0:
        n = len(u)
        return np.full(n, -1, np.int64), np.zeros(n, np.float32), np.zeros(n, np.uint32)
    i = np.searchsorted(c, np.asarray(u, np.uint64), "right")
    wi = w[i]
    return i.astype(np.int64), (wi.astype(np.float64) / np.float64(T)).astype(np.float32), wi.astype(np.uint32)


def sample(w, n, seed, sampler_id, draw, stratified):
    """snac_prio_sample on the leaves w."""
    T = int(np.asarray(w, np.uint64).sum(dtype=np.uint64))
    return draw_at(np.asarray(w, np.uint32), positions(T, n, seed, sampler_id, draw, stratified) if T else [0] * n)


def test_quant_by_hand():
    p = np.array([0.0, -0.0, 1.0, 0.5, 1e-9, 1e9, np.nan, -1.0, -np.inf, np.inf, 2.5 / 65536, 3.5 / 65536, 65535.99999], np.float32)
    assert quant(p, 16).tolist() == [0, 0, 65536, 32768, 1, 4294967295, 1, 1, 1, 4294967295, 2, 4, 4294967295]
    assert quant(p[:6], 0).tolist() == [0, 0, 1, 1, 1, 1000000000]   # 0.5 rounds to even 0, then at least 1
    assert quant(np.float32([1.0, 1.9999999]), 31).tolist() == [1 << 31, 4294967040]


def test_the_draw_by_hand():
    w = np.array([0, 3, 0, 5], np.uint32)
    idx, prob, wt = draw_at(w, list(range(8)))
    assert idx.tolist() == [1, 1, 1, 3, 3, 3, 3, 3]
    assert wt.tolist() == [3, 3, 3, 5, 5, 5, 5, 5]
    assert prob.tolist() == [np.float32(3 / 8)] * 3 + [np.float32(5 / 8)] * 5
    assert draw_at(np.zeros(4, np.uint32), [0, 0])[0].tolist() == [-1, -1]
    assert [int(x[0]) for x in level_sums(w)] == [8]
    big = np.full(4097, 0xFFFFFFFF, np.uint32)
    lv = level_sums(big)
    assert [len(x) for x in lv] == [128, 64, 64] and int(lv[2][0]) == 4097 * 0xFFFFFFFF and int(lv[0][64]) == 0xFFFFFFFF and int(lv[1][1]) == 0xFFFFFFFF


def test_the_segments_tile_the_total():
    for T, n in ((8, 3), (8, 8), (1000003, 7), (5, 7), ((1 << 63) - 1, 1000)):
        for stratified in (True, False):
            u = positions(T, n, 9, 5, 3, stratified)
            assert all(0 <= x < T for x in u)
            q, rem = divmod(T, n)
            if stratified and q >= 1:                                # draw j inside segment j, and the segments tile [0, T)
                lo = [j * q + min(j, rem) for j in range(n + 1)]
                assert lo[0] == 0 and lo[n] == T and all(lo[j] <= u[j] < lo[j + 1] for j in range(n))
    assert positions(1000, 4, 9, 5, 3, True) == positions(1000, 4, 9, 5, 3, True)
    assert positions(1000, 4, 9, 5, 3, True) != positions(1000, 4, 9, 5, 4, True)
    assert positions(1 << 40, 4, 9, 5, 3, False)[1:] == positions(1 << 40, 3, 9, 6, 3, False)    # sample j is keyed by sampler_id + j
