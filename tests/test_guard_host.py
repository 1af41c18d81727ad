"""The guard-band checker of tests/guard.py, checked itself: writers made of plain torch indexing on the arena -- one that stays inside
its output, and one each that strays by one byte before, one byte after, 16 bytes after, one whole row after, or leaves an interior
byte unwritten -- and what check() / view_untouched() / unwritten() report for each, offset for offset.  On CPU tensors, and once on
the device (the same writers: no kernel of the library is involved, and none is built wrongly for this)."""
import pytest
import torch

import guard

ROWS, D = 5, 461                                                       # the largest row of any layout: 461 float64 values
ROW_BYTES = D * 8


def _arena(device, offset=0):
    arena = guard.Arena(4 * guard.BAND + 2 * ROWS * ROW_BYTES + 4096, device)
    obs = arena.carve((ROWS, D), torch.float64, offset=offset, name="obs")
    done = arena.carve((ROWS,), torch.uint8, offset=1, name="done")
    return arena, obs, done


def _span(arena, view):
    start = view.data_ptr() - arena.buf.data_ptr()
    return start, start + view.numel() * view.element_size()


def _cases(device):
    # a writer that stays inside: every byte of both outputs, nothing else
    arena, obs, done = _arena(device)
    assert obs.data_ptr() % 512 == 0 and done.data_ptr() % 512 == 1
    assert guard.unwritten(obs) == (0, ROWS * ROW_BYTES - 1)           # fresh: all of it
    guard.view_untouched(obs, "obs")
    obs.fill_(1.0)                                                     # (bytes 00, 3f, f0: none of them the fresh byte)
    done.fill_(1)
    arena.check()
    assert guard.unwritten(obs) is None and guard.unwritten(done) is None
    with pytest.raises(guard.GuardError) as e:
        guard.view_untouched(obs[1:3], "rows 1-2")
    assert e.value.first == ("rows 1-2", "inside", 0) and e.value.last == ("rows 1-2", "inside", 2 * ROW_BYTES - 1)

    # the bands are as wide as promised on both sides of both views
    s0, e0 = _span(arena, obs)
    s1, e1 = _span(arena, done)
    assert s0 >= guard.BAND and s1 - e0 >= guard.BAND and arena.buf.numel() - e1 >= guard.BAND
    assert bool((arena.buf[:s0] == guard.BAND_BYTE).all()) and bool((arena.buf[e1:] == guard.BAND_BYTE).all())

    def stray(view, name, lo, hi, want_first, want_last, text):
        """Bytes lo .. hi - 1 relative to the view's START are written; the report names them relative to the nearest view."""
        arena, obs, done = _arena(device, offset=8)
        v = {"obs": obs, "done": done}[name]
        start, _ = _span(arena, v)
        arena.buf[start + lo:start + hi] = 0x11
        with pytest.raises(guard.GuardError) as e:
            arena.check()
        assert (e.value.first, e.value.last, e.value.count) == (want_first, want_last, hi - lo), (e.value.first, e.value.last)
        assert text in str(e.value), str(e.value)

    nb = ROWS * ROW_BYTES
    stray(obs, "obs", -1, 0, ("obs", "before", -1), ("obs", "before", -1), "-1 .. -1 before `obs`")
    stray(obs, "obs", nb, nb + 1, ("obs", "after", 0), ("obs", "after", 0), "+0 .. +0 after `obs`")
    stray(done, "done", ROWS, ROWS + 1, ("done", "after", 0), ("done", "after", 0), "+0 .. +0 after `done`")
    stray(done, "done", -1, 0, ("done", "before", -1), ("done", "before", -1), "-1 .. -1 before `done`")
    stray(done, "done", ROWS + 16, ROWS + 32, ("done", "after", 16), ("done", "after", 31), "+16 .. +31 after `done`")
    stray(obs, "obs", nb + 16, nb + 32, ("obs", "after", 16), ("obs", "after", 31), "+16 .. +31 after `obs`")
    stray(obs, "obs", nb, nb + ROW_BYTES, ("obs", "after", 0), ("obs", "after", ROW_BYTES - 1), "+0 .. +%d after `obs`" % (ROW_BYTES - 1))
    # a stray write is found at the far edge of a band too
    stray(obs, "obs", -guard.BAND, -guard.BAND + 4, ("obs", "before", -guard.BAND), ("obs", "before", -guard.BAND + 3), "before `obs`")

    # a writer that stays inside but leaves one interior byte out: the bands are clean, the byte is found where it is
    arena, obs, done = _arena(device)
    flat = obs.view(torch.uint8).reshape(-1)
    flat.fill_(0x11)
    flat[2 * ROW_BYTES + 17] = guard.FRESH_BYTE
    arena.check()
    assert guard.unwritten(obs) == (2 * ROW_BYTES + 17, 2 * ROW_BYTES + 17)
    assert guard.unwritten(obs[2]) == (17, 17) and guard.unwritten(obs[3]) is None
    guard.fresh(obs[:, 3:5])                                           # a strided region made fresh again
    guard.view_untouched(obs[:, 3:5], "columns 3-4")
    assert guard.unwritten(obs[1]) == (24, 39)

    # carve() refuses an offset below the natural alignment of the type, and an arena that has no band left
    with pytest.raises(AssertionError):
        arena.carve((4,), torch.float32, offset=2)
    with pytest.raises(AssertionError):
        arena.carve((arena.buf.numel(),), torch.uint8)


_OWNER = '''
class Owner:
    """An object as the package's: it allocates in its constructor and in a call, through its module's global `torch`."""
    def __init__(self, n):
        self.stats = torch.zeros((n, 64), dtype=torch.int32, device="cpu")
        self.work = torch.empty(2 * n, dtype=torch.int32, device="cpu")
        self.bounds = torch.empty_like(torch.ones((n, 2), dtype=torch.float64))
        self.table = torch.tensor([0.0, 1.0, 2.0])
        self.rows = torch.arange(n)
        self.none = torch.full((n,), -1, dtype=torch.int32)

    def call(self, n):
        return torch.empty(n, dtype=torch.uint8)
'''


def test_on_demand_allocations_come_from_the_arena():
    import types

    mod = types.ModuleType("package.owner")
    mod.torch = torch
    exec(_OWNER, mod.__dict__)
    other = types.ModuleType("package.other")
    other.torch = torch
    exec(_OWNER, other.__dict__)
    n = 5
    arena = guard.Arena(12 * (guard.BAND + 4096), "cpu")
    lo, hi = arena.buf.data_ptr(), arena.buf.data_ptr() + arena.buf.numel()
    with guard.allocations(mod, arena=arena):
        with guard.allocations(other, arena=arena, offset=128):        # nested: two modules at once
            assert mod.torch is not torch and other.torch is not torch
            o, p = mod.Owner(n), other.Owner(n)
            done = o.call(3)
    assert mod.torch is torch and other.torch is torch
    names = [v[2] for v in arena.views]
    assert names == ["owner#0 (5, 64) int32", "owner#1 (10,) int32", "owner#2 (5, 2) float64", "other#0 (5, 64) int32", "other#1 (10,) int32",
                     "other#2 (5, 2) float64", "owner#3 (3,) uint8"], names
    for t, off in [(o.stats, 0), (o.work, 0), (o.bounds, 0), (done, 0), (p.stats, 128), (p.work, 128), (p.bounds, 128)]:
        assert lo <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= hi and t.data_ptr() % 512 == off and t.is_contiguous()
    for t in (o.table, o.rows, o.none):                                # tables and constant inputs stay torch's own
        assert not lo <= t.data_ptr() < hi
    assert o.table.tolist() == [0.0, 1.0, 2.0] and o.rows.tolist() == list(range(n)) and o.none.tolist() == [-1] * n
    assert not o.stats.any() and not p.stats.any()                     # zeros() is zeroed,
    guard.view_untouched(o.work, "work"), guard.view_untouched(o.bounds, "bounds"), guard.view_untouched(done, "done")   # empty() is fresh
    # in-bounds writes leave the bands intact
    o.stats.fill_(7), o.work.fill_(-1), o.bounds.fill_(1.5), done.fill_(1), p.stats.fill_(3)
    arena.check()
    # one byte past a view is reported against that view's name
    start, end = _span(arena, o.work)
    arena.buf[end] = 0x11
    with pytest.raises(guard.GuardError) as e:
        arena.check()
    assert e.value.first == ("owner#1 (10,) int32", "after", 0) and e.value.count == 1 and "+0 .. +0 after `owner#1 (10,) int32`" in str(e.value)
    arena.buf[end] = guard.BAND_BYTE
    start, _ = _span(arena, p.bounds)
    arena.buf[start - 1] = 0x11
    with pytest.raises(guard.GuardError) as e:
        arena.check()
    assert e.value.first == ("other#2 (5, 2) float64", "before", -1), e.value.first
    # the module's torch is restored on an exception too, and the first mode is what it was
    with pytest.raises(ZeroDivisionError):
        with guard.allocations(mod, arena=arena):
            assert mod.torch is not torch
            1 / 0
    assert mod.torch is torch
    with pytest.raises(AssertionError):
        with guard.allocations(mod):                                   # neither views nor an arena
            pass
    assert mod.torch is torch
    v = arena.carve((3,), torch.uint8, name="listed")
    with guard.allocations(mod, [v]):
        assert mod.Owner.call(None, 3) is v
    # the twin's side: torch's own tensors, empty() fresh like a carved view
    with guard.fresh_allocations(mod):
        t = mod.Owner(n)
    assert mod.torch is torch and not lo <= t.work.data_ptr() < hi and not t.stats.any()
    guard.view_untouched(t.work, "the twin's work"), guard.view_untouched(t.bounds, "the twin's bounds")


def test_the_checker_on_cpu_tensors():
    _cases("cpu")


@pytest.mark.gpu
def test_the_checker_on_the_device():
    _cases("cuda")
