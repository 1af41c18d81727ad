"""Guard bands round the outputs of a call: one arena of bytes the test owns, every output carved out of it with a band on both sides.
A stray store of a kernel then lands in memory of the test -- it cannot fault -- and check() finds it.  A plain helper: no fixtures.

    arena = Arena(nbytes, device)                        one uint8 tensor, every byte BAND_BYTE (0xA5)
    view = arena.carve(shape, dtype, offset=0, name=..)  a contiguous view `offset` bytes past an `align`-aligned address, its bytes FRESH (0x5A)
    arena.check()                                        every byte outside the carved views is still 0xA5, or GuardError
    view_untouched(view)                                 every byte of a (sub)view is still 0x5A, or GuardError

Offsets in a report count from the nearest view: "+0 after `done`" is the first byte past its end, "-1 before `done`" the last byte
before its start; "+16 .. +31 after `done`" a run of 16 bytes that begins 16 bytes past its end.
"""
import contextlib
import math

import torch

# The width of a band, derived (not measured): the largest row any layout produces is 461 float64 values = 3688 bytes, and one store
# instruction of a wave covers 64 lanes x 16 bytes = 1024 bytes.  64 KiB hold more than 16 of the largest rows (17.7) and 64 wave-wide
# stores: a row index that is +1 .. +16 rows off, and a wrong count of 16-byte pieces for a whole tile, both land inside the band.
BAND = 64 * 1024
BAND_BYTE, FRESH_BYTE = 0xA5, 0x5A
_MAX_ALIGN = 4096


class GuardError(AssertionError):
    """first / last: (name of the nearest view, "before" | "after" | "inside", byte offset as in the module's docstring)."""

    def __init__(self, msg, first, last, count):
        super().__init__(msg)
        self.first, self.last, self.count = first, last, count


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


class Arena:
    def __init__(self, nbytes, device="cpu"):
        self.raw = torch.full((int(nbytes) + _MAX_ALIGN,), BAND_BYTE, dtype=torch.uint8, device=device)
        pad = (-self.raw.data_ptr()) % _MAX_ALIGN
        self.buf = self.raw[pad:pad + int(nbytes)]                     # starts on a 4096-byte boundary
        self.outside = torch.ones(int(nbytes), dtype=torch.bool, device=device)   # True: a band byte
        self.views = []                                                # (start, end, name), in address order
        self.cursor = 0

    def carve(self, shape, dtype, offset=0, align=512, name=None):
        """A contiguous `dtype` view of `shape` whose first byte lies `offset` bytes past an `align`-aligned address, at least BAND bytes
        of the arena on both sides of it, filled with FRESH_BYTE.  `offset` is a multiple of the element size: a view is never less
        aligned than its type."""
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        size, nbytes = _itemsize(dtype), _itemsize(dtype) * math.prod(shape)
        assert align >= size and _MAX_ALIGN % align == 0 and offset % size == 0 and 0 <= offset < align, (align, offset, dtype)
        start = -(-(self.cursor + BAND) // align) * align + offset
        end = start + nbytes
        assert end + BAND <= self.buf.numel(), "arena too small: %d bytes needed, %d held" % (end + BAND, self.buf.numel())
        self.buf[start:end] = FRESH_BYTE
        self.outside[start:end] = False
        self.views.append((start, end, name or "view%d" % len(self.views)))
        self.cursor = end
        view = self.buf[start:end].view(dtype).view(shape)
        assert view.data_ptr() % align == offset and view.is_contiguous()
        return view

    def _where(self, p):
        """Byte p of the arena relative to the nearest view."""
        best = None
        for start, end, name in self.views:
            if start <= p < end:
                return (name, "inside", p - start)
            cand = (start - p, name, "before", p - start) if p < start else (p - end + 1, name, "after", p - end)
            if best is None or cand[0] < best[0]:
                best = cand
        return best[1:] if best else ("arena", "inside", p)

    def check(self):
        """Every byte outside the carved views is still BAND_BYTE."""
        bad = torch.nonzero((self.buf != BAND_BYTE) & self.outside).reshape(-1)
        if bad.numel() == 0:
            return
        first, last = self._where(int(bad[0])), self._where(int(bad[-1]))
        if first[:2] == last[:2]:
            text = "%+d .. %+d %s `%s`" % (first[2], last[2], first[1], first[0])
        else:
            text = "%+d %s `%s` .. %+d %s `%s`" % (first[2], first[1], first[0], last[2], last[1], last[0])
        raise GuardError("%d byte(s) written outside every output: %s" % (bad.numel(), text), first, last, int(bad.numel()))


def fresh(view):
    """Fill a (sub)view with FRESH_BYTE again, whatever its dtype."""
    if view.is_contiguous():
        view.view(torch.uint8).fill_(FRESH_BYTE)
    else:
        view.copy_(torch.full((view.numel() * view.element_size(),), FRESH_BYTE, dtype=torch.uint8, device=view.device).view(view.dtype).view(view.shape))
    return view


def view_untouched(view, name="view"):
    """Every byte of the region is still FRESH_BYTE: nothing wrote it.  `view` may be a strided slice of a carved view."""
    flat = view.contiguous().view(torch.uint8).reshape(-1)
    bad = torch.nonzero(flat != FRESH_BYTE).reshape(-1)
    if bad.numel():
        first, last = (name, "inside", int(bad[0])), (name, "inside", int(bad[-1]))
        raise GuardError("%d byte(s) of `%s` were written (it is documented as not written): %+d .. %+d inside it, of %d bytes"
                         % (bad.numel(), name, first[2], last[2], flat.numel()), first, last, int(bad.numel()))


def unwritten(view):
    """The bytes of a view that still hold FRESH_BYTE, as (first, last) byte offsets inside it, or None: what a writer left out.  (A
    written byte may be 0x5A by chance; the tests compare the written bytes with a reference and use this for the report.)"""
    flat = view.contiguous().view(torch.uint8).reshape(-1)
    idx = torch.nonzero(flat == FRESH_BYTE).reshape(-1)
    return None if idx.numel() == 0 else (int(idx[0]), int(idx[-1]))


@contextlib.contextmanager
def allocations(module, views=None, arena=None, offset=None):
    """Inside: torch.empty / torch.empty_like / torch.zeros called from `module` (one of the package's, through its global `torch`) come
    from the test's arena; every other attribute of torch is torch's (torch.tensor, torch.full, torch.arange: tables and constant inputs).
    Several modules are patched at once by nesting the context.  Two modes:

    allocations(module, views): the calls return `views` in turn -- shape and dtype must match; zeros() zeroes the view.  The outputs that
    a call allocates itself then come from the arena, and the call stays the package's own.

    allocations(module, arena=A, offset=None): on demand -- every such call is carved from A as it is made, `offset` bytes (None: 0; a
    multiple of 128 below 512, so that records, statistics and bounds keep the alignment the header asks for) past a 512-byte boundary,
    zeros() zeroed, named "<module>#<k> <shape> <dtype>" with k counting the module's allocations from this arena.  For objects that
    allocate in their constructors and keep raw pointers: build them, and call them, inside the context."""
    assert (views is None) != (arena is None), "give the views in call order, or an arena to carve from on demand"
    queue = list(views) if views is not None else None
    short = module.__name__.rsplit(".", 1)[-1]
    count = None if arena is None else arena.__dict__.setdefault("allocated", {})      # per arena and module: names stay unique across contexts
    off = 0 if offset is None else int(offset)
    assert off % 128 == 0 and 0 <= off < 512, off

    def take(shape, dtype):
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        dtype = torch.get_default_dtype() if dtype is None else dtype
        if queue is None:
            k = count[short] = count.get(short, -1) + 1
            name = "%s#%d %s %s" % (short, k, shape, str(dtype).replace("torch.", ""))
            return arena.carve(shape, dtype, offset=off, name=name)
        v = queue.pop(0)
        assert tuple(v.shape) == shape and v.dtype == dtype, ("the call allocates", shape, dtype, "the test carved", tuple(v.shape), v.dtype)
        return v

    class Proxy:
        def __getattr__(self, name):
            return getattr(torch, name)

        def empty(self, shape, dtype=None, device=None):
            return take(shape, dtype)

        def empty_like(self, t):
            return take(t.shape, t.dtype)

        def zeros(self, shape, dtype=None, device=None):
            return take(shape, dtype).zero_()

    assert module.torch is torch
    module.torch = Proxy()
    try:
        yield
    finally:
        module.torch = torch
    assert not queue, "the call allocated fewer outputs than the test carved"


@contextlib.contextmanager
def fresh_allocations(module):
    """The twin's side of the on-demand mode: torch's own tensors, but what torch.empty / torch.empty_like give is filled with FRESH_BYTE as
    a carved view is, so that a byte neither object ever writes (the tail of a work array) compares equal between the two."""
    class Proxy:
        def __getattr__(self, name):
            return getattr(torch, name)

        def empty(self, *a, **kw):
            return fresh(torch.empty(*a, **kw))

        def empty_like(self, *a, **kw):
            return fresh(torch.empty_like(*a, **kw))

    assert module.torch is torch
    module.torch = Proxy()
    try:
        yield
    finally:
        module.torch = torch
