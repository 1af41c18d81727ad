"""PriorityTree: prioritised replay on the device (include/snac_hip.h, "Prioritised replay"; snac_amd/csrc/k_prio.hip).

A 64-ary sum tree of integer weights in one device buffer.  An entry is drawn with probability weight / total; update(), fill() and
sample() cost O(log64 entries) per item, enqueue a handful of small launches on the current stream and never wait for the device.
The weights are uint32 (quant(p) = rint(p * 2^scale_log2), at least 1 for p > 0, 0 for p == 0) and every sum is a uint64, so the
tree's contents, the draws and the probabilities are the same bits whatever order the updates arrived in:

    tree = PriorityTree(capacity, device="cuda:0", seed=1)
    tree.fill(first, count)                          # new transitions: the largest priority seen so far
    index, prob = tree.sample(1024)                  # int64 [1024], float32 [1024]; stratified over the total
    weight = (len_ring * prob) ** -beta; weight /= weight.max()
    tree.update(index, td_error.abs() ** alpha)      # alpha is the caller's

SelfPlay(prioritized=True) and ReplayRing(prioritized=True) keep one behind their rings.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import ptr as _ptr
from ._rule import OnDevice, cuda_device

MAX_ENTRIES = (1 << 31) - 64
MAX_DRAWS = 1 << 31


def layout(entries):
    """snac_prio_layout -> (bytes, levels, level_offset[0 .. levels]): [0] the leaves, [l] sum level l, bytes from the buffer's start."""
    b, lv, off = C.c_int64(), C.c_int32(), (C.c_int64 * 8)()
    _lib.check(_lib.lib().snac_prio_layout(int(entries), C.byref(b), C.byref(lv), C.byref(off)))
    return b.value, lv.value, list(off)[:lv.value + 1]


def _int(name, x, lo, hi):
    if isinstance(x, bool) or not isinstance(x, int) or not lo <= x <= hi:
        raise ValueError("%s must be an integer in [%d, %d]" % (name, lo, hi))
    return x


class PriorityTree(OnDevice):
    def __init__(self, entries, device, scale_log2=16, seed=0, sampler_id=0):
        """entries: 1 .. 2^31 - 64; device: a cuda device; scale_log2: 0 .. 31, a priority's weight is rint(priority * 2^scale_log2);
        seed, sampler_id: the counter RNG's (stream 4): sample j of the tree's d-th sample() draws with (seed, sampler_id + j, d).
        Every entry starts with weight 0: nothing can be drawn before an update() or a fill()."""
        self.entries = _int("entries", entries, 1, MAX_ENTRIES)
        self.scale_log2 = _int("scale_log2", scale_log2, 0, 31)
        self.seed = _int("seed", seed, -(1 << 63), (1 << 64) - 1) & 0xFFFFFFFFFFFFFFFF
        self.sampler_id = _int("sampler_id", sampler_id, 0, (1 << 62) - 1)
        self.device = cuda_device(device, "the tree lives")
        self.draw = 0                                                # sample() calls so far
        self._lib = _lib.lib()
        self.bytes, self.levels, self.level_offset = layout(self.entries)
        self.buffer = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)
        assert self.buffer.data_ptr() % 128 == 0
        self._tree = (_ptr(self.buffer), self.entries)
        self._launch(self._lib.snac_prio_init, *self._tree, self.scale_log2)

    def _on_device(self, name, t, dtype, n=None):
        if not torch.is_tensor(t) or t.dim() != 1 or (n is not None and int(t.numel()) != n):
            raise ValueError("%s must be a 1-D tensor%s" % (name, "" if n is None else " of %d entries" % n))
        if dtype.is_floating_point != t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError("%s must hold %s" % (name, "floats" if dtype.is_floating_point else "integers"))
        if t.device != self.device:
            raise ValueError("%s must be on %s" % (name, self.device))
        return t.to(dtype).contiguous()

    def update(self, index, priority):
        """Entries index [n] (an integer tensor on the tree's device; entries outside [0, entries) are skipped) get the priorities
        [n] (floats; NaN and negatives read as the smallest weight).  Where an index repeats, the largest priority wins."""
        if not torch.is_tensor(index) or index.dim() != 1:
            raise ValueError("index must be a 1-D tensor")
        idx = self._on_device("index", index, torch.int32)
        pri = self._on_device("priority", priority, torch.float32, int(idx.numel()))
        if idx.numel() == 0:                                         # an empty tensor has no address to hand over
            return
        self._launch(self._lib.snac_prio_update, *self._tree, self.scale_log2, _ptr(idx), _ptr(pri), int(idx.numel()))

    def fill(self, first, count, priority=None):
        """Entries [first, first + count) get one priority; None: the largest weight any update() has stored (1.0 before the first),
        read on the device.  The span does not wrap."""
        first = _int("first", first, 0, self.entries - 1)
        count = _int("count", count, 0, self.entries - first)
        p = -1.0
        if priority is not None:
            p = float(priority)
            if p != p or p < 0:
                raise ValueError("priority must be None or a number >= 0")
        self._launch(self._lib.snac_prio_fill, *self._tree, self.scale_log2, first, count, p)

    def sample(self, n, stratified=True, with_weight=False):
        """n draws with replacement -> (index int64 [n], prob float32 [n]) on the device; with_weight=True: and the entries' integer
        weights (int64 [n]).  stratified: draw j from the j-th of n equal segments of the total.  An empty tree (total 0) gives
        index -1 and prob 0.  Every call uses the next value of the host-side `draw` counter."""
        n = _int("n", n, 0, 0x7FFFFFFF)
        if not isinstance(stratified, bool):
            raise ValueError("stratified must be a bool")
        if self.draw >= MAX_DRAWS:
            raise ValueError("the tree has drawn 2^31 times: build a new one with another seed or sampler_id")
        idx = torch.empty(n, dtype=torch.int32, device=self.device)
        prob = torch.empty(n, dtype=torch.float32, device=self.device)
        w = torch.empty(n, dtype=torch.int32, device=self.device) if with_weight else None
        if n:                                                        # (empty tensors have no address to hand over)
            self._launch(self._lib.snac_prio_sample, *self._tree, self.seed, self.sampler_id, self.draw, n, int(stratified), _ptr(idx), _ptr(prob),
                         _ptr(w))
        self.draw += 1
        if with_weight:
            return idx.long(), prob, w.long() & 0xFFFFFFFF
        return idx.long(), prob

    def weights(self):
        """The leaves: a uint32 [entries] view of the buffer."""
        return self.buffer[self.level_offset[0]:self.level_offset[0] + 4 * self.entries].view(torch.uint32)

    def level(self, l):
        """Sum level l in 1 .. levels with its padding: an int64 view of the buffer (the sums are below 2^63)."""
        l = _int("l", l, 1, self.levels)
        n, at = self.entries, self.level_offset[l]
        for _ in range(l):
            n = (n + 63) // 64
        return self.buffer[at:at + 8 * ((n + 63) // 64 * 64)].view(torch.int64)

    def head(self):
        """The head's first three words (max_weight, entries, levels) as python ints: a host read, for tests and logs."""
        return [int(x) for x in self.buffer[:24].view(torch.int64).cpu()]

    def total(self):
        """The sum of all weights: a host read, for tests and logs."""
        return int(self.level(self.levels)[0].cpu())

    def max_priority(self):
        """The largest priority any update() has stored (1.0 before the first): a host read, for tests and logs."""
        return self.head()[0] / float(1 << self.scale_log2)
