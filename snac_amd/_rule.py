"""What the wrappers of the units on device tensors share (SoftValue, PPOLoss, CategoricalSupport; PriorityTree its device part): the
device they are bound to, the stream they launch on, how a launch reaches that device, and the checks of a tensor a kernel reads or
writes.  Private: nothing here is exported."""
import ctypes as C

import torch

from . import _lib

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # the handle without building a Stream object, as BatchedDMPEnv takes it


def cuda_device(device, holds):
    """`device` as torch.device("cuda", index); `holds`: what lives there, for the refusal of any other device."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("device must be a cuda device: %s in device memory" % holds)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class OnDevice:
    """self.device (a cuda_device()) and, where there is one, self.env: the stream and the launch."""
    env = None

    def _stream(self):
        if self.env is not None:
            return self.env._current_stream()
        if _raw_stream is not None:
            return C.c_void_p(_raw_stream(self.device.index))
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _launch(self, fn, *args):
        """fn(*args, stream) on self.device, on its current stream.  The context manager is entered only where the device is not the
        current one already: it costs several microseconds of a call that takes ten."""
        stream = self._stream()
        if torch.cuda.current_device() == self.device.index:
            return _lib.check(fn(*args, stream))
        with torch.cuda.device(self.device):
            _lib.check(fn(*args, stream))


class Rule(OnDevice):
    """A unit on rows of num_actions scores.  The constructor does not touch the device."""

    def __init__(self, num_actions, device, holds):
        """num_actions: 3, 5 or 8, or a BatchedDMPEnv, whose num_actions, device and stream are then taken; device: a cuda device (not
        with an env); holds: see cuda_device()."""
        if hasattr(num_actions, "num_actions") and hasattr(num_actions, "device"):
            if device is not None:
                raise ValueError("device is the env's when an env is given")
            self.env, device, num_actions = num_actions, num_actions.device, num_actions.num_actions
        if isinstance(num_actions, bool) or not isinstance(num_actions, int) or num_actions not in (3, 5, 8):
            raise ValueError("num_actions must be 3, 5 or 8 (or a BatchedDMPEnv)")
        if device is None:
            raise ValueError("device must be given (or an env)")
        self.device = cuda_device(device, holds)
        self.num_actions = num_actions
        self._lib = _lib.lib()
        self._bad = None                                             # made on first use

    def _bad_rows(self):
        """What a class's bad_rows property returns; each class gives the property its own words for what is counted."""
        if self._bad is None:
            self._bad = torch.zeros((1,), dtype=torch.int32, device=self.device)
        return self._bad

    def _check(self, t, shape, what, dtype=torch.float32):
        """`t` is what the kernel reads or writes: a contiguous tensor of `dtype` and `shape` (None: any size) on the device."""
        def shown():
            return "(%s)" % ", ".join("B" if s is None else str(s) for s in shape) if len(shape) > 1 else "(%s,)" % ("B" if shape[0] is None else shape[0])
        if not torch.is_tensor(t) or t.dtype != dtype or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (what, dtype, shown(), self.device))
        if t.dim() != len(shape) or any(s is not None and g != s for g, s in zip(t.shape, shape)) or t.shape[0] < 1:
            raise ValueError("%s must have shape %s, got %s" % (what, shown(), tuple(t.shape)))
        if t.device != self.device:
            raise ValueError("%s must be on %s" % (what, self.device))
        return t
