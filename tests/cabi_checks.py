"""What the host tests of the C ABI's argument checks share.  Every failing call fails its checks before any HIP call, so the placeholder
pointers are never dereferenced; and the Python surface rejects its arguments before it touches a device, so the stand-in envs below
fail the test when anything else of them is read.  The helpers keep the names the test files call them by; _err takes any of several
words and expects -1, _err_code takes the return code and one word."""
import ctypes as C

PH = C.c_void_p(1 << 20)                                             # a 128-byte aligned placeholder: never dereferenced
ODD = C.c_void_p((1 << 20) + 64)                                     # 64-byte aligned only


def _err(L, rc, *words):
    """The call returned -1 and the message holds one of `words`."""
    assert rc == -1, rc
    msg = L.snac_last_error()
    assert any(w in msg for w in words), msg


def _err_code(L, rc, code, word):
    """The call returned `code` and the message holds `word`."""
    assert rc == code, (rc, L.snac_last_error())
    assert word in L.snac_last_error(), L.snac_last_error()


def _desc(kind, n=16, frame_value=0):
    from snac_amd import _lib

    return _lib.EnvDesc(kind, 1, n, 4, 0, 0, 1, 0, 0, 0, frame_value, 0, 0, 0)


def _net(dims=(51, 64, 6), w=None, b=None, layers=None):
    """A network descriptor of placeholder pointers, or of the given ones."""
    from snac_amd import _lib

    net = _lib.Mlp()
    net.layers = len(dims) - 1 if layers is None else layers
    for l, d in enumerate(dims[:5]):
        net.dim[l] = d
    for l in range(min(4, len(dims) - 1)):
        net.w[l] = (1 << 20) if w is None else w[l]
        net.b[l] = (1 << 20) if b is None else b[l]
    return net


class _NoDevice:
    """Enough of an env to reach the argument checks; touching anything else is the failure the tests look for."""

    def __init__(self, **have):
        self.__dict__.update(have)

    def __getattr__(self, name):
        raise AssertionError("env.%s was touched before the arguments were rejected" % name)


class _NoDeviceOfFour:
    """Enough of an env for UCTSearch to reach its argument checks; touching anything else is the failure the test looks for."""
    num_envs = 4

    def __getattr__(self, name):
        raise AssertionError("UCTSearch touched env.%s before it rejected its arguments" % name)


def _fn(obs):
    """An evaluator for searches that must be refused before they evaluate anything."""
    raise AssertionError("the evaluator was called")
