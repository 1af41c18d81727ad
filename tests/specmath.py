"""The arithmetic steps of include/snac_hip.h that several rule restatements build on, in numpy -- every ufunc call below is one float64
operation, rounded on its own: EXP and LOG ("Acting from a policy"), the two-stage batch sum of the losses and the xor butterfly of the
optimiser's sum of squares -- and the byte comparison of a kernel's floats with a rule's."""
import math

import numpy as np

LOG2E, LN2_HI, LN2_LO = float.fromhex("0x1.71547652b82fep+0"), float.fromhex("0x1.62e42feep-1"), float.fromhex("0x1.a39ef35793c76p-33")
SQRT_HALF = float.fromhex("0x1.6a09e667f3bcdp-1")
EXP_C = [np.float64(1.0) / np.float64(math.factorial(n)) for n in range(14)]
LOG_D = [np.float64(1.0) / np.float64(2 * n + 1) for n in range(11)]


def spec_exp(x):
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        xc = np.where(x < -45.0, -45.0, x)
        k = np.rint(xc * LOG2E)
        r = (xc - k * LN2_HI) - k * LN2_LO
        p = np.full_like(xc, EXP_C[13])
        for n in range(12, -1, -1):
            p = p * r + EXP_C[n]
        return np.where(x < -45.0, 0.0, np.ldexp(p, k.astype(np.int32)))


def spec_log(s):
    s = np.asarray(s, np.float64)
    f, e = np.frexp(s)
    low = f < SQRT_HALF
    f, e = np.where(low, f * 2.0, f), np.where(low, e - 1, e).astype(np.float64)
    z = (f - 1.0) / (f + 1.0)
    z2 = z * z
    q = np.full_like(z, LOG_D[10])
    for n in range(9, -1, -1):
        q = q * z2 + LOG_D[n]
    return e * LN2_HI + ((2.0 * z) * q + e * LN2_LO)


def tree_sums(u):
    """The losses' reduction, two stages, each in the header's order: u float64 [B, 8], the samples' contributions -> (partials [W, 8],
    sums [8])."""
    B = len(u)
    W = (B + 63) // 64
    v = np.zeros((W * 64, u.shape[1]))
    v[:B] = u                                                        # the last wave is filled up with 0.0
    v = v.reshape(W, 64, -1)
    for h in (32, 16, 8, 4, 2, 1):
        v = v[:, :h] + v[:, h:]
    partials = v[:, 0]
    rounds = (W + 63) // 64
    p = np.zeros((rounds * 64, u.shape[1]))
    p[:W] = partials                                                 # a lane without a row in a round adds nothing: t + 0.0 is t (t is never -0.0)
    t = np.zeros((64, u.shape[1]))
    for k in range(rounds):
        t = t + p[64 * k:64 * k + 64]
    for h in (32, 16, 8, 4, 2, 1):
        t = t[:h] + t[h:]
    return partials, t[0]


def butterfly(u):
    """u float64 [.., 64]: u_j = u_j + u_{j ^ off} for off = 32 .. 1; every place holds the sum afterwards."""
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        u = u + u[..., lane ^ off]
    return u


def _same(got, want, what):
    """Byte for byte, but a NaN of the rule is any NaN."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaNs")
    word = np.uint32 if got.dtype == np.float32 else np.uint64
    g, w = np.where(nan, 0, got).astype(got.dtype), np.where(nan, 0, want).astype(got.dtype)
    diff = np.nonzero((g.view(word).reshape(len(g), -1) != w.view(word).reshape(len(w), -1)).any(axis=1))[0]
    assert diff.size == 0, (what, "first row that differs", int(diff[0]), g[diff[0]], w[diff[0]])
