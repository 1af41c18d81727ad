"""Device-side helpers of the GPU tests: arrays placed on the device and their pointers, started envs, the comparisons with the oracle that
several kernels' tests share, the last kernel's name, the example loader.  torch and snac_amd are imported inside the functions, so this
module imports on a machine without a GPU and before the library is built.  The helpers keep the names the test files call them by."""
import ctypes as C
import importlib.util
import os

import numpy as np

import helpers
from specmath import _same


# ---- pointers and placement ------------------------------------------------------------------------------------------------------------------
def _vp(t):
    """A tensor (or None) as the void pointer the C ABI takes."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _place(arr, offset, dev):
    """(flat tensor, view of arr's shape in it): arr on the device, one element into a larger tensor when offset."""
    import torch

    flat = torch.zeros((arr.size + 9,), dtype=torch.from_numpy(arr).dtype, device=dev)
    at = 1 if offset else 0
    view = flat[at:at + arr.size].view(arr.shape)
    view.copy_(torch.from_numpy(arr))
    assert view.data_ptr() % 16 == (arr.itemsize if offset else 0) and view.is_contiguous()
    return flat, view


def _place_floats(arr, offset, dev):
    """(flat tensor, view of arr's shape in it): arr on the device, one float into a larger tensor when offset."""
    import torch

    flat = torch.full((arr.size + 9,), 7.0, dtype=torch.float32, device=dev)
    at = 1 if offset else 0
    view = flat[at:at + arr.size].view(arr.shape)
    view.copy_(torch.from_numpy(arr))
    assert view.data_ptr() % 16 == (4 if offset else 0) and view.is_contiguous()
    return flat, view


def _raw(t):
    return t.cpu().numpy().tobytes()


# ---- the generated inputs of the loss kernels ------------------------------------------------------------------------------------------------
def _shifts(B, sorts):
    return range(len(sorts)) if B <= 2 else (B % len(sorts),)        # one or two samples take every sort in turn


def _equal(got, want, what, outputs):
    for k in outputs + ("partials",):
        g = got[k]
        if g is None:
            continue
        if k == "bad_rows":
            assert int(g[0]) == want[k], (what, k, int(g[0]), want[k])
        else:
            _same(g, np.ascontiguousarray(want[k]), (what, k))


# ---- envs ------------------------------------------------------------------------------------------------------------------------------------
def _tag(kind, dyn):
    return ("sin_train" if kind == 1 else "dense_train") if dyn else ("p0" if kind == 1 else "p1")


def _env(kind, dyn, n, seed, **kw):
    from snac_amd import BatchedDMPEnv

    table = helpers.plan_table(kind, dyn, _tag(kind, dyn))
    full = table.reshape((-1, 30) if kind == 1 else (-1, 26, 26))
    env = BatchedDMPEnv(kind, dyn, n, plans=full, seed=seed, **kw)
    env.reset()
    return env


def short_env(kind, n, f32, seed=3, **kw):
    """(a reset dataset env of 16 plans and a time limit of 12, its plans' cells float32 [16, cells])."""
    import torch
    from snac_amd import BatchedDMPEnv

    table = helpers.plan_table(kind, True, "sin_train" if kind == 1 else "dense_train")[:16]
    full = table.reshape(len(table), 30) if kind == 1 else table.reshape(len(table), 26, 26)
    env = BatchedDMPEnv(kind, True, n, plans=full, seed=seed, total_step=12, obs_dtype=torch.float32 if f32 else torch.float64, **kw)
    env.reset()
    cells = (full if kind == 1 else full[:, 3:23, 3:23].reshape(len(full), -1)).astype(np.float32)
    return env, cells


def _ids(v):
    return "%dd_%s" % (v[0], "dyn" if v[1] else "sta") if isinstance(v, tuple) else str(v)


# ---- a batch against its oracle --------------------------------------------------------------------------------------------------------------
def _compare(env, orc, T, t0, f32=False, actions=None, step_size=None):
    import torch

    a = None if actions is None else torch.from_numpy(actions).to(env.device)
    k = None if step_size is None else torch.from_numpy(step_size).to(env.device)
    og, rg, dg = env.rollout(T, actions=a, step_size=k)
    oc, rc, dc = orc.rollout(T, t0=t0, actions=actions, step_size=step_size, nthreads=16)
    want = oc.astype(np.float32) if f32 else oc
    assert og.cpu().numpy().tobytes() == want.tobytes(), "observations"
    assert rg.cpu().numpy().tobytes() == rc.tobytes(), "rewards"
    assert np.array_equal(dg.cpu().numpy().view(np.uint8), dc), "done flags"


def _end_state(env, orc):
    s, e = orc.stats(), env.episodic_stats()
    assert (e["episodes"], e["return_sum"], e["iou_fx_sum"]) == (int(s["episodes"].sum()), int(s["ret"].sum()), int(s["iou_fx"].sum()))
    assert env.iou().cpu().numpy().tobytes() == orc.iou().tobytes()
    st = orc.state()
    assert np.array_equal(env.environment_memory().cpu().numpy().reshape(env.num_envs, -1), st["grid"])


# ---- the search's trees ----------------------------------------------------------------------------------------------------------------------
def _subtree(ch, x, out):
    """Canonical traversal: preorder, children in action order."""
    out.append(x)
    for c in ch[x]:
        if c >= 0:
            _subtree(ch, int(c), out)
    return out


# ---- the library and the examples ------------------------------------------------------------------------------------------------------------
def _kernel():
    from snac_amd import _lib

    return _lib.lib().snac_last_kernel().decode()


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(helpers.ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
