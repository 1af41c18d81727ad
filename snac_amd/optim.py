"""DeviceAdam: the optimiser step of a DeviceMLP on the device (include/snac_hip.h, "Optimiser step of the device network";
snac_amd/csrc/k_adam.hip, adam_rule.h).

Through torch the end of a training step is clip_grad_norm_ and Adam.step(): ten to twenty small launches whose sums come in whatever
order the foreach kernels pick, and for a target network a copy or a lerp per parameter on top.  DeviceAdam does all of it in two
launches from the flat gradient that DeviceMLP.backward writes: the global norm as float64 sums in a stated order, the clip, Adam per
parameter in float64 rounded once, and the target's slow copy, written into the parameters where they lie.  The same gradients give
the same weights on every run.

    mlp = DeviceMLP(net, env); tgt = DeviceMLP(target_net, env)
    opt = DeviceAdam(mlp, lr=1e-3, max_norm=0.5, target=tgt, tau=0.005)
    y = mlp.forward(x).requires_grad_()                              # no autograd node for the network
    loss_of(y).backward()                                            # leaves y.grad: the loss's gradient to the outputs
    opt.backward_step(x, y.grad)                                     # backward (three launches) and the step (two)

It does not read .grad: with train_forward() and autograd the optimiser stays torch's.
"""
import torch

from . import _lib
from ._lib import ptr as _ptr
from ._rule import OnDevice
from .mlp import DeviceMLP

_bump = getattr(torch.autograd.graph, "increment_version", None)


class DeviceAdam(OnDevice):
    def __init__(self, mlp, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=None, target=None, tau=1.0):
        """mlp: the DeviceMLP whose parameters are stepped in place.  lr: finite and >= 0, a plain attribute that may be changed between
        steps.  betas: two numbers in [0, 1).  eps: finite and >= 0.  max_norm: None or 0 (no clip) or the largest global norm of the
        gradient (torch's clip_grad_norm_).  target: a DeviceMLP of the same dims on other tensors, or None.  tau: in (0, 1].  With
        tau < 1 the target follows every step inside the step's own launch, tgt += tau * (theta' - tgt) (SAC's and DDPG's slow copy); with
        tau == 1 (the default) a step leaves it alone and sync_target() copies the network when the caller asks, every K steps (DQN's hard
        copy: one made at every step would be no target).  The attribute sync_every_step holds that choice and may be set either way.
        The moments, the step's scratch and the flat gradient buffer of backward_step() are allocated on first use: nothing here touches
        the device."""
        if not isinstance(mlp, DeviceMLP):
            raise ValueError("mlp must be a DeviceMLP")
        if target is not None:
            if not isinstance(target, DeviceMLP):
                raise ValueError("target must be a DeviceMLP or None")
            if target.dims != mlp.dims:
                raise ValueError("the target's dims %s are not the network's %s" % (list(target.dims), list(mlp.dims)))
            if target.device != mlp.device:
                raise ValueError("the target must be on %s" % (mlp.device,))
            mine = {id(p) for wb in mlp._params for p in wb}
            if target is mlp or any(id(p) in mine for wb in target._params for p in wb):
                raise ValueError("the target shares a parameter with the network")
        for what, value in (("lr", lr), ("eps", eps)):
            if not _number(value) or not 0.0 <= float(value) < float("inf"):
                raise ValueError("%s must be a finite number >= 0" % what)
        try:
            beta1, beta2 = betas
        except (TypeError, ValueError):
            raise ValueError("betas must be two numbers in [0, 1)") from None
        if not all(_number(b) and 0.0 <= float(b) < 1.0 for b in (beta1, beta2)):
            raise ValueError("betas must be two numbers in [0, 1)")
        if max_norm is not None and (not _number(max_norm) or not 0.0 <= float(max_norm) < float("inf")):
            raise ValueError("max_norm must be None or a finite number >= 0 (0: no clip)")
        if not _number(tau) or not 0.0 < float(tau) <= 1.0:
            raise ValueError("tau must be in (0, 1]")
        self.mlp, self.target = mlp, target
        self.env, self.device = mlp.env, mlp.device
        self.lr, self.betas, self.eps = float(lr), (float(beta1), float(beta2)), float(eps)
        self.max_norm = 0.0 if max_norm is None else float(max_norm)
        self.tau = float(tau)
        self.sync_every_step = target is not None and self.tau < 1.0
        self.t = 0
        self._lib = mlp._lib
        self._m = self._v = self._flat = self._partials = self._norm = self._bad = None

    def _state(self):
        if self._m is None:
            P = self.mlp.num_params
            self._m = torch.zeros((P,), dtype=torch.float32, device=self.device)
            self._v = torch.zeros((P,), dtype=torch.float32, device=self.device)
            self._partials = torch.empty(((P + 63) // 64,), dtype=torch.float64, device=self.device)
            self._norm = torch.zeros((2,), dtype=torch.float64, device=self.device)
            self._bad = torch.zeros((1,), dtype=torch.int32, device=self.device)

    @property
    def grad_norm(self):
        """float64 [2] on the device: the last step's {norm, coef}: the global norm of the gradient and what it was scaled by (1.0:
        not clipped; 0.0: a bad step)."""
        self._state()
        return self._norm

    @property
    def bad_steps(self):
        """int32 [1] on the device: the steps refused so far because the gradient held a NaN or an infinity; they wrote nothing."""
        self._state()
        return self._bad

    def _written(self, nets):
        """The parameters of `nets` were written outside autograd: their versions move on, so that a graph which saved them before
        (train_forward) is refused at .backward(), as after a torch optimiser's step."""
        if _bump is None:
            raise _lib.SnacError("torch.autograd.graph.increment_version is missing: this torch cannot be told of an in-place write")
        _bump([p for net in nets for wb in net._params for p in wb])

    def step(self, flat):
        """One snac_mlp_adam_step from flat, the float32 [num_params] gradient in DeviceMLP.backward's layout (read only): t advances,
        bias1 = 1 - beta1^t and bias2 = 1 - beta2^t are computed here in float64, and the network's parameters, the moments and (with
        sync_every_step) the target are written in place.  A step whose gradient holds a NaN or an infinity writes none of them and
        counts in bad_steps; it still advances t.  Two launches on the current stream; nothing waits."""
        P = self.mlp.num_params
        lr = self.lr
        if not _number(lr) or not 0.0 <= float(lr) < float("inf"):
            raise ValueError("lr must be a finite number >= 0")
        if self.sync_every_step and self.target is None:
            raise ValueError("sync_every_step needs a target: give target= to the constructor")
        if not torch.is_tensor(flat) or flat.dtype != torch.float32 or not flat.is_contiguous() or tuple(flat.shape) != (P,):
            raise ValueError("flat must be a contiguous torch.float32 tensor of shape (%d,) on %s" % (P, self.device))
        if flat.device != self.device:
            raise ValueError("flat must be on %s" % (self.device,))
        self._state()
        self.t += 1
        beta1, beta2 = self.betas
        bias1, bias2 = 1.0 - beta1 ** self.t, 1.0 - beta2 ** self.t
        tgt = self.target if self.sync_every_step else None
        self._launch(self._lib.snac_mlp_adam_step, self.mlp._descriptor(), _ptr(flat), _ptr(self._m), _ptr(self._v), float(lr), beta1, beta2,
                     self.eps, bias1, bias2, self.max_norm, None if tgt is None else tgt._descriptor(), self.tau, _ptr(self._norm),
                     _ptr(self._partials), _ptr(self._bad))
        self._written((self.mlp,) if tgt is None else (self.mlp, tgt))

    def backward_step(self, x, grad_y):
        """mlp.backward(x, grad_y) into this object's own flat buffer, then step(): a whole update from the loss's gradient to the outputs
        of mlp.forward(x), with no autograd node for the network.  -> the flat gradient (overwritten by the next call)."""
        if self._flat is None:
            self._flat = torch.empty((self.mlp.num_params,), dtype=torch.float32, device=self.device)
        flat, _ = self.mlp.backward(x, grad_y, out=self._flat)
        self.step(flat)
        return flat

    def sync_target(self, tau=None):
        """snac_mlp_lerp: the target moves towards the network as it is now, tgt += tau * (theta - tgt); tau=None: the constructor's;
        tau = 1 copies the bits (DQN's hard copy every K ticks).  One launch; nothing waits."""
        if self.target is None:
            raise ValueError("sync_target needs a target: give target= to the constructor")
        tau = self.tau if tau is None else tau
        if not _number(tau) or not 0.0 < float(tau) <= 1.0:
            raise ValueError("tau must be in (0, 1]")
        self._launch(self._lib.snac_mlp_lerp, self.target._descriptor(), self.mlp._descriptor(), float(tau))
        self._written((self.target,))

    def state_dict(self):
        """{"t": the steps taken, "m", "v": copies of the moments, float32 [num_params]}."""
        self._state()
        return {"t": self.t, "m": self._m.clone(), "v": self._v.clone()}

    def load_state_dict(self, state):
        """The counterpart of state_dict(): t, and the moments copied into this object's own."""
        P = self.mlp.num_params
        try:
            t, m, v = state["t"], state["m"], state["v"]
        except (TypeError, KeyError):
            raise ValueError("the state must hold t, m and v") from None
        if isinstance(t, bool) or not isinstance(t, int) or t < 0:
            raise ValueError("t must be an integer >= 0")
        for what, a in (("m", m), ("v", v)):
            if not torch.is_tensor(a) or a.dtype != torch.float32 or tuple(a.shape) != (P,):
                raise ValueError("%s must be a torch.float32 tensor of shape (%d,)" % (what, P))
        self._state()
        self._m.copy_(m)
        self._v.copy_(v)
        self.t = t


def _number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool) and x == x
