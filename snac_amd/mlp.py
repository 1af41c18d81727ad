"""DeviceMLP: the policy / value network of the PUCT search on the device (include/snac_hip.h, "Policy / value network on the device"
and "Backward pass of the device network"; snac_amd/csrc/k_mlp.hip, k_mlp_grad.hip).

The networks that guide the search here are tiny: an observation row of 7 / 51 / 502 values through one or two hidden layers of 64 to
256 units into A + 1 outputs.  Through torch such a network is five or six launches and a handful of casts and copies per search
iteration, and its sums come in whatever order the BLAS library picks.  DeviceMLP runs it as one launch whose every output is a float64
sum in index order: the same inputs give the same bytes on every run.  The parameters stay torch's and every launch reads them where
they lie, so an optimiser step enqueued on the stream is seen by the next launch and nothing is copied.  Training: train_forward(x) is
forward(x) as an autograd function whose backward is the device's own (backward(): the gradient of every weight and bias in one flat
buffer, float64 chains in a stated order, three launches), so the weight gradients are as reproducible as the outputs; the optimiser
stays torch's.  Going through the module with autograd, as before, still works: both read the same parameters.  DeviceAdam
(snac_amd/optim.py) takes the flat gradient of backward() through the clip and an Adam step on the device instead.

    net = torch.nn.Sequential(torch.nn.Linear(env.obs_dim, 64), torch.nn.ReLU(), torch.nn.Linear(64, A + 1)).to(env.device)
    mlp = DeviceMLP(net, env)                                        # or DeviceMLP([(w0, b0), (w1, b1)], 5, device="cuda:0")
    priors, value = mlp(obs)                                         # obs float32 / float64 [rows, obs_dim]; softmax priors, float64 value
    search = UCTSearch(env, 512, 0, 0.99, c=1.25, evaluator=mlp)    # the search then values its leaves in one fused launch
    y = mlp.forward(obs)                                             # the raw outputs, float32 [rows, A + 1]
    y = mlp.train_forward(obs); loss_of(y).backward()                # the same bytes; net's parameters get their .grad from the device
    flat, views = mlp.backward(obs, grad_y)                          # or directly: float32 [P] and [(gw, gb)] views per layer
"""
import ctypes as C

import torch

from . import _lib
from ._lib import ptr as _ptr
from ._rule import OnDevice, cuda_device

MAX_LAYERS, MAX_IN, MAX_HIDDEN, MAX_OUT = 4, 512, 256, 64            # the header's limits


def _layers_of(module):
    """[(weight, bias)] of a torch.nn.Sequential of Linear and ReLU, a ReLU after every Linear but the last; or the refusal in words."""
    mods = list(module)
    if not mods:
        raise ValueError("the Sequential is empty: it must hold Linear layers with a ReLU between them")
    layers = []
    for k, m in enumerate(mods):
        want_linear = k % 2 == 0
        if want_linear and not isinstance(m, torch.nn.Linear):
            raise ValueError("module %d is %s: a Linear belongs there (Linear, ReLU, Linear, ..., Linear)" % (k, type(m).__name__))
        if not want_linear and not isinstance(m, torch.nn.ReLU):
            raise ValueError("module %d is %s: a ReLU belongs after every Linear but the last" % (k, type(m).__name__))
        if want_linear:
            if m.bias is None:
                raise ValueError("module %d is a Linear without a bias" % k)
            layers.append((m.weight, m.bias))
    if len(mods) % 2 == 0:
        raise ValueError("the Sequential ends in a ReLU: the last module must be a Linear")
    return layers


class DeviceMLP(OnDevice):
    def __init__(self, module_or_layers, num_actions_or_env=None, device=None):
        """module_or_layers: a torch.nn.Sequential of Linear and ReLU (a ReLU after every Linear but the last), or a list of (weight
        [out, in], bias [out]) tensors, one pair per layer; one to four layers, an input of 1 .. 512, hidden widths of 1 .. 256, 1 .. 64
        outputs; the parameters contiguous float32 on the device.  num_actions_or_env: None (forward() only), 3, 5 or 8, or a
        BatchedDMPEnv, whose num_actions, device and stream are then taken; the last layer then has num_actions + 1 outputs.  device: a
        cuda device (not with an env); None: the parameters'.  References to the parameters are kept and their addresses are read at
        each call.  Nothing here touches the device."""
        if isinstance(module_or_layers, torch.nn.Sequential):
            layers = _layers_of(module_or_layers)
        elif isinstance(module_or_layers, torch.nn.Module):
            raise ValueError("the network must be a torch.nn.Sequential of Linear and ReLU (or a list of (weight, bias)), not a %s"
                             % type(module_or_layers).__name__)
        else:
            try:
                layers = [(w, b) for w, b in module_or_layers]
            except (TypeError, ValueError):
                raise ValueError("the network must be a torch.nn.Sequential of Linear and ReLU or a list of (weight, bias) tensors") from None
        if not 1 <= len(layers) <= MAX_LAYERS:
            raise ValueError("the network must have 1 .. %d Linear layers, not %d" % (MAX_LAYERS, len(layers)))
        na = num_actions_or_env
        if hasattr(na, "num_actions") and hasattr(na, "device"):
            if device is not None:
                raise ValueError("device is the env's when an env is given")
            self.env, device, na = na, na.device, na.num_actions
        if na is not None and (isinstance(na, bool) or not isinstance(na, int) or na not in (3, 5, 8)):
            raise ValueError("num_actions must be None, 3, 5 or 8 (or a BatchedDMPEnv)")
        self.num_actions = na
        for l, (w, b) in enumerate(layers):
            if not torch.is_tensor(w) or not torch.is_tensor(b) or w.dim() != 2 or b.dim() != 1 or b.shape[0] != w.shape[0]:
                raise ValueError("layer %d must be (weight [out, in], bias [out]) tensors" % l)
        if device is None:
            device = layers[0][0].device
        self.device = cuda_device(device, "the parameters and the observation rows live")
        dims = [int(layers[0][0].shape[1])]
        for l, (w, b) in enumerate(layers):
            for what, p in (("weight", w), ("bias", b)):
                if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.device:
                    raise ValueError("the %s of layer %d must be a contiguous torch.float32 tensor on %s" % (what, l, self.device))
            if int(w.shape[1]) != dims[-1]:
                raise ValueError("layer %d takes %d inputs where layer %d gives %d" % (l, int(w.shape[1]), l - 1, dims[-1]))
            dims.append(int(w.shape[0]))
        if not 1 <= dims[0] <= MAX_IN:
            raise ValueError("the input width must be 1 .. %d, not %d" % (MAX_IN, dims[0]))
        if any(not 1 <= d <= MAX_HIDDEN for d in dims[1:-1]):
            raise ValueError("hidden widths must be 1 .. %d, not %s" % (MAX_HIDDEN, dims[1:-1]))
        if not 1 <= dims[-1] <= MAX_OUT:
            raise ValueError("the output width must be 1 .. %d, not %d" % (MAX_OUT, dims[-1]))
        if na is not None and dims[-1] != na + 1:
            raise ValueError("the last layer must give num_actions + 1 = %d outputs (the logits and the value), not %d" % (na + 1, dims[-1]))
        self.dims = tuple(dims)
        self._params = layers                                        # references: the optimiser updates these tensors in place
        self._net = _lib.Mlp()
        self._net.layers = len(layers)
        for l, d in enumerate(dims):
            self._net.dim[l] = d
        self._lib = _lib.lib()
        self._bad = None                                             # made on first use
        self._work = None                                            # backward()'s workspace: made on first use, grown when asked for

    @property
    def bad_rows(self):
        """int32 [1] on the device: the rows whose head was refused so far (a NaN or +inf logit, every logit -inf, a value that is not
        finite); they got priors of zeros and value 0."""
        if self._bad is None:
            self._bad = torch.zeros((1,), dtype=torch.int32, device=self.device)
        return self._bad

    def _descriptor(self):
        """The network descriptor with the parameters' addresses as they are now (a pointer to it: what the entry points take)."""
        net = self._net
        for l, (w, b) in enumerate(self._params):
            net.w[l], net.b[l] = w.data_ptr(), b.data_ptr()
        return C.byref(net)

    def _rows(self, x, what, on_device=True):
        if not torch.is_tensor(x) or x.dtype not in (torch.float32, torch.float64) or not x.is_contiguous():
            raise ValueError("%s must be a contiguous torch.float32 or torch.float64 tensor of shape (rows, %d) on %s" % (what, self.dims[0], self.device))
        if x.dim() != 2 or x.shape[1] != self.dims[0] or x.shape[0] < 1:
            raise ValueError("%s must have shape (rows, %d), got %s" % (what, self.dims[0], tuple(x.shape)))
        if on_device and x.device != self.device:
            raise ValueError("%s must be on %s" % (what, self.device))
        return int(x.shape[0]), int(x.dtype == torch.float64)

    def forward(self, x, out=None):
        """float32 [rows, dims[-1]]: the outputs of the last layer for the rows of x (float32, or float64 rounded to float32 first).
        out: a contiguous float32 tensor of that shape on the device to write into.  One launch on the current stream (the env's, where
        an env was given); nothing waits."""
        rows, f64 = self._rows(x, "x")
        if out is None:
            out = torch.empty((rows, self.dims[-1]), dtype=torch.float32, device=self.device)
        elif (not torch.is_tensor(out) or out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (rows, self.dims[-1])
              or out.device != self.device):
            raise ValueError("out must be a contiguous torch.float32 tensor of shape (%d, %d) on %s" % (rows, self.dims[-1], self.device))
        self._launch(self._lib.snac_mlp_forward, self._descriptor(), _ptr(x), f64, rows, _ptr(out))
        return out

    def policy_value(self, obs, want_logits=False):
        """(priors float32 [rows, A], value float64 [rows]) of the observation rows obs [rows, obs_dim]: the softmax of the first A
        outputs and the last output; want_logits: also the raw outputs, float32 [rows, A + 1].  A row the head refuses gets zeros and
        counts in bad_rows.  One launch; nothing waits."""
        if self.num_actions is None:
            raise ValueError("policy_value belongs to a network with a head: give num_actions (or an env)")
        rows, f64 = self._rows(obs, "obs")
        A = self.num_actions
        priors = torch.empty((rows, A), dtype=torch.float32, device=self.device)
        value = torch.empty((rows,), dtype=torch.float64, device=self.device)
        logits = torch.empty((rows, A + 1), dtype=torch.float32, device=self.device) if want_logits else None
        self._launch(self._lib.snac_mlp_policy_value, self._descriptor(), A, _ptr(obs), f64, rows, _ptr(priors), _ptr(value), _ptr(logits),
                     _ptr(self.bad_rows))
        return (priors, value, logits) if want_logits else (priors, value)

    __call__ = policy_value                                          # a valid evaluator= of any UCTSearch

    @property
    def num_params(self):
        """P: the length of the flat gradient, every layer's weights and then its bias, in layer order."""
        return sum(self.dims[l + 1] * (self.dims[l] + 1) for l in range(len(self.dims) - 1))

    def _views(self, flat):
        """[(gw, gb)]: the layers' parts of a flat gradient, as views of the parameters' shapes."""
        views, at = [], 0
        for l in range(len(self.dims) - 1):
            K, N = self.dims[l], self.dims[l + 1]
            views.append((flat[at:at + N * K].view(N, K), flat[at + N * K:at + N * K + N]))
            at += N * (K + 1)
        return views

    def backward(self, x, grad_y, accumulate=False, out=None):
        """(flat, views): the gradient of a scalar loss to every weight and bias from grad_y float32 [rows, dims[-1]], its gradient to
        the outputs of forward(x) (include/snac_hip.h, "Backward pass of the device network": float64 chains in a stated order, the same
        bytes on every run).  flat: float32 [num_params]; views: [(gw, gb)] per layer, views into flat of the parameters' shapes.  out: a
        contiguous float32 tensor [num_params] on the device to write into or, with accumulate=True, to add to (in float64, rounded once).
        The activations are recomputed: nothing is kept from a forward call.  The workspace is a tensor kept on this object, grown when a
        call needs more, and used on the current stream only.  Three launches (two for a single layer); nothing waits."""
        rows, f64 = self._rows(x, "x", on_device=False)            # shapes and types first, the devices after them: all before a launch
        N, P = self.dims[-1], self.num_params
        if not torch.is_tensor(grad_y) or grad_y.dtype != torch.float32 or not grad_y.is_contiguous() or tuple(grad_y.shape) != (rows, N):
            raise ValueError("grad_y must be a contiguous torch.float32 tensor of shape (%d, %d) on %s" % (rows, N, self.device))
        if not isinstance(accumulate, bool):
            raise ValueError("accumulate must be True or False")
        if out is None and accumulate:
            raise ValueError("accumulate=True needs out: the flat gradient to add to")
        if out is not None and (not torch.is_tensor(out) or out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (P,)):
            raise ValueError("out must be a contiguous torch.float32 tensor of shape (%d,) on %s" % (P, self.device))
        for what, t in (("x", x), ("grad_y", grad_y), ("out", out)):
            if t is not None and t.device != self.device:
                raise ValueError("%s must be on %s" % (what, self.device))
        if out is None:
            out = torch.empty((P,), dtype=torch.float32, device=self.device)
        net = self._descriptor()
        need = int(self._lib.snac_mlp_backward_work_bytes(net, rows))
        if need < 0:
            _lib.check(-1)
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty((need,), dtype=torch.uint8, device=self.device)
        self._launch(self._lib.snac_mlp_backward, net, _ptr(x), f64, rows, _ptr(grad_y), _ptr(out), int(accumulate), _ptr(self._work), need)
        return out, self._views(out)

    def train_forward(self, x):
        """float32 [rows, dims[-1]]: the bytes of forward(x), as the output of a torch.autograd.Function of x and the parameters.  Its
        backward runs backward(x, grad_y) once and hands the views to autograd as the parameters' gradients (None for x), so accumulation
        into .grad, hooks and zero_grad() are autograd's and any torch.optim optimiser works as before.  y[:, :A] and y[:, A] go into
        PPOLoss / SearchLoss, y into TDLoss, or into any torch loss.  The backward pass recomputes the activations from the parameters, so
        they are saved with the graph: an in-place update of a parameter between train_forward() and .backward() raises autograd's
        version error, as it does for a torch module.  The function is differentiable once: its backward runs outside autograd, and a
        double backward through it raises."""
        self._rows(x, "x")
        return _TrainForward.apply(self, x, *[p for wb in self._params for p in wb])


class _TrainForward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mlp, x, *params):
        ctx.mlp = mlp
        ctx.save_for_backward(x, *params)                            # the parameters: for the check of their versions at backward
        return mlp.forward(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x = ctx.saved_tensors[0]                                     # raises if x or a parameter was written in place since forward
        _, views = ctx.mlp.backward(x, grad_y.contiguous())
        return (None, None) + tuple(g for gw_gb in views for g in gw_gb)
