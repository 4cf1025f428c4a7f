"""Neural autoregressive flow — drop-in for src/flows/advanced/neural_autoregressive_flow.py.

  DeepMADE                  neural_autoregressive_flow.py:17-205   the conditioner: masked Linear ->
                                                                   [LayerNorm] -> act -> [Dropout] per hidden
                                                                   layer, a ResidualBlock where two widths
                                                                   are equal, outputs clamped to [-2, 2]
  ResidualBlock             neural_autoregressive_flow.py:208-239  act(LN(linear(x))) + x
  NeuralAutoregressiveFlow  neural_autoregressive_flow.py:242-391

(`ResidualBlock` here is the NAF one; `nfs_amd.ResidualBlock` is the residual flow's.)

inverse is one conditioner call: z = (x - mu) exp(clamp(-clamp(alpha))), ld = sum of the log-scales.
forward starts from x = 0 and makes `dim` conditioner calls; call i uses mu_i and alpha_i alone.
Both turn NaN / Inf elements of the result and of the log-det into 0 and clamp the log-det to +-100.

A QUIRK OF THE REFERENCE, MIRRORED AND NOT FIXED: LayerNorm mixes all the hidden units of a layer, so
with use_layer_norm=True (the default) the conditioner is not autoregressive: mu_i and alpha_i depend
on every x_j, and forward is NOT the inverse of inverse (round-trip error about 2e+1 at dim 3,
[32, 32]; about 2e-6 with use_layer_norm=False). The same happens at dim == 2 with a residual block,
whose skip joins the first layer's [0, 0, 1, 1] degree pattern to the next layer's linspace pattern.
The result the reference defines is what `dim` FULL conditioner passes give, so the gfx950 kernel
(csrc/nfx_naf*.hip, one launch per call and direction) runs every pass through the whole network and
never uses the masks to skip work across passes.

Routing: CPU or fp64 tensors run the composite (`_torch_call`, the reference's operations in the
reference's order, any dtype). Train mode with dropout > 0 runs the composite; LayerNorm has no
train / eval difference, so train mode with dropout == 0 runs the kernel. Gradients recompute
through the composite by default; with `NeuralAutoregressiveFlow.fused_backward = True` (on the
class or an instance) the gradients of `inverse`, the direction an NLL step uses, come from the
fused reverse sweep (csrc/nfx_naf_bwd*.hip: the conditioner recomputed from x, the sweep, a
fixed-order reduction) for hidden widths up to 64, in HIP only; wider layers and `forward` keep the
composite route. Double backward is not supported there. A row with a non-finite input element or
conditioner output adds nothing to any parameter gradient there and gets a zero input gradient,
where autograd on the composite gives NaN (0 * NaN behind torch.where). The kernel family is 1 <= dim <= 16, 1 to 4 hidden layers of width 1..128
whose packed image fits the LDS of one workgroup (nfx_naf_supported decides), relu / elu /
leaky_relu(0.1) / gelu; the constructor's default [512, 512, 512] is outside it and raises
NotImplementedError on the GPU (or runs the composite with ALLOW_TORCH_FALLBACK).

With `NeuralAutoregressiveFlow.wide_kernel = True` (on the class or an instance; off by default, so
that a shape that raised keeps raising) a shape outside that family runs the wide kernel
(csrc/nfx_naf_wide*.hip) when it lies in the wide family: the same dims, layer counts and activations
with widths up to 512, activations in LDS and the weights streamed from global memory, one launch per
call and direction. A shape inside the narrow family takes the narrow kernel whatever the switch
says, with the same bits. The wide family has no fused backward: its gradients recompute through the
composite, and train mode with dropout > 0 runs the composite, as everywhere.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .autoregressive import MaskedLinear
from .flow import HipFlow

_FAMILY = ("the kernel family (1 <= dim <= 16, 1 to 4 hidden layers of width 1..128 with the packed image inside "
           "160 KiB of LDS, relu / elu / leaky_relu(0.1) / gelu, the network the constructor builds)")
_WIDE_FAMILY = ("the wide kernel family (wide_kernel = True: 1 <= dim <= 16, 1 to 4 hidden layers of width 1..512, "
                "the same activations)")


def activation_code(a):
    """NFX_NAF_* of an activation module, or -1 for one the kernels do not have."""
    if type(a) is nn.ReLU:
        return _lib.NFX_NAF_RELU
    if type(a) is nn.ELU and a.alpha == 1.0:
        return _lib.NFX_NAF_ELU
    if type(a) is nn.LeakyReLU and a.negative_slope == 0.1:
        return _lib.NFX_NAF_LEAKY_RELU
    if type(a) is nn.GELU and getattr(a, "approximate", "none") == "none":
        return _lib.NFX_NAF_GELU
    return -1


_ACTIVATION_MODULES = {"relu": nn.ReLU, "elu": nn.ELU, "leaky_relu": lambda: nn.LeakyReLU(0.1), "gelu": nn.GELU}


def hidden_degrees(d, width, first):
    """Degrees of a hidden layer's units: floor(linspace(0, d - 1, width)); zeros at d == 1; and for
    the FIRST hidden layer at d == 2 the pattern [0, 0, 1, 1] repeated, as the reference assigns them."""
    if d == 1:
        return np.zeros(width, dtype=int)
    if first and d == 2:
        return np.array([0, 0, 1, 1] * (width // 4 + 1))[:width]
    return np.floor(np.linspace(0, d - 1, width)).astype(int)


class ResidualBlock(nn.Module):
    """act(LN(linear(x))) + x (neural_autoregressive_flow.py:208-239)."""

    def __init__(self, linear_layer, activation, use_layer_norm=True, dropout=0.0):
        super().__init__()
        self.linear = linear_layer
        self.activation = activation
        self.use_layer_norm = use_layer_norm
        self.dropout = dropout
        if use_layer_norm:
            self.layer_norm = nn.LayerNorm(linear_layer.out_features)
        if dropout > 0:
            self.dropout_layer = nn.Dropout(dropout)

    def forward(self, x):
        h = self.linear(x)
        if self.use_layer_norm:
            h = self.layer_norm(h)
        h = self.activation(h)
        if self.dropout > 0:
            h = self.dropout_layer(h)
        return h + x


class DeepMADE(nn.Module):
    """Deep masked MLP with LayerNorm and residual blocks (neural_autoregressive_flow.py:17-205)."""

    def __init__(self, input_dim, hidden_dims, output_dim_multiplier=2, activation="relu", use_layer_norm=True,
                 use_residual=True, dropout=0.0):
        super().__init__()
        self.input_dim = input_dim
        self.hidden_dims = hidden_dims
        self.output_dim_multiplier = output_dim_multiplier
        self.use_layer_norm = use_layer_norm
        self.use_residual = use_residual
        self.dropout = dropout
        if activation not in _ACTIVATION_MODULES:
            raise ValueError(f"Unsupported activation: {activation}")
        self.activation = _ACTIVATION_MODULES[activation]()  # one instance, shared by every position

        d = self.input_dim
        self.m = {-1: np.arange(d)}
        for i, width in enumerate(hidden_dims):
            self.m[i] = hidden_degrees(d, width, first=i == 0)
        self.masks = self._create_masks()
        self.network = self._build_network()

    def _create_masks(self):
        masks = []
        n = len(self.hidden_dims)
        if n == 0:
            return masks
        for i in range(n):  # layer i sees a unit below it of no larger degree
            m = (self.m[i - 1][:, np.newaxis] <= self.m[i][np.newaxis, :]).T
            masks.append(torch.from_numpy(m.astype(np.float32)))
        # mu_i and alpha_i see hidden units of degree <= i - 1: output 0 is bias only
        d = self.input_dim
        m_final = np.zeros((d * self.output_dim_multiplier, self.hidden_dims[-1]), dtype=np.float32)
        for i in range(d):
            m_final[i, :] = (self.m[n - 1] <= i - 1).astype(np.float32)
        for i in range(d):
            m_final[d + i, :] = (self.m[n - 1] <= i - 1).astype(np.float32)
        masks.append(torch.from_numpy(m_final))
        return masks

    def _build_network(self):
        dims = self.hidden_dims
        out_dim = self.input_dim * self.output_dim_multiplier
        if len(dims) == 0:
            return nn.Sequential(MaskedLinear(self.input_dim, out_dim, mask=None))
        layers = [MaskedLinear(self.input_dim, dims[0], mask=self.masks[0])]
        if self.use_layer_norm:
            layers.append(nn.LayerNorm(dims[0]))
        layers.append(self.activation)
        if self.dropout > 0:
            layers.append(nn.Dropout(self.dropout))
        for i in range(1, len(dims)):
            layer = MaskedLinear(dims[i - 1], dims[i], mask=self.masks[i])
            if self.use_residual and dims[i - 1] == dims[i]:
                layers.append(ResidualBlock(layer, self.activation, self.use_layer_norm, self.dropout))
            else:
                layers.append(layer)
                if self.use_layer_norm:
                    layers.append(nn.LayerNorm(dims[i]))
                layers.append(self.activation)
                if self.dropout > 0:
                    layers.append(nn.Dropout(self.dropout))
        layers.append(MaskedLinear(dims[-1], out_dim, mask=self.masks[-1]))
        self._initialize_weights(layers)
        return nn.Sequential(*layers)

    def _initialize_weights(self, layers):
        """Xavier-normal weights in network order (the order the RNG is consumed in): gain 0.5 on a
        plain Linear, 0.1 on a residual block's; zero biases."""
        for layer in layers:
            if isinstance(layer, ResidualBlock):
                linear, gain = layer.linear, 0.1
            elif isinstance(layer, nn.Linear):
                linear, gain = layer, 0.5
            else:
                continue
            nn.init.xavier_normal_(linear.weight, gain=gain)
            if linear.bias is not None:
                nn.init.zeros_(linear.bias)

    def forward(self, x):
        return torch.clamp(self.network(x), min=-2.0, max=2.0)

    def plan(self):
        """[(linear, layer_norm or None, activation, residual)] per hidden layer, then the output
        MaskedLinear: the network as the constructor builds it (Dropout modules skipped), or None
        for any other module tree."""
        mods = list(self.network)
        hidden, i = [], 0
        while i < len(mods) - 1:
            m = mods[i]
            if type(m) is ResidualBlock:
                if type(m.linear) is not MaskedLinear or not hidden:
                    return None
                ln = getattr(m, "layer_norm", None) if m.use_layer_norm else None
                if m.use_layer_norm and type(ln) is not nn.LayerNorm:
                    return None
                if m.dropout > 0 and type(getattr(m, "dropout_layer", None)) is not nn.Dropout:
                    return None
                hidden.append((m.linear, ln, m.activation, True))
                i += 1
                continue
            if type(m) is not MaskedLinear:
                return None
            i += 1
            ln = None
            if i < len(mods) - 1 and type(mods[i]) is nn.LayerNorm:
                ln = mods[i]
                i += 1
            if i >= len(mods) - 1 or isinstance(mods[i], (MaskedLinear, ResidualBlock, nn.LayerNorm, nn.Dropout)):
                return None  # no activation after the layer
            act = mods[i]
            i += 1
            if i < len(mods) - 1 and type(mods[i]) is nn.Dropout:
                i += 1
            hidden.append((m, ln, act, False))
        if not hidden or type(mods[-1]) is not MaskedLinear:
            return None
        return hidden, mods[-1]


class NeuralAutoregressiveFlow(HipFlow):
    """Neural autoregressive flow (neural_autoregressive_flow.py:242-391); see the module docstring
    for the reference's quirk that this class mirrors."""

    # True: the gradients of `inverse` come from the fused backward kernels (csrc/nfx_naf_bwd*.hip) for
    # 1 to 4 hidden layers of width 1..64; False (the default) recomputes through the composite on the GPU.
    fused_backward = False
    # True: a shape outside the narrow kernel family (nfx_naf_supported) runs the wide kernel
    # (csrc/nfx_naf_wide*.hip; widths up to 512, the default constructor's among them) instead of
    # raising NotImplementedError. Shapes inside the narrow family are not affected.
    wide_kernel = False

    def __init__(self, dim, hidden_dims=[512, 512, 512], activation="relu", use_layer_norm=True, use_residual=True,
                 dropout=0.1, clamp_alpha=3.0, clamp_log_scale=5.0):
        super().__init__()
        self.data_dim = dim
        self.dim = dim
        self.clamp_alpha = clamp_alpha
        self.clamp_log_scale = clamp_log_scale
        self.conditioner = DeepMADE(input_dim=dim, hidden_dims=hidden_dims, output_dim_multiplier=2,
                                    activation=activation, use_layer_norm=use_layer_norm, use_residual=use_residual,
                                    dropout=dropout)

    # -- the composite ----------------------------------------------------------------------------
    @staticmethod
    def _guards(y, log_det):
        y = torch.where(torch.isnan(y) | torch.isinf(y), torch.zeros_like(y), y)
        log_det = torch.where(torch.isnan(log_det) | torch.isinf(log_det), torch.zeros_like(log_det), log_det)
        return y, torch.clamp(log_det, min=-100, max=100)

    def _torch_call(self, x, direction):
        if direction < 0:
            mu, alpha = self.conditioner(x).chunk(2, dim=1)
            alpha = torch.clamp(alpha, min=-self.clamp_alpha, max=self.clamp_alpha)
            log_scale = torch.clamp(-alpha, min=-self.clamp_log_scale, max=self.clamp_log_scale)
            z = (x - mu) * torch.exp(log_scale)
            return self._guards(z, torch.sum(log_scale, dim=1))
        z = x
        x = torch.zeros(z.size(0), self.dim, device=z.device, dtype=z.dtype)
        log_det = torch.zeros(z.size(0), device=z.device, dtype=z.dtype)
        for i in range(self.dim):
            mu, alpha = self.conditioner(x).chunk(2, dim=1)
            alpha = torch.clamp(alpha, min=-self.clamp_alpha, max=self.clamp_alpha)
            log_scale_i = torch.clamp(alpha[:, i], min=-self.clamp_log_scale, max=self.clamp_log_scale)
            # (the reference writes x[:, i] in place; a fresh tensor per pass keeps autograd's saved
            # conditioner inputs intact, with the same values)
            x = x.clone()
            x[:, i] = z[:, i] * torch.exp(log_scale_i) + mu[:, i]
            log_det = log_det + log_scale_i
        return self._guards(x, log_det)

    # -- gfx950 path -------------------------------------------------------------------------------
    def _torch_only(self):
        return self.training and self.conditioner.dropout > 0

    def _plan(self):
        """(hidden, output, widths, activation code, flags) of the kernel call, cached until a module
        of the tree is replaced; None for a tree the constructor does not build. The cache travels
        with copy.deepcopy and pickle, so it holds plain Python values only, no ctypes object and no
        address: `_widths_arg` builds the host array for each call."""
        bind = self._nfx_binding()
        cached = self.__dict__.get("_nfx_naf_plan")
        if cached is not None and cached[0] is bind:
            return cached[1]
        plan = self.conditioner.plan() if isinstance(self.conditioner, DeepMADE) else None
        if plan is not None:
            hidden, out = plan
            d = self.dim
            codes = {activation_code(a) for _, _, a, _ in hidden}
            lns = {ln is not None for _, ln, _, _ in hidden}
            ok = len(codes) == 1 and len(lns) == 1 and out.weight.shape[0] == 2 * d
            prev = d
            for lin, ln, _, res in hidden:
                ok = ok and lin.weight.shape[1] == prev and lin.bias is not None and lin.mask is not None
                ok = ok and (not res or lin.weight.shape[0] == prev)
                if ln is not None:
                    ok = ok and tuple(ln.normalized_shape) == (lin.weight.shape[0],) and ln.weight is not None \
                        and ln.bias is not None
                prev = lin.weight.shape[0]
            ok = ok and out.weight.shape[1] == prev and out.bias is not None and out.mask is not None
            if ok:
                widths = tuple(int(lin.weight.shape[0]) for lin, _, _, _ in hidden)
                flags = _lib.NFX_NAF_LAYER_NORM if lns == {True} else 0
                for l, (_, _, _, res) in enumerate(hidden):
                    if res:
                        flags |= _lib.NFX_NAF_RESIDUAL(l)
                plan = (hidden, out, widths, codes.pop(), flags)
            else:
                plan = None
        object.__setattr__(self, "_nfx_naf_plan", (bind, plan))
        return plan

    @staticmethod
    def _widths_arg(plan):
        """(array, address) for a `const int* widths` argument: a fresh host array of the plan's
        widths, which the caller keeps alive for the duration of the C call."""
        arr = (ctypes.c_int * len(plan[2]))(*plan[2])
        return arr, ctypes.addressof(arr)

    def _hip_supported(self, x):
        if x.dim() != 2 or x.shape[1] != self.dim:
            return False, f"input shape {tuple(x.shape)} vs dim={self.dim}"
        plan = self._plan()
        if plan is None:
            return False, f"the conditioner's module tree is not one the constructor builds: outside {_FAMILY}"
        hidden, _, widths, _, flags = plan
        # (the activation is read at every call: an attribute of the shared module may change in place)
        code = activation_code(hidden[0][2])
        keep, widths_ptr = self._widths_arg(plan)
        L = _lib.checked()
        B = max(x.shape[0], 1)
        if L.nfx_naf_supported(B, self.dim, len(hidden), widths_ptr, code, flags):
            return True, ""
        outside = _FAMILY
        if self.wide_kernel:
            if L.nfx_naf_wide_supported(B, self.dim, len(hidden), widths_ptr, code, flags):
                return True, ""
            outside = f"{_FAMILY} and outside {_WIDE_FAMILY}"
        return False, (f"dim={self.dim} hidden_dims={list(widths)} activation={type(hidden[0][2]).__name__} "
                       f"outside {outside}")

    def _wide(self):
        """The call runs the wide kernel: the switch is on and the narrow family does not hold the
        shape (asked at every call, like the activation: both may change in place)."""
        if not self.wide_kernel:
            return False
        plan = self._plan()
        keep, widths_ptr = self._widths_arg(plan)
        return not _lib.checked().nfx_naf_supported(1, self.dim, len(plan[0]), widths_ptr,
                                                    activation_code(plan[0][0][2]), plan[4])

    def _state_key(self, device):
        plan = self._plan()
        eps = () if plan is None else tuple(None if ln is None else ln.eps for _, ln, _, _ in plan[0])
        return super()._state_key(device) + eps

    def _build_pack(self, device, wide=False):
        L = _lib.checked()
        plan = self._plan()
        hidden = plan[0]
        widths, widths_ptr = self._widths_arg(plan)
        raw, keep = self._raw_layers(device)
        floats, pack = (L.nfx_naf_wide_packed_floats, L.nfx_naf_wide_pack) if wide else \
            (L.nfx_naf_packed_floats, L.nfx_naf_pack)
        packed = torch.empty(floats(self.dim, len(hidden), widths_ptr), device=device, dtype=torch.float32)
        pack(ctypes.addressof(raw), self.dim, len(hidden), widths_ptr, packed, _lib.stream_of(packed))
        return packed

    def _build_wide_pack(self, device):
        return self._build_pack(device, wide=True)

    def _hip_launch(self, x, out, log_det, direction, accumulate):
        # (one cache slot per family: toggling the switch never hands a kernel the other's image)
        wide = self._wide()
        packed = self._packed(x.device, self._build_wide_pack, slot="_nfx_wide_pack_cache") if wide else \
            self._packed(x.device, self._build_pack)
        plan = self._plan()
        hidden, flags = plan[0], plan[4]
        widths, widths_ptr = self._widths_arg(plan)
        L = _lib.checked()
        (L.nfx_naf_wide_flow if wide else L.nfx_naf_flow)(
            packed, x, out, log_det, x.shape[0], self.dim, len(hidden), widths_ptr, activation_code(hidden[0][2]), flags,
            float(self.clamp_alpha), float(self.clamp_log_scale),
            _lib.NFX_FORWARD if direction > 0 else _lib.NFX_INVERSE, int(bool(accumulate)), _lib.stream_of(x))

    # -- fused backward of the density direction (opt-in: NeuralAutoregressiveFlow.fused_backward = True) --
    def _dispatch(self, x, direction):
        if (self.fused_backward and direction < 0 and torch.is_grad_enabled() and self._route(x) == "hip"
                and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
                and self._hip_backward_ok(x)):
            return _NafFunction.apply(self, x, *list(self.parameters()))
        return super()._dispatch(x, direction)

    def _hip_backward_ok(self, x, direction=-1):
        """The fused backward is switched on and has kernels for this call (the density direction, 1 to
        4 hidden layers of width 1..64); otherwise the gradients recompute through the composite."""
        if not (self.fused_backward and direction < 0 and x.dim() == 2 and x.shape[1] == self.dim
                and x.shape[0] >= 1):
            return False
        plan = self._plan()
        if plan is None:
            return False
        keep, widths_ptr = self._widths_arg(plan)
        return bool(_lib.lib().nfx_naf_backward_supported(x.shape[0], self.dim, len(plan[0]), widths_ptr,
                                                          activation_code(plan[0][0][2]), plan[4]))

    def _raw_layers(self, device):
        """(NfxNafLayer array, the tensors it points to): the plan's layers as the C entry points read them."""
        hidden, out = self._plan()[:2]
        keep = []

        def p(t):
            t = _lib.dense(t.detach().to(device=device, dtype=torch.float32))
            keep.append(t)
            return t.data_ptr()

        raw = (_lib.NfxNafLayer * (len(hidden) + 1))()
        for r, (lin, ln, _, res) in zip(raw, list(hidden) + [(out, None, None, False)]):
            r.weight, r.bias, r.mask = p(lin.weight), p(lin.bias), p(lin.mask)
            if ln is not None:
                r.ln_weight, r.ln_bias, r.ln_eps = p(ln.weight), p(ln.bias), float(ln.eps)
            r.residual = int(res)
        return raw, keep

    def _build_backward_pack(self, device):
        L = _lib.checked()
        plan = self._plan()
        widths, widths_ptr = self._widths_arg(plan)
        raw, keep = self._raw_layers(device)
        packed = torch.empty(L.nfx_naf_backward_packed_floats(self.dim, len(plan[0]), widths_ptr), device=device,
                             dtype=torch.float32)
        L.nfx_naf_pack_backward(ctypes.addressof(raw), self.dim, len(plan[0]), widths_ptr, packed,
                                _lib.stream_of(packed))
        return packed

    def _hip_backward(self, x, gz, gld, direction=-1):
        """(gx, one gradient per entry of list(self.parameters())) of the density direction, in HIP only."""
        L = _lib.checked()
        x = _lib.dense(x)
        B, d = x.shape[0], self.dim
        plan = self._plan()
        hidden, out, _, _, flags = plan
        widths, widths_ptr = self._widths_arg(plan)
        packed = self._packed(x.device, self._build_backward_pack, slot="_nfx_bwd_pack_cache")
        raw, keep = self._raw_layers(x.device)
        gz = _lib.dense(gz.to(torch.float32))
        gld = _lib.dense(gld.to(torch.float32))
        gx = torch.empty_like(x)
        by_param = {}
        grads = (_lib.NfxNafLayerGrad * (len(hidden) + 1))()
        for g, (lin, ln, _, _) in zip(grads, list(hidden) + [(out, None, None, False)]):
            for name, p in (("weight", lin.weight), ("bias", lin.bias)) + (
                    () if ln is None else (("ln_weight", ln.weight), ("ln_bias", ln.bias))):
                t = torch.empty(p.shape, device=x.device, dtype=torch.float32)
                by_param[id(p)] = t
                setattr(g, name, t.data_ptr())
        ws = torch.empty(L.nfx_naf_backward_workspace_floats(B, d, len(hidden), widths_ptr), device=x.device,
                         dtype=torch.float32)
        L.nfx_naf_backward(packed, ctypes.addressof(raw), x, gz, gld, gx, ctypes.addressof(grads), ws, B, d,
                           len(hidden), widths_ptr, activation_code(hidden[0][2]), flags, float(self.clamp_alpha),
                           float(self.clamp_log_scale), _lib.stream_of(x))
        return gx, [by_param[id(p)] for p in self.parameters()]


class _NafFunction(torch.autograd.Function):
    """NeuralAutoregressiveFlow.inverse with the fused backward: the forward kernel as it stands (only
    the dense x is saved), then the reverse sweep in HIP. No composite anywhere; double backward is
    not supported."""

    @staticmethod
    def forward(ctx, layer, x, *params):
        x = _lib.dense(x)  # (saved in this form: a strided or offset input is copied once, not per pass)
        with torch.no_grad():
            y, ld = layer._hip_call(x.detach(), -1)  # (counts STATS["hip"])
        ctx.layer = layer
        ctx.save_for_backward(x)
        return y, ld

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gz, gld):
        from . import flow as _flow
        (x,) = ctx.saved_tensors
        layer = ctx.layer
        _flow.STATS["hip"] += 1
        gx, gparams = layer._hip_backward(x.detach(), gz, gld)
        gparams = [g if p.requires_grad else None for p, g in zip(layer.parameters(), gparams)]
        return (None, gx, *gparams)
