"""Residual flow with Lipschitz constraints — drop-in for src/flows/advanced/residual_flow.py.

  SpectralNorm    residual_flow.py:17-81    one power iteration per call; W_eff = W * (c / sigma)
                                            where sigma > c, else W
  ResidualBlock   residual_flow.py:84-150   Linear(dim, H) -> act -> Linear(H, H) -> act -> Linear(H, dim),
                                            every layer under SpectralNorm(c = lipschitz_constant / 2)
  ResidualFlow    residual_flow.py:153-340

The flow is x = z + f(z) with f(z) = (z + mlp(z)) - z (the reference's `residual_block(z) - z`). Its
inverse is the fixed-point iteration z <- x - f(z) from z = x, and its log-det the truncated Neumann
series sum_{k=1..n} (-1)^(k+1) tr(J^k) / k of J = df/dz.

What the composite restates, and how:
  * J is the Jacobian of the EFFECTIVE (normalised) weights, in closed form: row i is
    W3[i, :] D2 W2 D1 W1 with the activation derivatives in torch autograd's forms. The reference
    builds the same matrix from `dim` autograd passes, which needs grad mode; this form runs under
    torch.no_grad() and in float64.
  * Parameter gradients are straight-through, as the reference's `weight.data = ...` makes them: the
    gradient with respect to the effective weight lands on the parameter, with no sigma term.
  * Train mode: `u` and `v` advance on every SpectralNorm call, and the calls come in the reference's
    order — one per layer for f, then one per layer for each of the `dim` Jacobian rows (each row
    from the weights of its own call), and one per layer for each fixed-point iteration.

TWO DELIBERATE DIFFERENCES from the reference:
  * The fixed-point iteration stops per sample. A sample stops when its own ||z_new - z||_2 < tol
    and keeps z, the iterate before that step, exactly as the reference does at its `break`; one that
    reaches max_iter keeps its last z_new; the loop runs while any sample is still running. The
    reference tests `torch.all(diff < tol)` over the batch, which makes a row's result depend on the
    rows it shares a batch with (by up to about 1e-6 at the default tol). The loop still ends at the
    iteration at which the reference's ends, so the number of SpectralNorm calls is the same.
  * Train mode always runs the composite (`_torch_only`): its semantics mutate buffers inside one
    call. The gfx950 kernel (csrc/nfx_residual*.hip, one launch per call) is for eval mode, dim <= 8
    and hidden_dim <= 128; other shapes raise NotImplementedError on the GPU (or run the composite
    with ALLOW_TORCH_FALLBACK).

Gradients in eval mode recompute through the composite by default. With
`ResidualFlow.fused_backward = True` (on the class or an instance) they come from the fused backward
kernels (csrc/nfx_residual_bwd*.hip) for dim <= 8 and hidden_dim <= 64, in HIP only: the unchanged
forward kernel, then one main kernel, a fixed-order float64 reduction and a finish. hidden_dim 65..128
and train mode keep the composite route. A THIRD DELIBERATE DIFFERENCE, on that route only: the
inverse's gradient is the implicit-function gradient at the returned z (one dim x dim solve of
(I + J)^T per sample), not the gradient of the unrolled iteration the composite differentiates; the
two differ by the iteration's residual (README). A row with a non-finite value adds nothing to the
parameter gradients and gets a zero input gradient, where autograd gives NaN. Double backward is not
supported there.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .flow import HipFlow


class _StraightThrough(torch.autograd.Function):
    """The value of `w_eff`, the gradient to `w`."""

    @staticmethod
    def forward(ctx, w, w_eff):
        return w_eff.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


class SpectralNorm(nn.Module):
    """Spectral normalisation of `module.weight` by power iteration (residual_flow.py:17-81)."""

    def __init__(self, module, lipschitz_constant=0.9, n_power_iterations=1):
        super().__init__()
        self.module = module
        self.lipschitz_constant = lipschitz_constant
        self.n_power_iterations = n_power_iterations
        if not hasattr(module, "weight"):
            raise ValueError("Module must have a 'weight' attribute")
        weight = module.weight
        self.register_buffer("u", torch.randn(weight.size(0)))
        self.register_buffer("v", torch.randn(weight.size(1)))
        self.u.data = F.normalize(self.u.data, dim=0)
        self.v.data = F.normalize(self.v.data, dim=0)

    def effective_weight(self, dtype=None):
        """One call's worth of the reference's forward up to the weight: the power iteration from
        the stored (u, v), sigma, the effective weight (gradient straight through to the parameter),
        and in train mode the buffer update."""
        weight = self.module.weight
        w = weight if dtype is None or dtype == weight.dtype else weight.to(dtype)
        with torch.no_grad():
            wd = w.detach()
            u, v = self.u.to(wd.dtype), self.v.to(wd.dtype)
            for _ in range(self.n_power_iterations):
                v = F.normalize(torch.mv(wd.t(), u), dim=0)
                u = F.normalize(torch.mv(wd, v), dim=0)
            sigma = torch.dot(u, torch.mv(wd, v))
            engaged = bool(sigma > self.lipschitz_constant)
            if engaged:
                normalized = wd * (self.lipschitz_constant / sigma)
            if self.training:
                self.u.data = u.to(self.u.dtype)
                self.v.data = v.to(self.v.dtype)
        return _StraightThrough.apply(w, normalized) if engaged else w

    def forward(self, *args, **kwargs):
        x = args[0]
        return F.linear(x, self.effective_weight(x.dtype), self._bias(x.dtype))

    def _bias(self, dtype):
        b = self.module.bias
        return None if b is None else b.to(dtype)


_ACTIVATIONS = {"relu": _lib.NFX_RESIDUAL_RELU, "elu": _lib.NFX_RESIDUAL_ELU,
                "leaky_relu": _lib.NFX_RESIDUAL_LEAKY_RELU, "tanh": _lib.NFX_RESIDUAL_TANH}


class ResidualBlock(nn.Module):
    """g(x) = x + mlp(x), every Linear under SpectralNorm (residual_flow.py:84-150)."""

    def __init__(self, dim, hidden_dim, lipschitz_constant=0.9, activation="relu"):
        super().__init__()
        self.dim = dim
        self.hidden_dim = hidden_dim
        self.lipschitz_constant = lipschitz_constant
        if activation == "relu":
            self.activation = nn.ReLU()
        elif activation == "elu":
            self.activation = nn.ELU()
        elif activation == "leaky_relu":
            self.activation = nn.LeakyReLU(0.1)
        elif activation == "tanh":
            self.activation = nn.Tanh()
        else:
            raise ValueError(f"Unsupported activation: {activation}")
        self.layer1 = SpectralNorm(nn.Linear(dim, hidden_dim), lipschitz_constant=lipschitz_constant / 2)
        self.layer2 = SpectralNorm(nn.Linear(hidden_dim, hidden_dim), lipschitz_constant=lipschitz_constant / 2)
        self.layer3 = SpectralNorm(nn.Linear(hidden_dim, dim), lipschitz_constant=lipschitz_constant / 2)
        self._initialize_weights()

    def _initialize_weights(self):
        for module in [self.layer1.module, self.layer2.module, self.layer3.module]:
            nn.init.xavier_normal_(module.weight, gain=0.1)
            if module.bias is not None:
                nn.init.zeros_(module.bias)

    def layers(self):
        return [self.layer1, self.layer2, self.layer3]

    def activation_code(self):
        """NFX_RESIDUAL_* of the activation module, or -1 for one the kernels do not have."""
        a = self.activation
        if type(a) is nn.ReLU:
            return _ACTIVATIONS["relu"]
        if type(a) is nn.ELU and a.alpha == 1.0:
            return _ACTIVATIONS["elu"]
        if type(a) is nn.LeakyReLU and a.negative_slope == 0.1:
            return _ACTIVATIONS["leaky_relu"]
        if type(a) is nn.Tanh:
            return _ACTIVATIONS["tanh"]
        return -1

    def derivative(self, pre, out):
        """The activation's derivative in torch autograd's form, from its input and its output."""
        a = self.activation
        if type(a) is nn.ReLU:
            return (out > 0).to(out.dtype)
        if type(a) is nn.LeakyReLU:
            return torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, a.negative_slope))
        if type(a) is nn.ELU and a.alpha == 1.0:
            return torch.where(pre > 0, torch.ones_like(pre), out + 1)
        if type(a) is nn.Tanh:
            return 1 - out * out
        raise NotImplementedError(f"no closed-form derivative for {type(a).__name__}")

    def weights(self, dtype):
        """One SpectralNorm call per layer, in layer order: [(W_eff, b)] * 3 in `dtype`."""
        return [(l.effective_weight(dtype), l._bias(dtype)) for l in self.layers()]

    def mlp(self, x, weights):
        """(out, g1, g2): the MLP on the given effective weights and its two derivative masks."""
        (w1, b1), (w2, b2), (w3, b3) = weights
        a1 = F.linear(x, w1, b1)
        h1 = self.activation(a1)
        a2 = F.linear(h1, w2, b2)
        h2 = self.activation(a2)
        return F.linear(h2, w3, b3), self.derivative(a1, h1), self.derivative(a2, h2)

    def forward(self, x):
        residual = x
        out = self.layer1(x)
        out = self.activation(out)
        out = self.layer2(out)
        out = self.activation(out)
        out = self.layer3(out)
        return residual + out


class ResidualFlow(HipFlow):
    """Residual flow (residual_flow.py:153-340); see the module docstring for the deliberate
    differences from the reference."""

    # True: eval-mode gradients come from the fused backward kernels (csrc/nfx_residual_bwd*.hip) for
    # dim <= 8 and hidden_dim <= 64; False (the default) recomputes through the composite on the GPU.
    fused_backward = False

    def __init__(self, dim, hidden_dim=64, lipschitz_constant=0.9, activation="relu", max_iter=100, tol=1e-6,
                 neumann_terms=3):
        super().__init__()
        self.data_dim = dim
        self.dim = dim
        self.hidden_dim = hidden_dim
        self.lipschitz_constant = lipschitz_constant
        self.max_iter = max_iter
        self.tol = tol
        self.neumann_terms = neumann_terms
        self.residual_block = ResidualBlock(dim=dim, hidden_dim=hidden_dim, lipschitz_constant=lipschitz_constant,
                                            activation=activation)

    # -- the composite ----------------------------------------------------------------------------
    def _residual_function(self, x):
        """f(x) = residual_block(x) - x = (x + mlp(x)) - x."""
        return self.residual_block(x) - x

    def _compute_jacobian(self, z):
        """[B, dim, dim], J[:, i, k] = d f_i / d z_k, of the effective weights. In train mode row i
        comes from the weights of its own SpectralNorm calls, as in the reference."""
        block = self.residual_block
        if not self.training:
            w = block.weights(z.dtype)
            _, g1, g2 = block.mlp(z, w)
            (w1, _), (w2, _), (w3, _) = w
            t1 = g1.unsqueeze(1) * w1.t().unsqueeze(0)     # [B, dim, H]: d h1 / d z_k
            t2 = g2.unsqueeze(1) * (t1 @ w2.t())           # [B, dim, H]: d h2 / d z_k
            return (t2 @ w3.t()).transpose(1, 2)           # [B, i, k]
        rows = []
        for i in range(self.dim):
            w = block.weights(z.dtype)
            _, g1, g2 = block.mlp(z, w)
            (w1, _), (w2, _), (w3, _) = w
            rows.append((((w3[i] * g2) @ w2) * g1) @ w1)   # [B, dim]
        return torch.stack(rows, dim=1)

    def _compute_log_det_neumann(self, z):
        jacobian = self._compute_jacobian(z)
        log_det = torch.zeros(z.shape[0], device=z.device, dtype=z.dtype)
        jac_power = jacobian
        for k in range(1, self.neumann_terms + 1):
            trace_term = torch.diagonal(jac_power, dim1=-2, dim2=-1).sum(dim=-1)
            log_det = log_det + ((-1) ** (k + 1)) * trace_term / k
            if k < self.neumann_terms:
                jac_power = torch.bmm(jac_power, jacobian)
        return log_det

    def _torch_call(self, x, direction):
        if direction > 0:
            f_z = self._residual_function(x)
            return x + f_z, self._compute_log_det_neumann(x)
        z = x.clone()
        running = torch.ones(x.shape[0], dtype=torch.bool, device=x.device)
        for _ in range(self.max_iter):
            z_new = x - self._residual_function(z)
            diff = torch.norm(z_new - z, dim=1)
            running = running & ~(diff < self.tol)
            if not bool(running.any()):
                break
            z = torch.where(running.unsqueeze(1), z_new, z)
        return z, -self._compute_log_det_neumann(z)

    # -- gfx950 path -------------------------------------------------------------------------------
    def _torch_only(self):
        return self.training

    def _hip_supported(self, x):
        if x.dim() != 2 or x.shape[1] != self.dim:
            return False, f"input shape {tuple(x.shape)} vs dim={self.dim}"
        block = self.residual_block
        H = block.layer1.module.out_features
        if any(l.n_power_iterations != 1 or l.module.bias is None for l in block.layers()):
            return False, "the kernels pack one power iteration and biased layers"
        if self.neumann_terms < 0 or self.max_iter < 0:
            return False, "neumann_terms and max_iter must not be negative"
        if not _lib.lib().nfx_residual_supported(max(x.shape[0], 1), self.dim, H, block.activation_code()):
            return False, (f"dim={self.dim} hidden_dim={H} activation={type(block.activation).__name__} outside the "
                           f"kernel family (dim <= 8, hidden_dim <= 128, relu / elu / leaky_relu(0.1) / tanh)")
        return True, ""

    def _state_key(self, device):
        return super()._state_key(device) + tuple(l.lipschitz_constant for l in self.residual_block.layers())

    def _build_pack(self, device):
        L = _lib.checked()
        d, H = self.dim, self.residual_block.layer1.module.out_features
        packed = torch.empty(L.nfx_residual_packed_floats(d, H), device=device, dtype=torch.float32)
        L.nfx_residual_pack(*self._raw_layers(device), d, H, packed, _lib.stream_of(packed))
        return packed

    def _hip_launch(self, x, out, log_det, direction, accumulate):
        packed = self._packed(x.device, self._build_pack)
        block = self.residual_block
        _lib.checked().nfx_residual_flow(
            packed, x, out, log_det, x.shape[0], self.dim, block.layer1.module.out_features, block.activation_code(),
            _lib.NFX_FORWARD if direction > 0 else _lib.NFX_INVERSE, int(self.neumann_terms), int(self.max_iter),
            float(self.tol), int(bool(accumulate)), _lib.stream_of(x))

    # -- fused backward (opt-in: ResidualFlow.fused_backward = True) -------------------------------
    def _dispatch(self, x, direction):
        if (self.fused_backward and torch.is_grad_enabled() and self._route(x) == "hip"
                and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
                and self._hip_backward_ok(x, direction)):
            return _ResidualFunction.apply(self, direction, x, *list(self.parameters()))
        return super()._dispatch(x, direction)

    def _hip_backward_ok(self, x, direction):
        """The fused backward is switched on and has kernels for this shape (dim <= 8, hidden_dim
        <= 64); otherwise the gradients recompute through the composite."""
        block = self.residual_block
        return bool(self.fused_backward and x.dim() == 2 and x.shape[1] == self.dim and x.shape[0] >= 1
                    and _lib.lib().nfx_residual_backward_supported(
                        x.shape[0], self.dim, block.layer1.module.out_features, block.activation_code()))

    def _raw_layers(self, device):
        """nfx_residual_pack's leading arguments: (weight, bias, u, v, c) per layer."""
        args = []
        for l in self.residual_block.layers():
            args += [_lib.dense(t.detach().to(device=device, dtype=torch.float32))
                     for t in (l.module.weight, l.module.bias, l.u, l.v)]
            args.append(float(l.lipschitz_constant))
        return args

    def _build_backward_pack(self, device):
        L = _lib.checked()
        d, H = self.dim, self.residual_block.layer1.module.out_features
        packed = torch.empty(L.nfx_residual_backward_packed_floats(d, H), device=device, dtype=torch.float32)
        L.nfx_residual_pack_backward(*self._raw_layers(device), d, H, packed, _lib.stream_of(packed))
        return packed

    def _hip_backward(self, z, gy, gld, direction):
        """(gx, [gW1, gb1, gW2, gb2, gW3, gb3]) in HIP only. `z` is the point the layer's function is
        differentiated at: the call's input (forward) or its output (inverse)."""
        L = _lib.checked()
        z = _lib.dense(z)
        block = self.residual_block
        B, d, H = z.shape[0], self.dim, block.layer1.module.out_features
        packed = self._packed(z.device, self._build_backward_pack, slot="_nfx_bwd_pack_cache")
        gy = _lib.dense(gy.to(torch.float32))
        gld = _lib.dense(gld.to(torch.float32))
        gx = torch.empty_like(z)
        grads = [torch.empty(p.shape, device=z.device, dtype=torch.float32)
                 for l in block.layers() for p in (l.module.weight, l.module.bias)]
        ws = torch.empty(L.nfx_residual_backward_workspace_floats(B, d, H), device=z.device, dtype=torch.float32)
        L.nfx_residual_backward(packed, z, gy, gld, gx, *grads, ws, B, d, H, block.activation_code(),
                                _lib.NFX_FORWARD if direction > 0 else _lib.NFX_INVERSE, int(self.neumann_terms),
                                _lib.stream_of(z))
        return gx, grads


class _ResidualFunction(torch.autograd.Function):
    """Eval-mode ResidualFlow with the fused backward: the unchanged forward kernel, then the backward
    kernels. It keeps the point of differentiation: the input (forward) or the output z (inverse).
    No composite anywhere; double backward is not supported."""

    @staticmethod
    def forward(ctx, layer, direction, x, *params):
        x = _lib.dense(x)
        with torch.no_grad():
            y, ld = layer._hip_call(x.detach(), direction)
        ctx.layer, ctx.direction = layer, direction
        ctx.save_for_backward(x if direction > 0 else y)
        return y, ld

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy, gld):
        from . import flow as _flow
        (z,) = ctx.saved_tensors
        layer = ctx.layer
        _flow.STATS["hip"] += 1
        gx, gparams = layer._hip_backward(z.detach(), gy, gld, ctx.direction)
        gparams = [g if p.requires_grad else None for p, g in zip(layer.parameters(), gparams)]
        return (None, None, gx, *gparams)
