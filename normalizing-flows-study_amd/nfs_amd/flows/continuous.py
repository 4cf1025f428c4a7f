"""Continuous normalizing flow — drop-in for src/flows/continuous/.

  ODEFunc          ode_func.py:4-91      Linear(dim+1, H) -> Tanh -> Linear(H, H) -> Tanh -> Linear(H, dim)
                                         on [z, t] (time is the LAST input column)
  ContinuousFlow   continuous_flow.py:6-138

The flow integrates the augmented state [z, l], dz/dt = v(z, t), dl/dt = +tr(dv/dz) (the
reference's sign, ode_func.py:72-76), from t = 0 to 1 (forward) or 1 to 0 (inverse) with the
reference's solver settings: torchdiffeq's fixed-grid `rk4` — the 3/8 rule, not the classic
tableau — at `step_size` 0.01:

    k1 = f(t0, y)
    k2 = f(t0 + dt/3,  y + dt*k1/3)
    k3 = f(t0 + 2dt/3, y + dt*(k2 - k1/3))
    k4 = f(t1,         y + dt*(k1 - k2 + k3))
    y1 = y + (k1 + 3*(k2 + k3) + k4) * dt * 0.125

on the grid g_k = k*step_size + a, k < n = ceil((b - a)/step_size + 1), g_{n-1} := b (computed in
the dtype of the times tensor, float32 by default; the last step may be short). A decreasing
interval integrates the negated-time problem: the same grid walked downward with negative dt.
Equal times return the input and zeros. After the last step the reference's guards apply
(continuous_flow.py:65-74): a NaN/Inf output element returns its input element, a NaN/Inf log-det
becomes 0, both are clamped to [-10, 10]. (Its try/except fall-backs to Euler and to the identity
are not reproduced: a fixed-step solver does not raise.)

On a ROCm device the whole integration of a call is ONE gfx950 kernel (csrc/nfx_cnf*.hip) for
dim <= 8 and hidden_dim in {32, 64, 128}; other shapes raise NotImplementedError there (or run the
composite with ALLOW_TORCH_FALLBACK). Gradients recompute through the torch composite on the GPU by
default; with `ContinuousFlow.fused_backward = True` (on the class or an instance) they come from
the fused reverse sweep of the discrete scheme (csrc/nfx_cnf_bwd*.hip: a trajectory-saving forward,
the sweep, a fixed-order reduction) for dim <= 8 and hidden_dim in {32, 64}, in HIP only;
hidden_dim = 128 keeps the composite route. Double backward is not supported there.
"""
import torch
import torch.nn as nn

from .. import _lib
from .flow import HipFlow


class ODEFunc(nn.Module):
    """Time-conditioned velocity field and its divergence (ode_func.py:4-91).

    The divergence is the exact closed-form trace for every `dim`: one forward-mode tangent per
    input dimension,

        tr = sum_i W3[i, :] . ((1 - h2^2) * (W2 . ((1 - h1^2) * W1[:, i])))

    with h1 = tanh(W1 [z; t] + b1), h2 = tanh(W2 h1 + b2). ONE DELIBERATE DIFFERENCE from the
    reference: for dim > 2 it switches to a Hutchinson estimate with fresh randn noise per
    evaluation (ode_func.py:64-70), which is unreproducible by construction; the exact trace is
    the quantity that estimate targets. For dim <= 2 the two agree."""

    def __init__(self, dim, hidden_dim):
        super().__init__()
        self.dim = dim
        self.net = nn.Sequential(
            nn.Linear(dim + 1, hidden_dim),
            nn.Tanh(),
            nn.Linear(hidden_dim, hidden_dim),
            nn.Tanh(),
            nn.Linear(hidden_dim, dim),
        )
        self._initialize_weights()

    def _initialize_weights(self):
        """ode_func.py:79-91: Xavier-normal weights, zero biases, zero final layer (a fresh flow is
        the identity with zero log-det). Same order as the reference, so seeded inits match."""
        for layer in self.net:
            if isinstance(layer, nn.Linear):
                nn.init.xavier_normal_(layer.weight, gain=1.0)
                if layer.bias is not None:
                    nn.init.zeros_(layer.bias)
        final = self.net[-1]
        nn.init.zeros_(final.weight)
        if final.bias is not None:
            nn.init.zeros_(final.bias)

    def linears(self):
        return [self.net[0], self.net[2], self.net[4]]

    def velocity_and_trace(self, t, z):
        """(v(z, t) [B, dim], tr(dv/dz) [B]) in z's dtype; t is a 0-d tensor or a float."""
        l1, l2, l3 = self.linears()
        d = self.dim
        w1, w2, w3 = (l.weight.to(z.dtype) for l in (l1, l2, l3))
        b1, b2, b3 = (l.bias.to(z.dtype) for l in (l1, l2, l3))
        t_col = torch.as_tensor(t, dtype=z.dtype, device=z.device).expand(z.shape[0]).unsqueeze(1)
        h1 = torch.tanh(torch.cat([z, t_col], dim=1) @ w1.t() + b1)
        h2 = torch.tanh(h1 @ w2.t() + b2)
        v = h2 @ w3.t() + b3
        t1 = (1 - h1 * h1).unsqueeze(1) * w1[:, :d].t().unsqueeze(0)   # [B, d, H]: d h1 / d z_i
        u = (1 - h2 * h2).unsqueeze(1) * (t1 @ w2.t())                  # [B, d, H]: d h2 / d z_i
        tr = (u * w3.unsqueeze(0)).sum(dim=(1, 2))
        return v, tr

    def forward(self, t, augmented_state):
        """d/dt of [z, log_det] (ode_func.py:30-77)."""
        v, tr = self.velocity_and_trace(t, augmented_state[:, :self.dim])
        return torch.cat([v, tr.unsqueeze(1)], dim=1)


class ContinuousFlow(HipFlow):
    """Continuous normalizing flow (continuous_flow.py:6-138) with the exact divergence for every
    `dim` (see ODEFunc for that one deliberate difference from the reference)."""

    step_size = 0.01  # options={'step_size': 0.01}; a class attribute, the signature stays the reference's
    # True: gradients come from the fused backward kernels (csrc/nfx_cnf_bwd*.hip) for dim <= 8 and
    # hidden_dim in {32, 64}; False (the default) recomputes through the composite on the GPU.
    fused_backward = False

    def __init__(self, dim, hidden_dim=64):
        super().__init__()
        self.data_dim = dim
        self.dim = dim
        self.ode_func = ODEFunc(dim, hidden_dim)

    @property
    def hidden_dim(self):
        return self.ode_func.net[0].out_features

    def forward(self, z, integration_times=None):
        """Sampling direction: t from 0 to 1 (or integration_times = [a, b])."""
        return self._dispatch(z, 1 if integration_times is None else self._times(integration_times))

    def inverse(self, x, integration_times=None):
        """Density direction: t from 1 to 0 (or integration_times = [a, b])."""
        return self._dispatch(x, -1 if integration_times is None else self._times(integration_times))

    # `direction` is +1, -1 or a times tensor [a, b]; it travels unchanged through HipFlow's routing
    # and the autograd recompute.
    @staticmethod
    def _times(direction):
        if isinstance(direction, int):
            return torch.tensor([0.0, 1.0] if direction > 0 else [1.0, 0.0])
        t = torch.as_tensor(direction).detach().cpu()
        if not t.is_floating_point():
            t = t.float()
        if t.numel() != 2:
            raise ValueError("integration_times must hold two times [t_begin, t_end]")
        return t.reshape(2)

    def time_grid(self, times):
        """(t_k [n], in the dtype of `times`): the solver's grid from times[0] to times[1]."""
        a, b = times[0], times[1]
        sgn = 1.0 if bool(a <= b) else -1.0
        s0, s1 = a * sgn, b * sgn
        step = torch.tensor(self.step_size, dtype=times.dtype)
        n = int(torch.ceil((s1 - s0) / step + 1))
        grid = torch.arange(n, dtype=times.dtype) * step + s0
        grid[-1] = s1
        return grid * sgn

    def _torch_call(self, x, direction):
        """The scheme, literally, in x's dtype (CPU tensors, float64, the autograd recompute)."""
        times = self._times(direction)
        if bool(times[0] == times[1]):
            return x, torch.zeros(x.shape[0], device=x.device, dtype=x.dtype)
        grid = self.time_grid(times).to(device=x.device, dtype=x.dtype).unbind(0)
        f = self.ode_func.velocity_and_trace
        y, ld = x, torch.zeros(x.shape[0], device=x.device, dtype=x.dtype)
        for t0, t1 in zip(grid[:-1], grid[1:]):
            dt = t1 - t0
            k1, l1 = f(t0, y)
            k2, l2 = f(t0 + dt / 3, y + dt * k1 / 3)
            k3, l3 = f(t0 + 2 * dt / 3, y + dt * (k2 - k1 / 3))
            k4, l4 = f(t1, y + dt * (k1 - k2 + k3))
            y = y + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
            ld = ld + (l1 + 3 * (l2 + l3) + l4) * dt * 0.125
        y = torch.where(torch.isnan(y) | torch.isinf(y), x, y)
        ld = torch.where(torch.isnan(ld) | torch.isinf(ld), torch.zeros_like(ld), ld)
        return torch.clamp(y, min=-10.0, max=10.0), torch.clamp(ld, min=-10.0, max=10.0)

    # -- gfx950 path -------------------------------------------------------------------------------
    def _hip_supported(self, x):
        if x.dim() != 2 or x.shape[1] != self.dim:
            return False, f"input shape {tuple(x.shape)} vs dim={self.dim}"
        if not _lib.lib().nfx_cnf_supported(max(x.shape[0], 1), self.dim, self.hidden_dim):  # (B = 0: a no-op)
            return False, (f"dim={self.dim} hidden_dim={self.hidden_dim} outside the kernel family "
                           f"(dim <= 8, hidden_dim in {{32, 64, 128}})")
        return True, ""

    def _build_pack(self, device):
        L = _lib.checked()
        d, H = self.dim, self.hidden_dim
        packed = torch.empty(L.nfx_cnf_packed_floats(d, H), device=device, dtype=torch.float32)
        t = [_lib.dense(p.detach().to(device=device, dtype=torch.float32))
             for lin in self.ode_func.linears() for p in (lin.weight, lin.bias)]
        L.nfx_cnf_pack(*t, d, H, packed, _lib.stream_of(packed))
        return packed

    def _hip_launch(self, x, out, log_det, direction, accumulate):
        packed = self._packed(x.device, self._build_pack)
        times = self._times(direction).float()
        _lib.checked().nfx_cnf_integrate(
            packed, x, out, log_det, x.shape[0], self.dim, self.hidden_dim, float(times[0]), float(times[1]),
            float(torch.tensor(self.step_size)), int(bool(accumulate)), _lib.stream_of(x))

    # -- fused backward (opt-in: ContinuousFlow.fused_backward = True) -----------------------------
    def _dispatch(self, x, direction):
        if (self.fused_backward and torch.is_grad_enabled() and self._route(x) == "hip"
                and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
                and self._hip_backward_ok(x, direction)):
            return _CnfFunction.apply(self, direction, x, *list(self.parameters()))
        return super()._dispatch(x, direction)

    def _hip_backward_ok(self, x, direction):
        """The fused backward is switched on and has kernels for this shape (dim <= 8, hidden_dim in
        {32, 64}); otherwise the gradients recompute through the composite."""
        return bool(self.fused_backward and x.dim() == 2 and x.shape[1] == self.dim and x.shape[0] >= 1
                    and _lib.lib().nfx_cnf_backward_supported(x.shape[0], self.dim, self.hidden_dim))

    def _build_backward_pack(self, device):
        L = _lib.checked()
        d, H = self.dim, self.hidden_dim
        packed = torch.empty(L.nfx_cnf_backward_packed_floats(d, H), device=device, dtype=torch.float32)
        L.nfx_cnf_pack_backward(*self._raw_weights(device), d, H, packed, _lib.stream_of(packed))
        return packed

    def _raw_weights(self, device):
        return [_lib.dense(p.detach().to(device=device, dtype=torch.float32))
                for lin in self.ode_func.linears() for p in (lin.weight, lin.bias)]

    def _time_args(self, direction):
        times = self._times(direction).float()
        return float(times[0]), float(times[1]), float(torch.tensor(self.step_size))

    def _hip_forward_save(self, x, direction):
        """(y, ld, traj): the forward kernel's outputs, bit for bit, and the trajectory the backward
        replays (the state at the start of every step, and the unclamped final state)."""
        L = _lib.checked()
        x = _lib.dense(x)
        B, d, H = x.shape[0], self.dim, self.hidden_dim
        t0, t1, step = self._time_args(direction)
        packed = self._packed(x.device, self._build_backward_pack, slot="_nfx_bwd_pack_cache")
        out = torch.empty_like(x)
        ld = torch.empty(B, device=x.device, dtype=torch.float32)
        traj = torch.empty(L.nfx_cnf_trajectory_floats(B, d, t0, t1, step), device=x.device, dtype=torch.float32)
        L.nfx_cnf_integrate_save(packed, x, out, ld, traj, B, d, H, t0, t1, step, 0, _lib.stream_of(x))
        return out, ld, traj

    def _hip_backward(self, x, gy, gld, direction, traj=None):
        """(gx, [gW1, gb1, gW2, gb2, gW3, gb3]) in HIP only; `traj` is the saving forward's
        trajectory (recomputed here when the caller kept none)."""
        L = _lib.checked()
        x = _lib.dense(x)
        B, d, H = x.shape[0], self.dim, self.hidden_dim
        if traj is None:
            traj = self._hip_forward_save(x, direction)[2]
        t0, t1, step = self._time_args(direction)
        packed = self._packed(x.device, self._build_backward_pack, slot="_nfx_bwd_pack_cache")
        w1, _, w2, _, w3, _ = raw = self._raw_weights(x.device)
        gy = _lib.dense(gy.to(torch.float32))
        gld = _lib.dense(gld.to(torch.float32))
        gx = torch.empty_like(x)
        grads = [torch.empty_like(t) for t in raw]
        ws = torch.empty(L.nfx_cnf_backward_workspace_floats(B, d, H), device=x.device, dtype=torch.float32)
        L.nfx_cnf_backward(packed, w1, w2, w3, x, traj, gy, gld, gx, *grads, ws, B, d, H, t0, t1, step,
                           _lib.stream_of(x))
        return gx, grads


class _CnfFunction(torch.autograd.Function):
    """ContinuousFlow with the fused backward: the trajectory-saving forward kernel, then the reverse
    sweep in HIP. No composite anywhere; double backward is not supported."""

    @staticmethod
    def forward(ctx, layer, direction, x, *params):
        from . import flow as _flow
        _flow.STATS["hip"] += 1
        x = _lib.dense(x)  # (saved in this form: a strided or offset input is copied once, not per pass)
        with torch.no_grad():
            y, ld, traj = layer._hip_forward_save(x.detach(), direction)
        ctx.layer, ctx.direction = layer, direction
        ctx.save_for_backward(x, traj)
        return y, ld

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy, gld):
        from . import flow as _flow
        x, traj = ctx.saved_tensors
        layer = ctx.layer
        _flow.STATS["hip"] += 1
        gx, gparams = layer._hip_backward(x.detach(), gy, gld, ctx.direction, traj)
        gparams = [g if p.requires_grad else None for p, g in zip(layer.parameters(), gparams)]
        return (None, None, gx, *gparams)
