"""Planar, Radial and Sylvester flows — drop-ins for src/flows/advanced/planar_flow.py,
radial_flow.py and sylvester_flow.py.

  PlanarFlow     z + u tanh(w.z + b), u = u_hat + (m - w.u_hat) w / (|w|^2 + 1e-8),
                 m = -1 + log1p(exp(w.u_hat));   log-det log(|1 + u.w psi| + 1e-8), psi = 1 - tanh^2
  RadialFlow     z + beta h (z - z0), h = 1 / (alpha + r + 1e-8), r = |z - z0|,
                 alpha = softplus(alpha_hat), beta = -alpha + softplus(beta_hat);
                 log-det (dim - 1) log(|1 + beta h| + 1e-8) + log(|1 + beta h + beta h' r| + 1e-8),
                 h' = -1 / ((alpha + r)^2 + 1e-8)
  SylvesterFlow  z + Q(tanh(Q(z) R^T + b) R), Q the Householder reflections in list order on row
                 vectors; log-det log(|det(I + R R^T diag(psi))| + 1e-8). That is the reference's
                 formula: it is the Jacobian's log-det only when Q is applied once as Q and once as
                 Q^T, which the reference does not do. Reproduced, not repaired.
A NaN / Inf log-det becomes 0; the values have no guard. Every inverse is the fixed-point iteration
z <- x - g(z) from z = x with the reference's hard-coded max_iter = 50 and tol = 1e-6, here instance
attributes (part of the pack-cache key).

ONE DELIBERATE DIFFERENCE from the reference, ResidualFlow's: the iteration stops per sample. A row
stops when its own ||z_new - z||_2 < tol and keeps z, the iterate before that step; one that reaches
max_iter keeps its last z_new. The reference tests `torch.all(diff < tol)` over the batch; with one
row the two rules are the same.

The gfx950 path is one kernel for all three kinds (csrc/nfx_lowrank*.hip): a stack of layers at one
dim in one launch, a single layer being a stack of one. Family: dim <= 64, num_transforms <= 8,
max_iter <= 1000, at most 256 layers. Gradients recompute through the composite by default
(HipFlowFunction's recompute route, counted in STATS["torch"]).

With `fused_backward = True` (on a class or an instance, default off) the gradients come from the fused
backward (csrc/nfx_lowrank_bwd*.hip), in HIP only, in train and eval mode alike: a single layer in
either direction, and the `inverse` (so log_prob and nll) of a SequentialFlow or NormalizingFlowModel
made only of these layers at one dim, every one with the switch on and no between-layer BatchNorm, as ONE
forward launch that saves only its output and ONE backward launch for the whole stack (up to
`max_fused_backward_layers(dim)` layers, the LDS budget of the gradient accumulators; a longer stack, and
`forward` under grad, run layer by layer, each layer with its own fused backward).
ONE DELIBERATE DIFFERENCE there: the composite differentiates the unrolled fixed-point iteration; the
fused backward of `inverse` returns the implicit-function gradient (I + J_g(z))^-T at the returned z,
the gradient of the function the iteration approximates. The two differ by about K rho^K (rho the
contraction, K the steps): measured in float64 between the own-settings unrolled gradient and the
converged one, 5e-7 .. 2.8e-4 of max|grad| for single layers at bounds 0.31 and 0.6, 7e-4 for a
five-layer mixed stack (tests/test_lowrank_backward_cpu.py prints it per case). A row with a non-finite z, cotangent or per-row coefficient adds nothing to the
parameter gradients and gets a zero input gradient, where autograd on the composite gives NaN. Double
backward is not supported there.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .flow import HipFlow, STATS

MAX_DIM = 64
MAX_TRANSFORMS = 8
MAX_ITER = 1000
MAX_LAYERS = 256


def _rows_dot(z, w):
    """torch.mv(z, w) as a per-row sum: a BLAS call may block by the batch size, and a row's result
    must not depend on the rows beside it (the composite's sums are row-wise throughout)."""
    return (z * w.unsqueeze(0)).sum(dim=-1)


def _rows_mm(a, m):
    """torch.mm(a, m.t()) for a [B, k], m [n, k], row-wise as _rows_dot."""
    return (a.unsqueeze(1) * m.unsqueeze(0)).sum(dim=-1)


def _guard(log_det):
    return torch.where(torch.isnan(log_det) | torch.isinf(log_det), torch.zeros_like(log_det), log_det)


def max_fused_backward_layers(dim):
    """Layers one fused stack backward takes at this dim: the stack's gradient image and the staging
    of one wave must fit the LDS of a workgroup (nfx_lrbwd_max_layers)."""
    return int(_lib.lib().nfx_lrbwd_max_layers(int(dim)))


class _LowRankFlow(HipFlow):
    """What the three kinds share: the fixed-point inverse, the routing and the one-record pack."""

    # True: gradients come from the fused backward kernels (csrc/nfx_lowrank_bwd*.hip) instead of a
    # recompute through the composite; see the module docstring for the implicit-gradient difference.
    fused_backward = False
    _KIND = None  # the record's kind code (csrc/nfx_lowrank_kernel.h)

    def _init_common(self, dim):
        self.data_dim = dim
        self.dim = dim
        self.max_iter = 50
        self.tol = 1e-6

    # -- the composite ----------------------------------------------------------------------------
    def _fixed_point(self, x, g):
        """z <- x - g(z) from z = x with the per-sample stopping rule."""
        z = x.clone()
        running = torch.ones(x.shape[0], dtype=torch.bool, device=x.device)
        for _ in range(self.max_iter):
            z_new = x - g(z)
            diff = torch.norm(z_new - z, dim=1)
            running = running & ~(diff < self.tol)
            if not bool(running.any()):
                break
            z = torch.where(running.unsqueeze(1), z_new, z)
        return z

    # -- gfx950 path ------------------------------------------------------------------------------
    def _family_reason(self):
        """'' inside the kernel family, else what is outside it."""
        if not 1 <= self.dim <= MAX_DIM:
            return f"dim={self.dim} outside 1..{MAX_DIM}"
        if not (isinstance(self.max_iter, int) and 0 <= self.max_iter <= MAX_ITER):
            return f"max_iter={self.max_iter!r} outside 0..{MAX_ITER}"
        return ""

    def _hip_supported(self, x):
        if x.dim() != 2 or x.shape[1] != self.dim:
            return False, f"input shape {tuple(x.shape)} vs dim={self.dim}"
        why = self._family_reason()
        if why:
            return False, why + " (the kernel family)"
        if not _lib.lib().nfx_lowrank_supported(max(x.shape[0], 1), self.dim, 1):
            return False, f"dim={self.dim} outside the kernel family"
        return True, ""

    def _state_key(self, device):
        return super()._state_key(device) + (self.max_iter, float(self.tol))

    def _dev(self, t, device):
        return _lib.dense(t.detach().to(device=device, dtype=torch.float32))

    def _build_pack(self, device):
        record = torch.empty(_lib.checked().nfx_lowrank_record_floats(self.dim), device=device, dtype=torch.float32)
        self._pack_record(record, device)
        return record

    def _hip_launch(self, x, out, log_det, direction, accumulate):
        record = self._packed(x.device, self._build_pack)
        _lib.checked().nfx_lowrank_stack(record, 1, x, out, log_det, x.shape[0], self.dim,
                                         _lib.NFX_FORWARD if direction > 0 else _lib.NFX_INVERSE,
                                         int(bool(accumulate)), _lib.stream_of(x))

    # -- fused backward (opt-in: fused_backward = True) ---------------------------------------------
    def _dispatch(self, x, direction):
        if (self.fused_backward and torch.is_grad_enabled() and self._route(x) == "hip"
                and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
                and self._hip_backward_ok(x, direction)):
            return _LowRankFunction.apply((self,), None, direction, x, *list(self.parameters()))
        return super()._dispatch(x, direction)

    def _hip_backward_ok(self, x, direction=-1):
        """The fused backward is switched on and has a kernel for this call."""
        if not (self.fused_backward and x.dim() == 2 and x.shape[1] == self.dim and x.shape[0] >= 1):
            return False
        if x.device.type != "cuda" or x.dtype != torch.float32 or self._family_reason():
            return False
        return bool(_lib.lib().nfx_lrbwd_supported(x.shape[0], self.dim, 1,
                                                   _lib.NFX_FORWARD if direction > 0 else _lib.NFX_INVERSE))

    def _hip_backward(self, x, gy, gld, direction=-1):
        """HipFlowFunction's hook: (gx, one gradient per entry of list(self.parameters())) from the
        layer's INPUT x. The inverse's Jacobian is taken at its output, which the forward kernel
        computes again here (_LowRankFunction, the route `_dispatch` takes, saves it instead)."""
        x = _lib.dense(x)
        point = x if direction > 0 else self._hip_call(x, -1)[0]
        record = self._packed(x.device, self._build_pack)
        gx, grads = _stack_backward((self,), record, point, gy, gld, direction)
        return gx, grads

    def _param_tensors(self, device):
        """(p0, p1, p2, num_householder, num_transforms, [(parameter, gradient slot)]) of
        nfx_lrbwd_param_grads: the parameters as the pack reads them and which output is whose."""
        raise NotImplementedError

    def _param_grads(self, ws, B, n_layers, layer):
        """This layer's parameter gradients from the reduced record gradients in `ws`, in
        list(self.parameters()) order; no launch when no parameter needs one."""
        params = list(self.parameters())
        if not any(p.requires_grad for p in params):
            return [None] * len(params)
        p0, p1, p2, nh, nt, shapes = self._param_tensors(ws.device)
        outs = [torch.empty(shape, device=ws.device, dtype=torch.float32) for shape in shapes]
        _lib.checked().nfx_lrbwd_param_grads(ws, B, self.dim, n_layers, layer, self._KIND, p0, p1, p2, outs[0], outs[1],
                                             outs[2], nh, nt, _lib.stream_of(ws))
        return self._grads_in_order(outs)

    def _grads_in_order(self, outs):
        return outs


class PlanarFlow(_LowRankFlow):
    """Planar flow (planar_flow.py): z + u tanh(w.z + b)."""

    def __init__(self, dim):
        super().__init__()
        self._init_common(dim)
        self.w = nn.Parameter(torch.randn(dim))
        self.u_hat = nn.Parameter(torch.randn(dim))
        self.b = nn.Parameter(torch.randn(1))
        self._initialize_parameters()

    def _initialize_parameters(self):
        nn.init.normal_(self.w, mean=0, std=0.1)
        nn.init.normal_(self.u_hat, mean=0, std=0.1)
        nn.init.normal_(self.b, mean=0, std=0.1)

    def _get_u(self, dtype=None):
        """The constrained u, with u.w >= -1."""
        w, u_hat = self.w, self.u_hat
        if dtype is not None and dtype != w.dtype:
            w, u_hat = w.to(dtype), u_hat.to(dtype)
        wtu = torch.dot(w, u_hat)
        m = -1 + torch.log1p(torch.exp(wtu))
        return u_hat + (m - wtu) * w / (torch.sum(w ** 2) + 1e-8)

    def _log_det(self, z, u, w, b):
        psi = 1 - torch.tanh(_rows_dot(z, w) + b) ** 2
        return _guard(torch.log(torch.abs(1 + torch.dot(u, w) * psi) + 1e-8))

    def _torch_call(self, x, direction):
        u, w, b = self._get_u(x.dtype), self.w.to(x.dtype), self.b.to(x.dtype)

        def g(z):
            return u.unsqueeze(0) * torch.tanh(_rows_dot(z, w) + b).unsqueeze(1)

        if direction > 0:
            return x + g(x), self._log_det(x, u, w, b)
        z = self._fixed_point(x, g)
        return z, -self._log_det(z, u, w, b)

    _KIND = 0

    def _param_tensors(self, device):
        return (self._dev(self.w, device), self._dev(self.u_hat, device), self._dev(self.b, device), 0, 0,
                [self.w.shape, self.u_hat.shape, self.b.shape])

    def _pack_record(self, record, device):
        _lib.checked().nfx_lowrank_pack_planar(self._dev(self.w, device), self._dev(self.u_hat, device),
                                               self._dev(self.b, device), self.dim, self.max_iter, float(self.tol),
                                               record, _lib.stream_of(record))


class RadialFlow(_LowRankFlow):
    """Radial flow (radial_flow.py): z + beta h(alpha, r) (z - z0)."""

    def __init__(self, dim):
        super().__init__()
        self._init_common(dim)
        self.z0 = nn.Parameter(torch.randn(dim))
        self.alpha_hat = nn.Parameter(torch.randn(1))
        self.beta_hat = nn.Parameter(torch.randn(1))
        self._initialize_parameters()

    def _initialize_parameters(self):
        nn.init.normal_(self.z0, mean=0, std=0.1)
        nn.init.normal_(self.alpha_hat, mean=0, std=0.1)
        nn.init.normal_(self.beta_hat, mean=0, std=0.1)

    def _get_alpha(self, dtype=None):
        a = self.alpha_hat
        return F.softplus(a if dtype is None else a.to(dtype))

    def _get_beta(self, alpha):
        return -alpha + F.softplus(self.beta_hat.to(alpha.dtype))

    def _log_det(self, z, z0, alpha, beta):
        r = torch.norm(z - z0.unsqueeze(0), dim=1, keepdim=True)
        h = 1.0 / (alpha + r + 1e-8)
        h_prime = -1.0 / ((alpha + r) ** 2 + 1e-8)
        term1 = 1 + beta * h
        term2 = 1 + beta * h + beta * h_prime * r
        ld = (self.dim - 1) * torch.log(torch.abs(term1) + 1e-8) + torch.log(torch.abs(term2) + 1e-8)
        return _guard(ld.squeeze(1))

    def _torch_call(self, x, direction):
        alpha = self._get_alpha(x.dtype)
        beta = self._get_beta(alpha)
        z0 = self.z0.to(x.dtype)

        def g(z):
            d = z - z0.unsqueeze(0)
            r = torch.norm(d, dim=1, keepdim=True)
            return beta * (1.0 / (alpha + r + 1e-8)) * d

        if direction > 0:
            return x + g(x), self._log_det(x, z0, alpha, beta)
        z = self._fixed_point(x, g)
        return z, -self._log_det(z, z0, alpha, beta)

    _KIND = 1

    def _param_tensors(self, device):
        return (self._dev(self.z0, device), self._dev(self.alpha_hat, device), self._dev(self.beta_hat, device), 0, 0,
                [self.z0.shape, self.alpha_hat.shape, self.beta_hat.shape])

    def _pack_record(self, record, device):
        _lib.checked().nfx_lowrank_pack_radial(self._dev(self.z0, device), self._dev(self.alpha_hat, device),
                                               self._dev(self.beta_hat, device), self.dim, self.max_iter,
                                               float(self.tol), record, _lib.stream_of(record))


class HouseholderReflection(nn.Module):
    """H = I - 2 v v^T / (|v|^2 + 1e-8) (sylvester_flow.py)."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.v = nn.Parameter(torch.randn(dim))
        self._initialize_parameters()

    def _initialize_parameters(self):
        nn.init.normal_(self.v, mean=0, std=0.1)

    def forward(self, x):
        v = self.v.to(x.dtype)
        v_norm_sq = torch.sum(v ** 2) + 1e-8
        if x.dim() == 1:
            return x - 2 * v * torch.dot(v, x) / v_norm_sq
        return x - 2 * v.unsqueeze(0) * _rows_dot(x, v).unsqueeze(1) / v_norm_sq

    def get_matrix(self):
        v_norm_sq = torch.sum(self.v ** 2) + 1e-8
        eye = torch.eye(self.dim, device=self.v.device, dtype=self.v.dtype)
        return eye - 2 * torch.outer(self.v, self.v) / v_norm_sq


class OrthogonalMatrix(nn.Module):
    """A product of at most `dim` Householder reflections, applied in list order."""

    def __init__(self, dim, num_householder=8):
        super().__init__()
        self.dim = dim
        self.num_householder = min(num_householder, dim)
        self.reflections = nn.ModuleList([HouseholderReflection(dim) for _ in range(self.num_householder)])

    def forward(self, x):
        for reflection in self.reflections:
            x = reflection(x)
        return x

    def get_matrix(self):
        """H_K ... H_1: the matrix that `forward` applies to a column vector."""
        v0 = self.reflections[0].v
        q = torch.eye(self.dim, device=v0.device, dtype=v0.dtype)
        for reflection in self.reflections:
            q = torch.mm(reflection.get_matrix(), q)
        return q

    def log_det(self):
        """log|det Q| = 0: every reflection has determinant -1."""
        return torch.log(torch.abs(torch.tensor((-1) ** self.num_householder, dtype=torch.float32)))


class SylvesterFlow(_LowRankFlow):
    """Sylvester flow (sylvester_flow.py): z + Q(tanh(Q(z) R^T + b) R)."""

    def __init__(self, dim, num_householder=8, num_transforms=None):
        super().__init__()
        self._init_common(dim)
        self.num_householder = min(num_householder, dim)
        self.num_transforms = num_transforms if num_transforms is not None else dim
        self.Q = OrthogonalMatrix(dim, num_householder)
        self.R = nn.Parameter(torch.randn(self.num_transforms, dim))
        self.b = nn.Parameter(torch.randn(self.num_transforms))
        self._initialize_parameters()

    def _initialize_parameters(self):
        nn.init.xavier_normal_(self.R, gain=0.1)
        nn.init.normal_(self.b, mean=0, std=0.1)

    def _activation(self, z, R, b):
        return torch.tanh(_rows_mm(self.Q(z), R) + b.unsqueeze(0))

    def _compute_log_det(self, z, activation):
        """The reference's formula, for the whole batch at once."""
        R = self.R.to(z.dtype)
        psi = 1 - activation ** 2
        rrt = torch.mm(R, R.t())
        eye = torch.eye(self.num_transforms, device=z.device, dtype=z.dtype)
        matrix = eye.unsqueeze(0) + rrt.unsqueeze(0) * psi.unsqueeze(1)  # I + R R^T diag(psi), per row
        return _guard(torch.log(torch.abs(torch.linalg.det(matrix)) + 1e-8))

    def _torch_call(self, x, direction):
        R, b = self.R.to(x.dtype), self.b.to(x.dtype)

        def g(z):
            return self.Q(_rows_mm(self._activation(z, R, b), R.t()))

        if direction > 0:
            act = self._activation(x, R, b)
            return x + self.Q(_rows_mm(act, R.t())), self._compute_log_det(x, act)
        z = self._fixed_point(x, g)
        return z, -self._compute_log_det(z, self._activation(z, R, b))

    def get_orthogonal_matrix(self):
        return self.Q.get_matrix()

    def check_orthogonality(self):
        q = self.get_orthogonal_matrix()
        eye = torch.eye(self.dim, device=q.device, dtype=q.dtype)
        return torch.norm(torch.mm(q.t(), q) - eye, p="fro")

    def _family_reason(self):
        why = super()._family_reason()
        if not why and not 1 <= self.num_transforms <= MAX_TRANSFORMS:
            why = f"num_transforms={self.num_transforms} outside 1..{MAX_TRANSFORMS}"
        return why

    _KIND = 2

    def _param_tensors(self, device):
        refl = list(self.Q.reflections)
        v = torch.stack([self._dev(r.v, device) for r in refl]) if refl else None
        return (v, self._dev(self.R, device), self._dev(self.b, device), len(refl), self.num_transforms,
                [(max(len(refl), 1), self.dim), self.R.shape, self.b.shape])

    def _grads_in_order(self, outs):
        gv, gR, gb = outs
        by_param = {id(self.R): gR, id(self.b): gb}
        for k, r in enumerate(self.Q.reflections):
            by_param[id(r.v)] = gv[k]
        return [by_param[id(p)] for p in self.parameters()]

    def _pack_record(self, record, device):
        refl = list(self.Q.reflections)
        v = torch.stack([self._dev(r.v, device) for r in refl]) if refl else None
        _lib.checked().nfx_lowrank_pack_sylvester(v, self._dev(self.R, device), self._dev(self.b, device), self.dim,
                                                  len(refl), self.num_transforms, self.max_iter, float(self.tol),
                                                  record, _lib.stream_of(record))


# ---- a stack of these layers in one launch ------------------------------------------------------
_KINDS = (PlanarFlow, RadialFlow, SylvesterFlow)


def chain_ok(flows, x):
    """Every layer one of the three kinds, inside the kernel family, at one dim; fp32 ROCm rows."""
    if not flows or len(flows) > MAX_LAYERS or x.dim() != 2 or x.device.type != "cuda" or x.dtype != torch.float32:
        return False
    dim = x.shape[1]
    for f in flows:
        if type(f) not in _KINDS or f.dim != dim or f._family_reason():
            return False
    return bool(_lib.lib().nfx_lowrank_supported(max(x.shape[0], 1), dim, len(flows)))


def _stack_image(flows, device, owner):
    """The stack's device image, cached on `owner` (the container; the first layer without one) and
    keyed on every layer's state key: a layer whose key changed re-packs its own record only."""
    owner = owner if owner is not None else flows[0]
    keys = [f._state_key(device) for f in flows]
    ident = (device, tuple(id(f) for f in flows))
    cache = owner.__dict__.get("_nfx_lowrank_pack_cache")
    if cache is None or cache[0] != ident:
        rec = _lib.checked().nfx_lowrank_record_floats(flows[0].dim)
        cache = [ident, [None] * len(flows), torch.empty(len(flows) * rec, device=device, dtype=torch.float32), rec]
        object.__setattr__(owner, "_nfx_lowrank_pack_cache", cache)
    _, have, image, rec = cache
    for i, (f, key) in enumerate(zip(flows, keys)):
        if have[i] != key:
            f._pack_record(image[i * rec:(i + 1) * rec], device)
            have[i] = key
    return image


def chain_launch(flows, x, out, ld, direction, accumulate, owner=None):
    """All `flows` (module order; the kernel reverses them for the inverse) in one
    nfx_lowrank_stack launch. No fused Gaussian log-density: the caller runs nfx_gauss_logprob."""
    image = _stack_image(flows, x.device, owner)
    _lib.checked().nfx_lowrank_stack(image, len(flows), x, out, ld, x.shape[0], flows[0].dim,
                                     _lib.NFX_FORWARD if direction > 0 else _lib.NFX_INVERSE, int(bool(accumulate)),
                                     _lib.stream_of(x))
    STATS["hip"] += 1


# ---- the fused backward: one layer in either direction, or a whole stack's inverse -----------------
def _stack_backward(flows, image, point, gv, gld, direction):
    """(gx, [one gradient per parameter of every layer, in order]) from one nfx_lrbwd_stack launch (and
    its fixed-order reduction), then one nfx_lrbwd_param_grads launch per layer. HIP only."""
    L = _lib.checked()
    B, dim, n = point.shape[0], flows[0].dim, len(flows)
    gv = _lib.dense(gv.to(torch.float32))
    gld = _lib.dense(gld.to(torch.float32))
    gx = torch.empty_like(point)
    ws = torch.empty(L.nfx_lrbwd_workspace_floats(B, dim, n), device=point.device, dtype=torch.float32)
    L.nfx_lrbwd_stack(image, n, point, gv, gld, gx, ws, B, dim,
                      _lib.NFX_FORWARD if direction > 0 else _lib.NFX_INVERSE, _lib.stream_of(point))
    grads = []
    for i, f in enumerate(flows):
        grads += f._param_grads(ws, B, n, i)
    return gx, grads


class _LowRankFunction(torch.autograd.Function):
    """`flows` (one layer, either direction; or a stack, inverse only) with the fused backward: the
    forward kernel as it stands in one launch, saving the point the Jacobian is taken at (the input
    for forward, the OUTPUT z for inverse), then the sweep in HIP. No composite anywhere; double
    backward is not supported."""

    @staticmethod
    def forward(ctx, flows, owner, direction, x, *params):
        x = _lib.dense(x)
        with torch.no_grad():
            if len(flows) == 1:
                y, ld = flows[0]._hip_call(x.detach(), direction)  # (counts STATS["hip"])
            else:
                y = torch.empty_like(x)
                ld = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
                chain_launch(list(flows), x.detach(), y, ld, direction, False, owner=owner)
        ctx.flows, ctx.owner, ctx.direction = flows, owner, direction
        ctx.save_for_backward(x if direction > 0 else y)
        return y, ld

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy, gld):
        (point,) = ctx.saved_tensors
        flows = ctx.flows
        STATS["hip"] += 1
        if len(flows) == 1:
            image = flows[0]._packed(point.device, flows[0]._build_pack)
        else:
            image = _stack_image(list(flows), point.device, ctx.owner)
        gx, grads = _stack_backward(flows, image, point.detach(), gy, gld, ctx.direction)
        params = [p for f in flows for p in f.parameters()]
        grads = [g if p.requires_grad else None for p, g in zip(params, grads)]
        return (None, None, None, gx, *grads)


def fused_stack_ok(flows, x):
    """`inverse` of these layers under grad as one forward and one backward launch: every layer one
    of the three kinds with the switch on, one dim, fp32 ROCm rows, within the backward's budget."""
    if not torch.is_grad_enabled() or len(flows) < 2 or not chain_ok(flows, x) or x.shape[0] < 1:
        return False
    if not all(f.fused_backward for f in flows):
        return False
    if not (x.requires_grad or any(p.requires_grad for f in flows for p in f.parameters())):
        return False
    return bool(_lib.lib().nfx_lrbwd_supported(x.shape[0], x.shape[1], len(flows), _lib.NFX_INVERSE))


def fused_stack_inverse(flows, x, owner=None):
    """(z, log_det) of the stack's inverse with the one-launch fused backward behind it."""
    return _LowRankFunction.apply(tuple(flows), owner, -1, x, *[p for f in flows for p in f.parameters()])
