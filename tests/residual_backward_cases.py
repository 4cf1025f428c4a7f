"""Shared references of the ResidualFlow backward tests (test_residual_backward_cpu.py,
test_gpu_residual_backward.py): autograd on the CONVERGED CPU composite, and the recurrences
csrc/nfx_residual_bwd_kernel.h implements written out in torch with no autograd.

The fused backward differentiates the inverse implicitly at the returned z. Autograd differentiates
the composite's unrolled iteration, which is the same gradient once the iteration has converged, so
the oracle is a copy of the layer with tol = 0 and enough iterations (`converged`)."""
import copy

import torch

from residual_cases import as_double

NAMES = ("gx", "W1", "b1", "W2", "b2", "W3", "b3")


def cotangents(B, d, seed=0):
    """Random (gy [B, d], gld [B]) from a seeded generator."""
    g = torch.Generator().manual_seed(7300 + seed)
    return torch.randn(B, d, generator=g), torch.randn(B, generator=g)


def _last_step(flow64, x64, n):
    """max over rows of ||z_(n+1) - z_n||_2 of the fixed-point iteration from z_0 = x, float64."""
    with torch.no_grad():
        z = x64.clone()
        for _ in range(n):
            z = x64 - flow64._residual_function(z)
        return float(torch.norm((x64 - flow64._residual_function(z)) - z, dim=1).max())


def converged(flow, dtype, x):
    """A copy of `flow` in `dtype` with tol = 0 and a max_iter at which the last step of its inverse
    on `x` is below 1e-14 in float64 (asserted). The iteration contracts at least by the layer's
    lipschitz_constant per step, so max_iter grows by 50 until the step is there."""
    f64 = as_double(flow)
    x64 = x.detach().double()
    n = 50
    while _last_step(f64, x64, n) >= 1e-14:
        n += 50
        assert n <= 3000, "the fixed-point iteration does not converge"
    out = f64 if dtype == torch.float64 else copy.deepcopy(flow)
    out.tol, out.max_iter = 0.0, n
    assert _last_step(f64, x64, out.max_iter) < 1e-14
    return out


def autograd_grads(flow, x, direction, gy, gld):
    """(gx, [gW1, gb1, gW2, gb2, gW3, gb3]) of <gy, y> + <gld, ld> by autograd on the composite, in
    the dtype of `flow` (CPU). gld = None: of <gy, y> alone."""
    p = next(flow.parameters())
    xr = x.detach().to(p.dtype).clone().requires_grad_(True)
    y, ld = flow._torch_call(xr, direction)
    params = list(flow.parameters())
    outs, cots = ([y], [gy.to(p.dtype)]) if gld is None else ([y, ld], [gy.to(p.dtype), gld.to(p.dtype)])
    grads = torch.autograd.grad(outs, [xr] + params, cots, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, [xr] + params)]
    return grads[0], list(grads[1:])


def references(flow, x, direction, gy, gld):
    """(g64, g32): the float64 and the fp32 autograd gradients of the converged CPU composite, each
    flattened to [gx, gW1, gb1, gW2, gb2, gW3, gb3]."""
    gx64, gp64 = autograd_grads(converged(flow, torch.float64, x), x, direction, gy, gld)
    gx32, gp32 = autograd_grads(converged(flow, torch.float32, x), x, direction, gy, gld)
    return [gx64] + gp64, [gx32] + gp32


def gclose(a, b, what, ref32, frac=2e-4):
    """The project's criterion for these gradients (cnf_backward_cases.gclose):
    max|a - b| <= max(frac * max|b|, 4 * max|ref32 - b|)."""
    a, b, r = (t.detach().cpu().double() for t in (a, b, ref32))
    err = (a - b).abs().max().item()
    bound = max(frac * max(b.abs().max().item(), 1e-30), 4 * (r - b).abs().max().item())
    print(f"[residual bwd] {what}: max err {err:.3e} (bound {bound:.3e}, fp32 composite "
          f"{(r - b).abs().max().item():.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def second_derivative(block, pre, out):
    """act'' as autograd differentiates the forms of ResidualBlock.derivative."""
    name = type(block.activation).__name__
    if name in ("ReLU", "LeakyReLU"):
        return torch.zeros_like(out)
    if name == "ELU":
        return torch.where(pre > 0, torch.zeros_like(out), out + 1)
    if name == "Tanh":
        return -2 * out * (1 - out * out)
    raise NotImplementedError(name)


def preactivations(flow, z):
    """(a1, a2) of the effective weights at z, in z's dtype."""
    block = flow.residual_block
    with torch.no_grad():
        (w1, b1), (w2, b2), _ = block.weights(z.dtype)
        a1 = z @ w1.t() + b1
        return a1, block.activation(a1) @ w2.t() + b2


def recurrence_grads(flow, x, direction, gy, gld):
    """The fused backward's recurrences, literally, in the dtype of `flow`: no autograd anywhere.
    The inverse takes z from the layer's own composite inverse (pass a converged layer) and
    differentiates implicitly there. Returns (gx, [gW1, gb1, gW2, gb2, gW3, gb3])."""
    block = flow.residual_block
    dt = next(flow.parameters()).dtype
    with torch.no_grad():
        x, gy, gld = x.detach().to(dt), gy.to(dt), gld.to(dt)
        (W1, b1), (W2, b2), (W3, b3) = [(w.detach(), b.detach()) for w, b in block.weights(dt)]
        H, d, n = W1.shape[0], W1.shape[1], flow.neumann_terms
        z = x if direction > 0 else flow._torch_call(x, -1)[0]
        B = z.shape[0]
        a1 = z @ W1.t() + b1
        h1 = block.activation(a1)
        g1, c1 = block.derivative(a1, h1), second_derivative(block, a1, h1)
        a2 = h1 @ W2.t() + b2
        h2 = block.activation(a2)
        g2, c2 = block.derivative(a2, h2), second_derivative(block, a2, h2)
        T1 = g1.unsqueeze(2) * W1.unsqueeze(0)          # [B, H, d]
        U = torch.matmul(W2, T1)
        T2 = g2.unsqueeze(2) * U
        J = torch.matmul(W3, T2)                        # [B, d, d]
        eye = torch.eye(d, dtype=dt).expand(B, d, d)

        def over_samples(a, b):
            """sum_s a[s] b[s]^T for a [B, m, d], b [B, k, d] without a [B, m, k] intermediate."""
            return a.permute(1, 0, 2).reshape(a.shape[1], -1) @ b.permute(1, 0, 2).reshape(b.shape[1], -1).t()

        def point(vb, lb):
            S, P = torch.zeros(B, d, d, dtype=dt), eye.clone()
            for k in range(1, n + 1):
                S = S + ((-1) ** (k + 1)) * P
                P = torch.bmm(P, J)
            G = lb.view(B, 1, 1) * S.transpose(1, 2)
            dT2 = torch.matmul(W3.t(), G)               # [B, H, d]
            dW3 = over_samples(G, T2) + vb.t() @ h2
            dg2 = (dT2 * U).sum(2)
            dU = g2.unsqueeze(2) * dT2
            dT1 = torch.matmul(W2.t(), dU)
            dg1 = (dT1 * W1.unsqueeze(0)).sum(2)
            ab2 = g2 * (vb @ W3) + c2 * dg2
            ab1 = g1 * (ab2 @ W2) + c1 * dg1
            dW2 = over_samples(dU, T1) + ab2.t() @ h1
            dW1 = (g1.unsqueeze(2) * dT1).sum(0) + ab1.t() @ z
            return ab1 @ W1, [dW1, ab1.sum(0), dW2, ab2.sum(0), dW3, vb.sum(0)]

        if direction > 0:
            zbar, gp = point(gy, gld)
            return gy + zbar, gp
        zbar, gp = point(torch.zeros_like(gy), -gld)
        w = torch.linalg.solve((eye + J).transpose(1, 2), (gy + zbar).unsqueeze(2)).squeeze(2)
        _, gp2 = point(-w, torch.zeros_like(gld))
        return w, [a + b for a, b in zip(gp, gp2)]
