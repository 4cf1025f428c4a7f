"""Shared references of the ContinuousFlow backward tests (test_cnf_backward_cpu.py,
test_gpu_cnf_backward.py): autograd on the CPU composite, and the reverse sweep of the discrete
RK4 scheme written out by hand (the recurrences csrc/nfx_cnf_bwd_kernel.h implements)."""
import torch

from cnf_cases import as_double


def cotangents(B, d, seed=0):
    """Random (gy [B, d], gld [B]) from a seeded generator."""
    g = torch.Generator().manual_seed(5200 + seed)
    return torch.randn(B, d, generator=g), torch.randn(B, generator=g)


def autograd_grads(flow, x, direction, gy, gld):
    """(gx, [gW1, gb1, gW2, gb2, gW3, gb3]) of <gy, y> + <gld, ld> by autograd on the composite, in
    the dtype of `flow` (CPU). `direction` is +1, -1 or a times tensor."""
    p = next(flow.parameters())
    xr = x.detach().to(p.dtype).clone().requires_grad_(True)
    y, ld = flow._torch_call(xr, direction)
    params = list(flow.parameters())
    grads = torch.autograd.grad([y, ld], [xr] + params, [gy.to(p.dtype), gld.to(p.dtype)], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, [xr] + params)]
    return grads[0], list(grads[1:])


def references(flow, x, direction, gy, gld):
    """(g64, g32): the float64 and the fp32 autograd gradients on the CPU composite, each flattened
    to [gx, gW1, gb1, gW2, gb2, gW3, gb3]."""
    gx64, gp64 = autograd_grads(as_double(flow), x, direction, gy, gld)
    gx32, gp32 = autograd_grads(flow, x, direction, gy, gld)
    return [gx64] + gp64, [gx32] + gp32


def preclamp(flow, x, direction):
    """(y_n, ld_n) of the composite before its guards, in x's dtype."""
    with torch.no_grad():
        grid = flow.time_grid(flow._times(direction)).to(x.dtype).unbind(0)
        f = flow.ode_func.velocity_and_trace
        y, ld = x, torch.zeros(x.shape[0], dtype=x.dtype)
        for t0, t1 in zip(grid[:-1], grid[1:]):
            dt = t1 - t0
            k1, l1 = f(t0, y)
            k2, l2 = f(t0 + dt / 3, y + dt * k1 / 3)
            k3, l3 = f(t0 + 2 * dt / 3, y + dt * (k2 - k1 / 3))
            k4, l4 = f(t1, y + dt * (k1 - k2 + k3))
            y = y + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
            ld = ld + (l1 + 3 * (l2 + l3) + l4) * dt * 0.125
    return y, ld


NAMES = ("gx", "W1", "b1", "W2", "b2", "W3", "b3")


def gclose(a, b, what, ref32, frac=2e-4):
    """The project's criterion for these gradients (tests/test_gpu_cnf.py, _gclose):
    max|a - b| <= max(frac * max|b|, 4 * max|ref32 - b|)."""
    a, b, r = (t.detach().cpu().double() for t in (a, b, ref32))
    err = (a - b).abs().max().item()
    bound = max(frac * max(b.abs().max().item(), 1e-30), 4 * (r - b).abs().max().item())
    print(f"[cnf bwd] {what}: max err {err:.3e} (bound {bound:.3e}, fp32 composite {(r - b).abs().max().item():.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def recurrence_grads(flow, x, direction, gy, gld):
    """The reverse sweep, literally, in the dtype of `flow`: no autograd anywhere. Returns
    (gx, [gW1, gb1, gW2, gb2, gW3, gb3])."""
    l1, l2, l3 = flow.ode_func.linears()
    W1, b1, W2, b2, W3, b3 = (t.detach() for t in (l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias))
    dt_ = W1.dtype
    d = flow.dim
    x, gy, gld = x.to(dt_), gy.to(dt_), gld.to(dt_)
    times = flow._times(direction)
    gW1, gb1, gW2, gb2 = (torch.zeros_like(t) for t in (W1, b1, W2, b2))
    gW3, gb3, gC = torch.zeros_like(W3), torch.zeros_like(b3), torch.zeros_like(W2)
    if bool(times[0] == times[1]):
        return gy.clone(), [gW1, gb1, gW2, gb2, gW3, gb3]
    N = W3.t() @ W1[:, :d].t()      # N[k, j] = sum_i W3[i, k] W1[j, i]
    C = W2 * N

    def field(t, z):
        zt = torch.cat([z, torch.full((z.shape[0], 1), float(t), dtype=dt_)], dim=1)
        h1 = torch.tanh(zt @ W1.t() + b1)
        h2 = torch.tanh(h1 @ W2.t() + b2)
        g1, g2 = 1 - h1 * h1, 1 - h2 * h2
        q = g1 @ C.t()
        return zt, h1, h2, g1, g2, q, h2 @ W3.t() + b3, (g2 * q).sum(1)

    def vjp(t, z, vb, tb):
        nonlocal gW1, gb1, gW2, gb2, gW3, gb3, gC
        zt, h1, h2, g1, g2, q, _, _ = field(t, z)
        qb = tb[:, None] * g2
        a2 = g2 * (vb @ W3 - 2 * h2 * (tb[:, None] * q))
        a1 = g1 * (a2 @ W2 - 2 * h1 * (qb @ C))
        gW3 += vb.t() @ h2
        gb3 += vb.sum(0)
        gW2 += a2.t() @ h1
        gb2 += a2.sum(0)
        gC += qb.t() @ g1
        gW1 += a1.t() @ zt
        gb1 += a1.sum(0)
        return a1 @ W1[:, :d]

    grid = flow.time_grid(times).to(dt_).unbind(0)
    ys, y, ld = [], x, torch.zeros(x.shape[0], dtype=dt_)
    for t0, t1 in zip(grid[:-1], grid[1:]):  # the forward, keeping y_k
        ys.append(y)
        dt = t1 - t0
        k1, t1_ = field(t0, y)[6:]
        k2, t2_ = field(t0 + dt / 3, y + dt * k1 / 3)[6:]
        k3, t3_ = field(t0 + 2 * dt / 3, y + dt * (k2 - k1 / 3))[6:]
        k4, t4_ = field(t1, y + dt * (k1 - k2 + k3))[6:]
        y = y + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        ld = ld + (t1_ + 3 * (t2_ + t3_) + t4_) * dt * 0.125
    yb = torch.where((y >= -10) & (y <= 10), gy, torch.zeros_like(gy))
    lb = torch.where((ld >= -10) & (ld <= 10), gld, torch.zeros_like(gld))
    for k in range(len(ys) - 1, -1, -1):
        t0, t1 = grid[k], grid[k + 1]
        dt = t1 - t0
        y = ys[k]
        k1 = field(t0, y)[6]
        z2 = y + dt * k1 / 3
        k2 = field(t0 + dt / 3, z2)[6]
        z3 = y + dt * (k2 - k1 / 3)
        k3 = field(t0 + 2 * dt / 3, z3)[6]
        z4 = y + dt * (k1 - k2 + k3)
        zb4 = vjp(t1, z4, dt / 8 * yb, dt / 8 * lb)
        zb3 = vjp(t0 + 2 * dt / 3, z3, 3 * dt / 8 * yb + dt * zb4, 3 * dt / 8 * lb)
        zb2 = vjp(t0 + dt / 3, z2, 3 * dt / 8 * yb - dt * zb4 + dt * zb3, 3 * dt / 8 * lb)
        zb1 = vjp(t0, y, dt / 8 * yb + dt * zb4 - dt / 3 * zb3 + dt / 3 * zb2, dt / 8 * lb)
        yb = yb + zb1 + zb2 + zb3 + zb4
    # finish: C = W2 * N
    gW2 = gW2 + gC * N
    Nb = gC * W2
    gW3 = gW3 + (Nb @ W1[:, :d]).t()
    gW1 = gW1.clone()
    gW1[:, :d] += Nb.t() @ W3.t()
    return yb, [gW1, gb1, gW2, gb2, gW3, gb3]
