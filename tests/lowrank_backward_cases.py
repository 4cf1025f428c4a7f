"""Shared references of the Planar / Radial / Sylvester backward tests (test_lowrank_backward_cpu.py,
test_gpu_lowrank_backward.py).

The oracle is float64 autograd of the composite RUN TO CONVERGENCE (`converged`: max_iter 400, tol 0),
not of the layer's own 50-step iteration: the fused backward returns the implicit-function gradient at
the returned z, and the unrolled gradient at the layer's own settings is itself up to 3.5e-4 away from
the converged one. `recurrence_grads` is the sweep of csrc/nfx_lowrank_bwd_kernel.h and the
record-to-parameter adjoint of csrc/nfx_lowrank_bwd.hip written out by hand, with no autograd."""
import copy

import torch

from lowrank_cases import kind_of

EPS = 1e-8


def cotangents(B, d, seed=0):
    """Random (gz [B, d], gld [B]) from a seeded generator."""
    g = torch.Generator().manual_seed(8300 + seed)
    return torch.randn(B, d, generator=g), torch.randn(B, generator=g)


def as_list(flows):
    return list(flows) if isinstance(flows, (list, tuple, torch.nn.ModuleList)) else [flows]


def converged(flow, dtype=torch.float64):
    """A deep copy in `dtype` whose inverse runs to convergence: max_iter = 400, tol = 0."""
    f = copy.deepcopy(flow).to(dtype)
    f.max_iter, f.tol = 400, 0.0
    return f


def names(flows):
    """"gx", then every layer's parameter names in order ("<layer>.<name>" for a list)."""
    flows = as_list(flows)
    if len(flows) == 1:
        return ["gx"] + [n for n, _ in flows[0].named_parameters()]
    return ["gx"] + [f"{i}.{n}" for i, f in enumerate(flows) for n, _ in f.named_parameters()]


def run(flows, x, direction):
    """The layers in order (forward) or reversed (inverse): (y, total log-det)."""
    ld = 0
    for f in (flows if direction > 0 else reversed(flows)):
        x, l = f.forward(x) if direction > 0 else f.inverse(x)
        ld = ld + l
    return x, ld


def autograd_grads(flows, x, gz, gld, direction):
    """[gx, one gradient per parameter] of <gz, y> + <gld, ld> by autograd through the CPU composite,
    in the dtype of `flows` (a layer or a list of layers) and with their own max_iter / tol."""
    flows = as_list(flows)
    params = [p for f in flows for p in f.parameters()]
    dt = params[0].dtype
    xr = x.detach().to(dt).clone().requires_grad_(True)
    y, ld = run(flows, xr, direction)
    grads = torch.autograd.grad([y, ld], [xr] + params, [gz.to(dt), gld.to(dt)], allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(grads, [xr] + params)]


def references(flows, x, gz, gld, direction):
    """(g64, g32): float64 and fp32 autograd of the converged composite."""
    flows = as_list(flows)
    g64 = autograd_grads([converged(f) for f in flows], x, gz, gld, direction)
    g32 = autograd_grads([converged(f, torch.float32) for f in flows], x, gz, gld, direction)
    return g64, g32


def gclose(a, b, what, ref32, frac=2e-4):
    """The project's criterion for these gradients (naf_backward_cases.gclose):
    max|a - b| <= max(frac * max|b|, 4 * max|ref32 - b|)."""
    a, b, r = (t.detach().cpu().double() for t in (a, b, ref32))
    err = (a - b).abs().max().item()
    bound = max(frac * max(b.abs().max().item(), 1e-30), 4 * (r - b).abs().max().item())
    print(f"[lowrank bwd] {what}: max err {err:.3e} (bound {bound:.3e}, fp32 composite {(r - b).abs().max().item():.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


# ---- the recurrences, by hand ---------------------------------------------------------------------
def record(flow):
    """The float64 entries of the layer's packed record (csrc/nfx_lowrank.hip)."""
    sd = {k: v.detach().double() for k, v in flow.state_dict().items()}
    kind = kind_of(flow)
    if kind == "planar":
        w, u_hat = sd["w"], sd["u_hat"]
        s, n = torch.dot(w, u_hat), torch.dot(w, w)
        coef = (-1 + torch.log1p(torch.exp(s)) - s) / (n + EPS)
        u = u_hat + coef * w
        return {"w": w, "u": u, "b": sd["b"][0], "c": torch.dot(u, w)}
    if kind == "radial":
        alpha = torch.nn.functional.softplus(sd["alpha_hat"][0])
        return {"z0": sd["z0"], "alpha": alpha, "beta": -alpha + torch.nn.functional.softplus(sd["beta_hat"][0])}
    vs = [sd[f"Q.reflections.{k}.v"] for k in range(len(flow.Q.reflections))]
    q = torch.eye(flow.dim, dtype=torch.float64)
    for v in vs:
        q = (torch.eye(flow.dim, dtype=torch.float64) - 2 * torch.outer(v, v) / (torch.dot(v, v) + EPS)) @ q
    R = sd["R"]
    return {"A": R @ q, "Bt": R @ q.t(), "S": R @ R.t(), "bias": sd["b"], "Q": q, "R": R, "v": vs}


def _dlogabs(d):
    return torch.sign(d) / (d.abs() + EPS)


def _col(t):
    return t.unsqueeze(1)


def sweep_layer(kind, rec, dim, z, cot, lbar, direction, adjoint_steps=400):
    """One layer of the sweep at the point z (forward: its input; inverse: its output).
    Returns (the outgoing cotangent, the record gradients, g(z))."""
    sg = 1.0 if direction > 0 else -1.0
    zero = torch.zeros_like(lbar)
    if kind == "planar":
        w, u, b, c = rec["w"], rec["u"], rec["b"], rec["c"]
        t = torch.tanh(z @ w + b)
        psi = 1 - t * t
        D = 1 + c * psi
        lb = torch.where(torch.isfinite(torch.log(D.abs() + EPS)), lbar, zero)
        sD = _dlogabs(D)
        le = lb * sD * c * (-2 * t * psi)
        if direction > 0:
            v = cot
        else:
            lam = cot - _col(le) * w
            v = lam - _col(psi * (lam @ u) / D) * w
        abar = (v @ u) * psi + le
        grads = {"w": sg * (_col(abar) * z).sum(0), "b": sg * abar.sum(), "u": sg * (_col(t) * v).sum(0),
                 "c": sg * (lb * sD * psi).sum()}
        return (v + _col(abar) * w if direction > 0 else v), grads, _col(t) * u
    if kind == "radial":
        z0, alpha, beta = rec["z0"], rec["alpha"], rec["beta"]
        d = z - z0
        r = d.norm(dim=1)
        ar = alpha + r
        h = 1 / (ar + EPS)
        hp = -1 / (ar * ar + EPS)
        dh = -h * h
        dhp = 2 * ar * hp * hp
        t1 = 1 + beta * h
        t2 = t1 + beta * hp * r
        ld = (dim - 1) * torch.log(t1.abs() + EPS) + torch.log(t2.abs() + EPS)
        lb = torch.where(torch.isfinite(ld), lbar, zero)
        s1, s2 = (dim - 1) * _dlogabs(t1), _dlogabs(t2)
        ld_r = s1 * beta * dh + s2 * (beta * dh + beta * (dhp * r + hp))
        ld_a = s1 * beta * dh + s2 * (beta * dh + beta * r * dhp)
        ld_b = s1 * h + s2 * (h + hp * r)
        invr = torch.where(r > 0, 1 / r, torch.zeros_like(r))
        if direction > 0:
            v = cot
        else:
            lam = cot - _col(lb * ld_r * invr) * d
            v = lam / _col(t1) - _col(beta * dh * invr * (d * lam).sum(1) / (t1 * (t1 + beta * dh * r))) * d
        dv = (d * v).sum(1)
        kappa = (beta * dh * dv + lb * ld_r) * invr
        part = _col(beta * h) * v + _col(kappa) * d
        grads = {"z0": -sg * part.sum(0), "alpha": sg * (beta * dh * dv + lb * ld_a).sum(),
                 "beta": sg * (h * dv + lb * ld_b).sum()}
        return (v + part if direction > 0 else v), grads, _col(beta * h) * d
    A, Bt, S, bias = rec["A"], rec["Bt"], rec["S"], rec["bias"]
    M = S.shape[0]
    t = torch.tanh(z @ A.t() + bias)
    psi = 1 - t * t
    mat = torch.eye(M, dtype=z.dtype) + S.unsqueeze(0) * psi.unsqueeze(1)  # I + S D per row
    det = torch.linalg.det(mat)
    lb = torch.where(torch.isfinite(torch.log(det.abs() + EPS)), lbar * det.abs() / (det.abs() + EPS), zero)
    W = torch.linalg.inv(mat)
    le = _col(lb) * torch.diagonal(W @ S, dim1=1, dim2=2) * (-2 * t * psi)
    s_row = W.transpose(1, 2) * psi.unsqueeze(1)  # [i][j] = psi_j W[j][i]
    if direction > 0:
        v = cot
    else:
        lam0 = cot - le @ A
        v = lam0
        for _ in range(adjoint_steps):
            v = lam0 - ((v @ Bt.t()) * psi) @ A
    abar = (v @ Bt.t()) * psi + le
    grads = {"A": sg * abar.t() @ z, "bias": sg * abar.sum(0), "Bt": sg * t.t() @ v,
             "S": sg * (lb[:, None, None] * s_row).sum(0)}
    return (v + abar @ A if direction > 0 else v), grads, t @ Bt


def param_grads(flow, rec, g):
    """The adjoint of the pack: record gradients -> one gradient per parameter, in parameters() order."""
    kind = kind_of(flow)
    sd = {k: v.detach().double() for k, v in flow.state_dict().items()}
    if kind == "planar":
        w, u_hat = sd["w"], sd["u_hat"]
        s, n = torch.dot(w, u_hat), torch.dot(w, w)
        coef = (-1 + torch.log1p(torch.exp(s)) - s) / (n + EPS)
        ubar = g["u"] + g["c"] * w
        coefbar = torch.dot(ubar, w)
        sbar = coefbar * (torch.sigmoid(s) - 1) / (n + EPS)
        nbar = -coefbar * coef / (n + EPS)
        out = {"w": g["w"] + g["c"] * rec["u"] + coef * ubar + sbar * u_hat + 2 * nbar * w,
               "u_hat": ubar + sbar * w, "b": g["b"].reshape(1)}
    elif kind == "radial":
        out = {"z0": g["z0"], "alpha_hat": ((g["alpha"] - g["beta"]) * torch.sigmoid(sd["alpha_hat"][0])).reshape(1),
               "beta_hat": (g["beta"] * torch.sigmoid(sd["beta_hat"][0])).reshape(1)}
    else:
        q, R, vs = rec["Q"], rec["R"], rec["v"]
        out = {"R": g["A"] @ q.t() + g["Bt"] @ q + (g["S"] + g["S"].t()) @ R, "b": g["bias"]}
        T = (R.t() @ g["A"] + g["Bt"].t() @ R) @ q.t()  # Qm_bar Qm^T
        for k in reversed(range(len(vs))):
            v = vs[k]
            n = torch.dot(v, v)
            c = 2 / (n + EPS)
            Mk = T - (c / (c * n - 1)) * torch.outer(T @ v, v)  # T H_k^-1
            mv = Mk @ v
            out[f"Q.reflections.{k}.v"] = c * c * torch.dot(v, mv) * v - c * (mv + Mk.t() @ v)
            T = Mk - c * torch.outer(v, v @ Mk)  # H_k M
    return [out[n] for n, _ in flow.named_parameters()]


def recurrence_grads(flows, x, gz, gld, direction):
    """[gx, one gradient per parameter] by the hand-written sweep in float64, no autograd anywhere.
    Inverse: the converged z is the point, the layers are swept first to last and z <- z + g(z) steps
    to the next layer's output. Forward: the inputs are kept and the layers swept last to first."""
    flows = as_list(flows)
    with torch.no_grad():
        recs = [record(f) for f in flows]
        x, cot, lbar = x.double(), gz.double(), gld.double()
        per_layer = [None] * len(flows)
        if direction < 0:
            z, _ = run([converged(f) for f in flows], x, -1)
            for i, (f, rec) in enumerate(zip(flows, recs)):
                cot, g, step = sweep_layer(kind_of(f), rec, f.dim, z, cot, lbar, -1)
                per_layer[i] = param_grads(f, rec, g)
                z = z + step
        else:
            points, z = [], x
            for f, rec in zip(flows, recs):
                points.append(z)
                z = z + sweep_layer(kind_of(f), rec, f.dim, z, torch.zeros_like(z), torch.zeros_like(lbar), 1)[2]
            for i in reversed(range(len(flows))):
                cot, g, _ = sweep_layer(kind_of(flows[i]), recs[i], flows[i].dim, points[i], cot, lbar, 1)
                per_layer[i] = param_grads(flows[i], recs[i], g)
    return [cot] + [g for gs in per_layer for g in gs]
