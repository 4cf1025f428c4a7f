"""Shared references of the NeuralAutoregressiveFlow backward tests (test_naf_backward_cpu.py,
test_gpu_naf_backward.py): autograd on the CPU composite, and the reverse sweep of the density
direction written out by hand (the recurrences csrc/nfx_naf_bwd_kernel.h implements)."""
import math

import torch

from naf_cases import activation_name, as_double


def cotangents(B, d, seed=0):
    """Random (gz [B, d], gld [B]) from a seeded generator."""
    g = torch.Generator().manual_seed(6100 + seed)
    return torch.randn(B, d, generator=g), torch.randn(B, generator=g)


def names(flow):
    """"gx", then the parameter names in list(flow.parameters()) order."""
    return ["gx"] + [n for n, _ in flow.named_parameters()]


def autograd_grads(flow, x, gz, gld):
    """(gx, [one gradient per parameter]) of <gz, z> + <gld, ld> by autograd on the composite's density
    direction, in the dtype of `flow` (CPU)."""
    p = next(flow.parameters())
    xr = x.detach().to(p.dtype).clone().requires_grad_(True)
    z, ld = flow._torch_call(xr, -1)
    params = list(flow.parameters())
    grads = torch.autograd.grad([z, ld], [xr] + params, [gz.to(p.dtype), gld.to(p.dtype)], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, [xr] + params)]
    return grads[0], list(grads[1:])


def references(flow, x, gz, gld):
    """(g64, g32): the float64 and the fp32 autograd gradients on the CPU composite, each flattened
    to [gx, one per parameter]."""
    gx64, gp64 = autograd_grads(as_double(flow), x, gz, gld)
    gx32, gp32 = autograd_grads(flow, x, gz, gld)
    return [gx64] + gp64, [gx32] + gp32


def gclose(a, b, what, ref32, frac=2e-4):
    """The project's criterion for these gradients (cnf_backward_cases.gclose):
    max|a - b| <= max(frac * max|b|, 4 * max|ref32 - b|)."""
    a, b, r = (t.detach().cpu().double() for t in (a, b, ref32))
    err = (a - b).abs().max().item()
    bound = max(frac * max(b.abs().max().item(), 1e-30), 4 * (r - b).abs().max().item())
    print(f"[naf bwd] {what}: max err {err:.3e} (bound {bound:.3e}, fp32 composite {(r - b).abs().max().item():.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def _act(name, p):
    if name == "relu":
        return torch.relu(p)
    if name == "leaky_relu":
        return torch.where(p > 0, p, 0.1 * p)
    if name == "elu":
        return torch.where(p > 0, p, torch.expm1(p))
    return p * 0.5 * (1 + torch.erf(p / math.sqrt(2.0)))


def _dact(name, p):
    one = torch.ones_like(p)
    if name == "relu":
        return torch.where(p > 0, one, 0 * one)
    if name == "leaky_relu":
        return torch.where(p > 0, one, 0.1 * one)
    if name == "elu":
        return torch.where(p > 0, one, torch.exp(p))
    return 0.5 * (1 + torch.erf(p / math.sqrt(2.0))) + p * torch.exp(-0.5 * p * p) / math.sqrt(2 * math.pi)


def trace(flow, x):
    """The density direction in the dtype of `flow`, every intermediate kept, no autograd: a dict with
    per hidden layer (input h, x^ or None, rstd or None, pre-activation p), the last hidden output,
    the conditioner output o before its clamp, alpha after the +-2 clamp, -clamp(alpha), the
    log-scale, z and the log-det before their guards."""
    with torch.no_grad():
        hidden, out = flow.conditioner.plan()
        act = activation_name(flow)
        d = flow.dim
        ca, cl = flow.clamp_alpha, flow.clamp_log_scale
        h, keep = x, []
        for lin, ln, _, res in hidden:
            u = h @ (lin.weight * lin.mask).t() + lin.bias
            if ln is not None:
                mean = u.mean(1, keepdim=True)
                rstd = 1 / torch.sqrt(((u - mean) ** 2).mean(1, keepdim=True) + ln.eps)
                xh = (u - mean) * rstd
                p = xh * ln.weight + ln.bias
            else:
                xh, rstd, p = None, None, u
            keep.append((h, xh, rstd, p))
            a = _act(act, p)
            h = a + h if res else a
        o = h @ (out.weight * out.mask).t() + out.bias
        oc = o.clamp(-2.0, 2.0)
        mu, alpha = oc[:, :d], oc[:, d:]
        nls = -alpha.clamp(-ca, ca)
        ls = nls.clamp(-cl, cl)
        e = torch.exp(ls)
        return {"layers": keep, "h": h, "o": o, "mu": mu, "alpha": alpha, "nls": nls, "ls": ls, "e": e,
                "z": (x - mu) * e, "ld": ls.sum(1)}


def recurrence_grads(flow, x, gz, gld):
    """The reverse sweep, literally, in the dtype of `flow`: no autograd anywhere. Returns
    (gx, [one gradient per parameter, in list(flow.parameters()) order])."""
    hidden, out = flow.conditioner.plan()
    act = activation_name(flow)
    dt_ = out.weight.dtype
    ca, cl = flow.clamp_alpha, flow.clamp_log_scale
    x, gz, gld = x.to(dt_), gz.to(dt_), gld.to(dt_)
    with torch.no_grad():
        t = trace(flow, x)
        o, z, ld, e, nls, alpha = t["o"], t["z"], t["ld"], t["e"], t["nls"], t["alpha"]
        zero = torch.zeros_like(gz)
        gl = torch.where(torch.isfinite(ld) & (ld >= -100) & (ld <= 100), gld, torch.zeros_like(gld))
        g = torch.where(torch.isfinite(z), gz, zero)
        mu_bar = -g * e
        ls_bar = g * z + gl[:, None]
        both = (nls >= -cl) & (nls <= cl) & (alpha >= -ca) & (alpha <= ca)
        alpha_bar = torch.where(both, -ls_bar, zero)
        o_bar = torch.cat([mu_bar, alpha_bar], dim=1)
        o_bar = torch.where((o >= -2) & (o <= 2), o_bar, torch.zeros_like(o_bar))
        grads = {id(out.weight): out.mask * (o_bar.t() @ t["h"]), id(out.bias): o_bar.sum(0)}
        gh = o_bar @ (out.weight * out.mask)
        for (lin, ln, _, res), (hin, xh, rstd, p) in reversed(list(zip(hidden, t["layers"]))):
            gp = gh * _dact(act, p)
            if ln is not None:
                grads[id(ln.weight)] = (gp * xh).sum(0)
                grads[id(ln.bias)] = gp.sum(0)
                gg = gp * ln.weight
                a = rstd * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
            else:
                a = gp
            grads[id(lin.weight)] = lin.mask * (a.t() @ hin)
            grads[id(lin.bias)] = a.sum(0)
            in_bar = a @ (lin.weight * lin.mask)
            gh = in_bar + gh if res else in_bar
        gx = g * e + gh
    return gx, [grads[id(p)] for p in flow.parameters()]


def away_from_kinks(flow, x, tol=1e-4):
    """The rows of x whose float64 conditioner stays `tol` away from every point where the gradient
    jumps: a relu or leaky_relu pre-activation at 0, an output at +-2, alpha at +-clamp_alpha, -alpha at
    +-clamp_log_scale (a bound above 2 is never met: |alpha| <= 2 after the output clamp). fp32 may
    land on the other side of such a point. At most 5 % of the rows may go."""
    f64 = as_double(flow)
    t = trace(f64, x.double())
    near = ((t["o"].abs() - 2).abs() < tol).any(1)
    near |= ((t["alpha"].abs() - flow.clamp_alpha).abs() < tol).any(1)
    near |= ((t["nls"].abs() - flow.clamp_log_scale).abs() < tol).any(1)
    if activation_name(flow) in ("relu", "leaky_relu"):
        for _, _, _, p in t["layers"]:
            near |= (p.abs() < tol).any(1)
    dropped = int(near.sum())
    assert dropped <= 0.05 * x.shape[0], f"{dropped} of {x.shape[0]} rows lie within {tol} of a kink"
    return x[~near]
