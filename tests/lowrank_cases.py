"""Shared parameters, inputs and references of the Planar / Radial / Sylvester tests
(test_lowrank_cpu.py, test_gpu_lowrank.py, golden/make_golden_lowrank.py).

The constructors' own std-0.1 initialisation is nearly the identity and would test nothing, so
`redraw` puts each layer's contraction bound at a chosen value in [0.3, 0.7]:
  Planar     |u.w| (u the constrained one)     Radial   |beta| / alpha     Sylvester   ||R||_2^2
and `contraction_bound` reads it back in float64. `redraw` works on this project's modules and on
the reference's (same attribute names)."""
import copy
import functools
import math

import torch

import nfs_amd

KINDS = ("planar", "radial", "sylvester")
LO, HI = 0.3, 0.7


def kind_of(flow):
    return type(flow).__name__.replace("Flow", "").lower()


def contraction_bound(flow):
    """The layer's contraction bound, in float64."""
    sd = {k: v.detach().double().cpu() for k, v in flow.state_dict().items()}
    kind = kind_of(flow)
    if kind == "planar":
        w, u_hat = sd["w"], sd["u_hat"]
        wtu = torch.dot(w, u_hat)
        u = u_hat + (-1 + torch.log1p(torch.exp(wtu)) - wtu) * w / (torch.sum(w ** 2) + 1e-8)
        return abs(float(torch.dot(u, w)))
    if kind == "radial":
        alpha = torch.nn.functional.softplus(sd["alpha_hat"])
        beta = -alpha + torch.nn.functional.softplus(sd["beta_hat"])
        return abs(float(beta)) / float(alpha)
    return float(torch.linalg.matrix_norm(sd["R"], 2)) ** 2


def redraw(flow, seed, bound=0.6):
    """Redraw every parameter in place so that contraction_bound(flow) == `bound` (to rounding); the
    sign of u.w and of beta alternates with the seed. Asserts the bound in float64."""
    assert LO <= bound <= HI
    g = torch.Generator().manual_seed(seed)
    kind, d = kind_of(flow), flow.dim
    sign = 1.0 if seed % 2 == 0 else -1.0
    with torch.no_grad():
        if kind == "planar":
            w = torch.randn(d, generator=g, dtype=torch.float64) / math.sqrt(d)
            if float(w.norm()) < 0.3:
                w = w * (0.3 / float(w.norm()))
            noise = torch.randn(d, generator=g, dtype=torch.float64) / math.sqrt(d)
            noise = noise - w * torch.dot(noise, w) / torch.dot(w, w)
            # u.w = m(w.u_hat) = -1 + log1p(exp(w.u_hat)), so w.u_hat = log(exp(1 + t) - 1)
            s = math.log(math.exp(1.0 + sign * bound) - 1.0)
            flow.w.copy_(w.float())
            flow.u_hat.copy_((w * s / torch.dot(w, w) + 0.3 * noise).float())
            flow.b.copy_(0.3 * torch.randn(1, generator=g))
        elif kind == "radial":
            alpha = 0.5 + float(torch.rand(1, generator=g))
            beta = sign * bound * alpha
            flow.z0.copy_(0.5 * torch.randn(d, generator=g))
            flow.alpha_hat.fill_(math.log(math.expm1(alpha)))
            flow.beta_hat.fill_(math.log(math.expm1(alpha + beta)))
        else:
            for r in flow.Q.reflections:
                r.v.copy_(torch.randn(d, generator=g))
            R = torch.randn(flow.R.shape, generator=g, dtype=torch.float64)
            R = R * math.sqrt(bound) / float(torch.linalg.matrix_norm(R, 2))
            flow.R.copy_(R.float())
            flow.b.copy_(0.3 * torch.randn(flow.b.shape, generator=g))
    got = contraction_bound(flow)
    assert LO <= got <= HI and abs(got - bound) < 1e-3, (kind, d, got, bound)
    return flow


def construct(kind, dim, num_householder=8, num_transforms=None, module=nfs_amd):
    if kind == "planar":
        return module.PlanarFlow(dim)
    if kind == "radial":
        return module.RadialFlow(dim)
    return module.SylvesterFlow(dim, num_householder=num_householder, num_transforms=num_transforms)


def make_layer(kind, dim, seed=0, bound=0.6, **kw):
    """An eval-mode layer with redrawn parameters. Fixed seed."""
    flow = construct(kind, dim, **kw)
    return redraw(flow, 7300 + 2 * (97 * KINDS.index(kind) + 13 * dim) + seed, bound).eval()


def make_inputs(B, d, seed=0):
    """Rows from N(0, 1.5^2)."""
    g = torch.Generator().manual_seed(2311 + seed)
    return 1.5 * torch.randn(B, d, generator=g)


def as_double(flow):
    """A float64 copy of a layer or of a container of layers (same parameters and settings)."""
    return copy.deepcopy(flow).double()


def composite(flow, x, direction):
    """The torch composite on the CPU in x's dtype: (y, ld)."""
    with torch.no_grad():
        return flow.forward(x) if direction > 0 else flow.inverse(x)


B_MAX = 257


@functools.lru_cache(maxsize=None)
def parity_case(kind, dim, num_householder, num_transforms, direction):
    """(flow, x [B_MAX, dim], (y32, ld32), (y64, ld64)): the layer, its inputs and the fp32 and
    float64 CPU composites in `direction`. Rows are independent (the stopping rule is per sample),
    so a test at a smaller batch slices these; computed once per session and never modified."""
    flow = make_layer(kind, dim, num_householder=num_householder, num_transforms=num_transforms)
    x = make_inputs(B_MAX, dim, seed=3 + (direction > 0))
    c32 = composite(flow, x, direction)
    c64 = composite(as_double(flow), x.double(), direction)
    return flow, x, c32, c64


def mixed_stack(dim, seed=0):
    """Planar, Radial, Sylvester, Planar, Radial at one dim."""
    kinds = ("planar", "radial", "sylvester", "planar", "radial")
    return [make_layer(k, dim, seed=seed + 2 * i + (i % 2), num_householder=3, num_transforms=min(dim, 4))
            for i, k in enumerate(kinds)]
