"""Shared weights, inputs and references of the ContinuousFlow tests (test_cnf_cpu.py,
test_gpu_cnf.py)."""
import functools

import torch

import nfs_amd


def make_flow(d, H, final_scale=3.0, seed=0):
    """ContinuousFlow(d, H) with every layer redrawn: weights from the reference initialisation's
    distribution (Xavier normal) — the final one too, which is zero at init and would make every
    test vacuous — scaled by `final_scale` there; biases 0.1 N(0, 1). Fixed seed."""
    flow = nfs_amd.ContinuousFlow(d, H)
    g = torch.Generator().manual_seed(4100 + 131 * seed + 17 * d + H)
    with torch.no_grad():
        for lin in flow.ode_func.linears():
            fan_out, fan_in = lin.weight.shape
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * (2.0 / (fan_in + fan_out)) ** 0.5)
            lin.bias.copy_(0.1 * torch.randn(lin.bias.shape, generator=g))
        flow.ode_func.net[4].weight.mul_(final_scale)
    return flow.eval()


def make_inputs(B, d, seed=0):
    """Rows from N(0, 1.5^2)."""
    g = torch.Generator().manual_seed(977 + seed)
    return 1.5 * torch.randn(B, d, generator=g)


def as_double(flow):
    """A float64 copy of `flow` (same weights)."""
    f64 = nfs_amd.ContinuousFlow(flow.dim, flow.hidden_dim).double()
    f64.load_state_dict({k: v.double() for k, v in flow.state_dict().items()})
    f64.step_size = flow.step_size
    return f64.eval()


def composite(flow, x, direction, times=None):
    """The torch composite on the CPU in x's dtype: (y, ld)."""
    with torch.no_grad():
        if times is not None:
            return flow.forward(x, times) if direction > 0 else flow.inverse(x, times)
        return flow.forward(x) if direction > 0 else flow.inverse(x)


B_MAX = 4099


@functools.lru_cache(maxsize=None)
def parity_case(d, H, direction, B_max=B_MAX):
    """(flow, x [B_max, d], (y32, ld32), (y64, ld64)): the shared-weights flow, its inputs, and
    the fp32 and float64 CPU composites in `direction`. Rows are independent, so a test at a
    smaller batch slices these; computed once per session and never modified.
    (test_gpu_tile_instantiations.py draws 33 rows per case: `B_max=33`.)"""
    flow = make_flow(d, H)
    x = make_inputs(B_max, d, seed=3 + (direction > 0))
    c32 = composite(flow, x, direction)
    c64 = composite(as_double(flow), x.double(), direction)
    return flow, x, c32, c64
