"""Shared weights, inputs and references of the NeuralAutoregressiveFlow tests (test_naf_cpu.py,
test_gpu_naf.py)."""
import functools

import torch

import nfs_amd

ACTIVATIONS = ("relu", "elu", "leaky_relu", "gelu")


def redraw(flow, seed):
    """Redraw every layer of a NeuralAutoregressiveFlow-shaped module in place (this project's or the
    reference's: same submodule names): Xavier-normal weights at gain 2, biases 0.2 N(0, 1), LayerNorm
    gamma 1 + 0.2 N(0, 1) and beta 0.2 N(0, 1). At this scale 7 % to 28 % of the conditioner outputs
    sit on the +-2 clamp; the constructor's own init never reaches it."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in flow.conditioner.network.modules():
            if isinstance(m, torch.nn.Linear):
                fan_out, fan_in = m.weight.shape
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 2.0 * (2.0 / (fan_in + fan_out)) ** 0.5)
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
    return flow


def make_flow(d, hidden, act="relu", ln=True, res=True, seed=0, dropout=0.0, **kw):
    """NeuralAutoregressiveFlow(d, hidden) in eval mode with every layer redrawn. Fixed seed."""
    flow = nfs_amd.NeuralAutoregressiveFlow(d, list(hidden), activation=act, use_layer_norm=ln, use_residual=res,
                                            dropout=dropout, **kw)
    return redraw(flow, 7300 + 131 * seed + 17 * d + sum(hidden)).eval()


def make_inputs(B, d, seed=0):
    """Rows from N(0, 1.5^2)."""
    g = torch.Generator().manual_seed(2203 + seed)
    return 1.5 * torch.randn(B, d, generator=g)


def activation_name(flow):
    return {"ReLU": "relu", "ELU": "elu", "LeakyReLU": "leaky_relu", "GELU": "gelu"}[
        type(flow.conditioner.activation).__name__]


def as_double(flow):
    """A float64 copy of `flow` (same weights, buffers, settings and mode)."""
    c = flow.conditioner
    f64 = nfs_amd.NeuralAutoregressiveFlow(flow.dim, list(c.hidden_dims), activation=activation_name(flow),
                                           use_layer_norm=c.use_layer_norm, use_residual=c.use_residual,
                                           dropout=c.dropout, clamp_alpha=flow.clamp_alpha,
                                           clamp_log_scale=flow.clamp_log_scale).double()
    f64.load_state_dict({k: v.double() for k, v in flow.state_dict().items()})
    return f64.train(flow.training)


def composite(flow, x, direction):
    """The torch composite on the CPU in x's dtype: (y, ld)."""
    with torch.no_grad():
        return flow.forward(x) if direction > 0 else flow.inverse(x)


B_MAX = 4099


def hardest_row(c32, c64):
    """The row on which the reference's own fp32 arithmetic is least accurate, in x / z and in the
    log-det at once: the largest min(row's mean |y32 - y64| / its mean over all rows, |ld32 - ld64| / its
    mean over all rows). It is chosen from the CPU results alone, before any kernel runs.

    Only the one-row parity batch uses it. conftest.assert_fp32_parity bounds the kernel's MEAN error
    by 1.5 times the reference's over the same rows (+ 1e-7); over one row that compares two single
    rounding errors, and the reference's can lie far below the half ulp of the log-det (1.2e-7 at
    |ld| = 2, 4.8e-7 at |ld| = 8) that even a correctly rounded result may be off by. On this row the
    reference's error is several times its mean, so the ratio says something about the kernel."""
    ey = (c32[0].double() - c64[0]).abs().mean(dim=1)
    el = (c32[1].double() - c64[1]).abs()
    score = torch.minimum(ey / ey.mean().clamp_min(1e-30), el / el.mean().clamp_min(1e-30))
    return int(score.argmax())


@functools.lru_cache(maxsize=None)
def parity_case(d, hidden, act, ln, res, direction, B_max=B_MAX):
    """(flow, x [B_max, d], (y32, ld32), (y64, ld64)): the shared-weights flow, its inputs as drawn,
    and the fp32 and float64 CPU composites in `direction`. Rows are independent, so a test at a
    smaller batch slices these; computed once per session and never modified."""
    flow = make_flow(d, hidden, act, ln, res)
    x = make_inputs(B_max, d, seed=3 + (direction > 0))
    c32 = composite(flow, x, direction)
    c64 = composite(as_double(flow), x.double(), direction)
    return flow, x, c32, c64
