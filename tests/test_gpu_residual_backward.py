"""GPU: ResidualFlow's fused backward (csrc/nfx_residual_bwd*.hip, ResidualFlow.fused_backward)
against float64 autograd of the converged CPU composite, by the project's criterion for these
gradients (residual_backward_cases.gclose). The layer under test keeps its own max_iter = 100 and
tol = 1e-6."""

import pytest
import torch

import nfs_amd
from nfs_amd import _lib
from residual_backward_cases import (NAMES, autograd_grads, converged, cotangents, gclose, preactivations,
                                     recurrence_grads, references)
from residual_cases import ACTIVATIONS, make_flow, make_inputs, sigmas

pytestmark = pytest.mark.gpu

BWD_KERNELS = ("residual_bwd_kernel", "res_bwd_reduce_kernel", "res_bwd_finish_kernel")


def _fused(flow, device):
    flow = flow.to(device)
    flow.fused_backward = True  # on the instance: the class default stays off
    return flow


def _twin(flow_cpu, device):
    """A copy of `flow_cpu` on the device with the fused backward on."""
    block = flow_cpu.residual_block
    act = {"ReLU": "relu", "ELU": "elu", "LeakyReLU": "leaky_relu", "Tanh": "tanh"}[type(block.activation).__name__]
    gpu = nfs_amd.ResidualFlow(flow_cpu.dim, flow_cpu.hidden_dim, lipschitz_constant=flow_cpu.lipschitz_constant,
                               activation=act, max_iter=flow_cpu.max_iter, tol=flow_cpu.tol,
                               neumann_terms=flow_cpu.neumann_terms)
    gpu.load_state_dict(flow_cpu.state_dict())
    return _fused(gpu.train(flow_cpu.training), device)


def _grads(flow, x, direction, gy, gld):
    """[gx, gW1, gb1, gW2, gb2, gW3, gb3] through the public forward/inverse and autograd."""
    flow.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    y, ld = flow.forward(xr) if direction > 0 else flow.inverse(xr)
    torch.autograd.backward([y, ld], [gy, gld])
    return [xr.grad] + [p.grad for p in flow.parameters()]


def _fused_grads(gpu, x, direction, gy, gld):
    """_grads on the fused route, asserting that it ran in HIP only and ended in a backward kernel."""
    launched, fused_backward = [], gpu._hip_backward

    def spy(*args, **kwargs):  # (nfx_last_kernel is per thread, and autograd runs backward on its own)
        out = fused_backward(*args, **kwargs)
        launched.append(_lib.last_kernel())
        return out
    gpu._hip_backward = spy
    try:
        nfs_amd.reset_stats()
        dev = next(gpu.parameters()).device
        got = _grads(gpu, x.to(dev), direction, gy.to(dev), gld.to(dev))
        torch.cuda.synchronize()
    finally:
        del gpu._hip_backward
    assert nfs_amd.STATS["torch"] == 0 and nfs_amd.STATS["hip"] == 2, nfs_amd.STATS
    assert len(launched) == 1 and launched[0] in BWD_KERNELS, launched
    return got


def _assert_masks_are_stable(flow_cpu, x, direction):
    """relu / leaky_relu: no float64 pre-activation at the converged z within 1e-5 of zero, so no
    derivative mask differs between fp32 and float64."""
    if type(flow_cpu.residual_block.activation).__name__ not in ("ReLU", "LeakyReLU"):
        return
    conv = converged(flow_cpu, torch.float64, x)
    with torch.no_grad():
        z = x.double() if direction > 0 else conv._torch_call(x.double(), -1)[0]
    a1, a2 = preactivations(conv, z)
    assert float(a1.abs().min()) > 1e-5 and float(a2.abs().min()) > 1e-5, "choose another seed"


def _check(cuda_device, flow_cpu, x, direction, seed, what):
    _assert_masks_are_stable(flow_cpu, x, direction)
    gy, gld = cotangents(x.shape[0], x.shape[1], seed=seed)
    g64, g32 = references(flow_cpu, x, direction, gy, gld)
    got = _fused_grads(_twin(flow_cpu, cuda_device), x, direction, gy, gld)
    for name, g, a, b in zip(NAMES, got, g64, g32):
        assert g is not None and g.shape == a.shape and float(a.abs().max()) > 0, name
        gclose(g, a, f"{what} {name}", b)
    return got


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("d,H,B", [(2, 64, 33), (1, 7, 1), (5, 20, 70), (8, 64, 40), (3, 33, 45)])
def test_parity_against_float64_autograd(cuda_device, d, H, B, direction):
    """gx and the six parameter gradients: one row, a partial second tile, three tiles, both padded
    widths, padding 7 -> 32 and 33 -> 64, the smallest and the largest dim."""
    _check(cuda_device, make_flow(d, H, "tanh"), make_inputs(B, d, seed=41), direction, d + B,
           f"d={d} H={H} B={B} dir={direction}")


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("d,H,B", [(2, 64, 33), (8, 64, 40)])
@pytest.mark.parametrize("act", ACTIVATIONS)
def test_parity_for_every_activation(cuda_device, act, d, H, B, direction):
    _check(cuda_device, make_flow(d, H, act, seed=2), make_inputs(B, d, seed=43), direction, 3 + d,
           f"{act} d={d} dir={direction}")


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("nterms", [1, 3, 5])
@pytest.mark.parametrize("lipschitz", [0.9, 1.8])
def test_parity_over_lipschitz_constant_and_neumann_terms(cuda_device, lipschitz, nterms, direction):
    _check(cuda_device, make_flow(3, 33, "elu", lipschitz, seed=4, neumann_terms=nterms), make_inputs(45, 3, seed=47),
           direction, nterms, f"L={lipschitz} n={nterms} dir={direction}")


@pytest.mark.parametrize("direction", [1, -1])
def test_parity_when_no_layer_is_normalised(cuda_device, direction):
    flow = make_flow(2, 64, "tanh", weight_scale=0.1)
    assert not any(s > c for s, c in sigmas(flow))
    _check(cuda_device, flow, make_inputs(33, 2, seed=51), direction, 5, f"plain dir={direction}")


@pytest.mark.parametrize("direction", [1, -1])
def test_parity_when_only_one_layer_is_normalised(cuda_device, direction):
    flow = make_flow(2, 64, "tanh", weight_scale=0.1)
    with torch.no_grad():
        flow.residual_block.layer2.module.weight.mul_(30.0)
    assert [s > c for s, c in sigmas(flow)] == [False, True, False]
    _check(cuda_device, flow, make_inputs(33, 2, seed=53), direction, 6, f"mixed dir={direction}")


@pytest.mark.parametrize("direction", [1, -1])
def test_no_neumann_terms(cuda_device, direction):
    """neumann_terms = 0: ld is identically 0, the gradients are those of gy alone, and gld changes
    nothing, bit for bit."""
    flow = make_flow(2, 64, "tanh", neumann_terms=0)
    x = make_inputs(40, 2, seed=57)
    gy, gld = cotangents(40, 2, seed=9)
    gx64, gp64 = autograd_grads(converged(flow, torch.float64, x), x, direction, gy, None)
    gx32, gp32 = autograd_grads(converged(flow, torch.float32, x), x, direction, gy, None)
    gpu = _twin(flow, cuda_device)
    with torch.no_grad():
        _, ld = gpu.forward(x.to(cuda_device)) if direction > 0 else gpu.inverse(x.to(cuda_device))
    assert float(ld.abs().max()) == 0.0
    got = _fused_grads(gpu, x, direction, gy, gld)
    for name, g, a, b in zip(NAMES, got, [gx64] + gp64, [gx32] + gp32):
        assert float(a.abs().max()) > 0, name
        gclose(g, a, f"n=0 dir={direction} {name}", b)
    again = _fused_grads(gpu, x, direction, gy, 7.0 * gld + 1.0)
    for name, u, v in zip(NAMES, got, again):
        assert torch.equal(u, v), name


def test_many_tiles_per_wave_and_the_cross_wave_reduction(cuda_device):
    """A batch beyond the slot cap (four-wave workgroups, several tiles per wave, a partial last
    tile, every slot reduced) and one between the two launch shapes. The oracle is the recurrence in
    float64 under no_grad, which test_residual_backward_cpu.py pins to autograd: an unrolled float64
    autograd graph does not fit at this batch. ref32 is the same recurrence in fp32."""
    d, H = 2, 32
    L = _lib.lib()
    cap = L.nfx_residual_backward_slots(1 << 40, d, H)
    B = 32 * (2 * cap + 5) + 7
    assert L.nfx_residual_backward_block_threads(B, d, H) == 256 and L.nfx_residual_backward_slots(B, d, H) == cap
    assert (B + 31) // 32 > 2 * cap
    B2 = 32 * (cap // 2) + 3
    assert L.nfx_residual_backward_block_threads(B2, d, H) == 256
    assert cap // 2 < L.nfx_residual_backward_slots(B2, d, H) <= cap
    flow = make_flow(d, H, "tanh", 0.9)
    gpu = _twin(flow, cuda_device)
    for batch, seed, direction in ((B, 61, -1), (B, 61, 1), (B2, 63, -1)):
        x = make_inputs(batch, d, seed=seed)
        gy, gld = cotangents(batch, d, seed=seed)
        probe = x[:512]
        gx64, gp64 = recurrence_grads(converged(flow, torch.float64, probe), x, direction, gy, gld)
        gx32, gp32 = recurrence_grads(converged(flow, torch.float32, probe), x, direction, gy, gld)
        got = _fused_grads(gpu, x, direction, gy, gld)
        for name, g, a, b in zip(NAMES, got, [gx64] + gp64, [gx32] + gp32):
            assert float(a.abs().max()) > 0, name
            gclose(g, a, f"B={batch} dir={direction} {name}", b)


def test_outputs_on_the_fused_route_are_the_plain_kernels(cuda_device):
    """y and ld bit-equal to _hip_call's in both directions, and the forward part of the backward
    image bit-equal to the forward pack."""
    for d, H in [(2, 64), (5, 20)]:
        gpu = _twin(make_flow(d, H, "elu"), cuda_device)
        x = make_inputs(77, d, seed=59).to(cuda_device)  # a partial third tile
        for direction in (1, -1):
            with torch.no_grad():
                y, ld = gpu._hip_call(x, direction)
            xr = x.clone().requires_grad_(True)
            nfs_amd.reset_stats()
            ys, lds = gpu.forward(xr) if direction > 0 else gpu.inverse(xr)
            assert ys.grad_fn is not None and type(ys.grad_fn).__name__.startswith("_ResidualFunction")
            assert torch.equal(y, ys) and torch.equal(ld, lds)
        fwd = gpu._build_pack(x.device)
        bwd = gpu._build_backward_pack(x.device)
        assert bwd.numel() == _lib.lib().nfx_residual_backward_packed_floats(d, H) > fwd.numel()
        assert torch.equal(bwd[:fwd.numel()].view(torch.int32), fwd.view(torch.int32))


@pytest.mark.parametrize("direction", [1, -1])
def test_dead_rows(cuda_device, direction):
    """A NaN row and an Inf row add nothing: finite gradients everywhere, gx = 0 on those rows,
    parameter gradients bit-equal to the batch with those rows' inputs and cotangents zeroed."""
    gpu = _twin(make_flow(2, 64, "tanh"), cuda_device)
    x = make_inputs(40, 2, seed=61)
    gy, gld = cotangents(40, 2, seed=13)
    bad = x.clone()
    bad[7, 1] = float("nan")
    bad[35] = float("inf")
    zx, zgy, zgld = x.clone(), gy.clone(), gld.clone()
    zx[[7, 35]] = 0.0
    zgy[[7, 35]] = 0.0
    zgld[[7, 35]] = 0.0
    got = _fused_grads(gpu, bad, direction, gy, gld)
    ref = _fused_grads(gpu, zx, direction, zgy, zgld)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert float(got[0][[7, 35]].abs().max()) == 0.0
    live = [i for i in range(40) if i not in (7, 35)]
    assert torch.equal(got[0][live], ref[0][live])
    for name, a, b in zip(NAMES[1:], got[1:], ref[1:]):
        assert torch.equal(a, b), name
        assert float(a.abs().max()) > 0, name


def test_determinism(cuda_device):
    gpu = _twin(make_flow(5, 64, "tanh"), cuda_device)
    x = make_inputs(300, 5, seed=67)
    gy, gld = cotangents(300, 5, seed=17)
    for direction in (1, -1):
        a = [g.clone() for g in _fused_grads(gpu, x, direction, gy, gld)]
        b = _fused_grads(gpu, x, direction, gy, gld)
        for name, u, v in zip(NAMES, a, b):
            assert torch.equal(u, v), (name, direction)


def test_flag_and_family(cuda_device):
    """The default keeps the composite route; hidden_dim = 128 keeps it with the flag on; train mode
    keeps it, with u and v advancing as before; frozen parameters get no gradient on the fused route."""
    assert nfs_amd.ResidualFlow.fused_backward is False
    x = make_inputs(20, 2, seed=73).to(cuda_device)
    gy, gld = (t.to(cuda_device) for t in cotangents(20, 2, seed=23))
    flow = make_flow(2, 32, "tanh").to(cuda_device)
    nfs_amd.reset_stats()
    plain = _grads(flow, x, -1, gy, gld)
    assert nfs_amd.STATS["torch"] == 1, nfs_amd.STATS
    wide = _fused(make_flow(2, 128, "tanh"), cuda_device)
    nfs_amd.reset_stats()
    _grads(wide, x, -1, gy, gld)
    assert nfs_amd.STATS["torch"] == 1, nfs_amd.STATS
    # train mode: the composite, buffer updates included, whatever the flag says
    off, on = make_flow(2, 32, "tanh").to(cuda_device).train(), _fused(make_flow(2, 32, "tanh"), cuda_device).train()
    nfs_amd.reset_stats()
    g_off = _grads(off, x, 1, gy, gld)
    g_on = _grads(on, x, 1, gy, gld)
    assert nfs_amd.STATS == {"hip": 0, "torch": 2}, nfs_amd.STATS
    start = make_flow(2, 32, "tanh")
    for l_off, l_on, l0 in zip(off.residual_block.layers(), on.residual_block.layers(), start.residual_block.layers()):
        assert torch.equal(l_off.u, l_on.u) and torch.equal(l_off.v, l_on.v)
        assert not torch.equal(l_on.u.cpu(), l0.u)
    for a, b in zip(g_off, g_on):
        assert torch.equal(a, b)
    fused = _fused(make_flow(2, 32, "tanh"), cuda_device)
    fused.residual_block.layer2.module.weight.requires_grad_(False)
    fused.residual_block.layer3.module.bias.requires_grad_(False)
    nfs_amd.reset_stats()
    got = _grads(fused, x, -1, gy, gld)
    assert nfs_amd.STATS["torch"] == 0, nfs_amd.STATS
    assert got[3] is None and got[6] is None
    assert all(got[i] is not None and got[i].shape == plain[i].shape for i in (0, 1, 2, 4, 5))


def _nll_grads(model, x):
    model.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    loss = -model.log_prob(xr).mean()
    loss.backward()
    return loss.detach(), xr.grad, [p.grad for p in model.parameters()]


def test_nll_step_of_three_layers(cuda_device):
    """One backward of the NLL of three ResidualFlow(2, 64) layers in eval mode, each on its own
    fused backward: no composite call at all. The oracle's layers are converged on the inputs they
    meet in the chain."""
    B = 600
    x = make_inputs(B, 2, seed=23)
    layers = [make_flow(2, 64, "tanh", seed=s) for s in (1, 2, 3)]

    def oracle(dtype):
        conv, cur = [], x
        for f in reversed(layers):  # log_prob runs the inverses last layer first
            c = converged(f, dtype, cur)
            with torch.no_grad():
                cur = converged(f, torch.float64, cur)._torch_call(cur.double(), -1)[0].float()
            conv.append(c)
        model = nfs_amd.NormalizingFlowModel(list(reversed(conv))).eval()
        return _nll_grads(model, x.to(dtype))
    ref64, ref32 = oracle(torch.float64), oracle(torch.float32)
    model = nfs_amd.NormalizingFlowModel([_twin(f, cuda_device) for f in layers]).to(cuda_device).eval()
    assert all(f.fused_backward for f in model.flows)
    nfs_amd.reset_stats()
    loss, gx, gp = _nll_grads(model, x.to(cuda_device))
    torch.cuda.synchronize()
    assert nfs_amd.STATS["torch"] == 0 and nfs_amd.STATS["hip"] >= 6, nfs_amd.STATS
    gclose(loss, ref64[0], "loss", ref32[0])
    gclose(gx, ref64[1], "dL/dx", ref32[1])
    names = [n for n, _ in model.named_parameters()]
    assert len(names) == 18
    for n, g, g64, g32 in zip(names, gp, ref64[2], ref32[2]):
        assert g is not None and float(g64.abs().max()) > 0, n
        gclose(g, g64, n, g32)
