"""GPU: ResidualFlow — forward, or the whole fixed-point inverse, with the full Jacobian and the
Neumann log-det in one gfx950 kernel (csrc/nfx_residual*.hip) against the torch composite that
test_residual_cpu.py pins to the reference."""
import copy

import numpy as np
import pytest
import torch

from conftest import assert_fp32_parity
import nfs_amd
from nfs_amd import _lib
from nfs_amd.flows import flow as flow_mod
from residual_cases import as_double, composite, make_flow, make_inputs, parity_case, sigmas

pytestmark = pytest.mark.gpu

# (d, H, activation, lipschitz_constant): every activation at every padded width (32, 64, 128), both
# Lipschitz settings at every shape
CASES = [(1, 8, "relu", 0.9), (1, 8, "elu", 1.8), (3, 16, "leaky_relu", 0.9), (3, 16, "tanh", 1.8),
         (2, 64, "relu", 1.8), (2, 64, "tanh", 0.9), (4, 48, "elu", 0.9), (4, 48, "leaky_relu", 1.8),
         (8, 128, "relu", 0.9), (8, 128, "elu", 1.8), (8, 128, "leaky_relu", 0.9), (8, 128, "tanh", 1.8)]


def _gpu(flow, dev):
    return copy.deepcopy(flow).to(dev)


def _call(flow, x, direction):
    with torch.no_grad():
        return flow.forward(x) if direction > 0 else flow.inverse(x)


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("B", [1, 31, 33, 4099])
@pytest.mark.parametrize("d,H,act,lipschitz", CASES)
def test_parity_against_float64(cuda_device, d, H, act, lipschitz, B, direction):
    """Below, across and beyond one 32-row tile and an odd tail, both directions: the kernel against
    the fp32 CPU composite and the float64 composite with conftest's fixed caps, the log-det (small
    here) also directly against float64, and the proof that the fused kernel ran."""
    flow, x, (y32, ld32), (y64, ld64) = parity_case(d, H, act, lipschitz, direction)
    assert all(abs(s - c) > 1e-3 * c for s, c in sigmas(flow))  # no rounding flips a layer's regime
    gpu = _gpu(flow, cuda_device)
    nfs_amd.reset_stats()
    y, ld = _call(gpu, x[:B].to(cuda_device), direction)
    torch.cuda.synchronize()
    assert nfs_amd.STATS["torch"] == 0 and nfs_amd.STATS["hip"] > 0, nfs_amd.STATS
    assert _lib.last_kernel() == "residual_flow_kernel"
    assert y.shape == (B, d) and ld.shape == (B,)
    what = f"residual d={d} H={H} {act} L={lipschitz} B={B} dir={direction}"
    assert_fp32_parity(y.cpu().numpy(), y32[:B].numpy(), y64[:B].numpy(), what=what + " y", kind="y")
    assert_fp32_parity(ld.cpu().numpy(), ld32[:B].numpy(), ld64[:B].numpy(), what=what + " ld", kind="ld")
    e_gpu = float((ld.cpu().double() - ld64[:B]).abs().max())
    e_cpu = float((ld32[:B].double() - ld64[:B]).abs().max())
    print(f"[{what}] log-det: gpu {e_gpu:.3e} cpu fp32 {e_cpu:.3e} of max {float(ld64[:B].abs().max()):.3e}")
    assert e_gpu <= 4 * e_cpu + 1e-6


def _against_composite(flow, x, direction, dev, what):
    y32, ld32 = composite(flow, x, direction)
    y64, ld64 = composite(as_double(flow), x.double(), direction)
    nfs_amd.reset_stats()
    y, ld = _call(_gpu(flow, dev), x.to(dev), direction)
    assert nfs_amd.STATS == {"hip": 1, "torch": 0}
    assert_fp32_parity(y.cpu().numpy(), y32.numpy(), y64.numpy(), what=what + " y", kind="y")
    assert float((ld.cpu().double() - ld64).abs().max()) <= 4 * float((ld32.double() - ld64).abs().max()) + 1e-6, what
    return y, ld, y64, ld64


def test_runtime_arguments(cuda_device):
    """max_iter, neumann_terms and tol are read at every call."""
    dev = cuda_device
    x = make_inputs(200, 2, seed=31)
    full = composite(as_double(make_flow(2, 64, "tanh", 1.8)), x.double(), -1)[0]
    # max_iter = 3 at lipschitz 1.8: every row leaves through the not-converged exit
    flow = make_flow(2, 64, "tanh", 1.8, max_iter=3)
    z, _, z64, _ = _against_composite(flow, x, -1, dev, "residual max_iter=3")
    assert float((z64 - full).abs().max()) > 1e-5
    # max_iter = 0 returns x itself, with the log-det the forward has there, negated
    flow = _gpu(make_flow(2, 64, "tanh", 1.8, max_iter=0), dev)
    xg = x.to(dev)
    z0, l0 = _call(flow, xg, -1)
    _, lf = _call(flow, xg, 1)
    assert torch.equal(z0, xg) and torch.equal(l0, -lf) and float(lf.abs().max()) > 1e-3
    # neumann_terms
    for n in (0, 1, 5):
        flow = make_flow(2, 64, "tanh", 1.8, neumann_terms=n)
        for direction in (1, -1):
            _, ld, _, ld64 = _against_composite(flow, x, direction, dev, f"residual neumann_terms={n}")
            assert (float(ld.abs().max()) == 0.0) if n == 0 else (float(ld.abs().max()) > 1e-3)
    ld1 = composite(as_double(make_flow(2, 64, "tanh", 1.8, neumann_terms=1)), x.double(), 1)[1]
    ld5 = composite(as_double(make_flow(2, 64, "tanh", 1.8, neumann_terms=5)), x.double(), 1)[1]
    assert float((ld1 - ld5).abs().max()) > 1e-4
    # a loose tol stops earlier
    flow = make_flow(2, 64, "tanh", 1.8, tol=1e-3)
    z, _, z64, _ = _against_composite(flow, x, -1, dev, "residual tol=1e-3")
    assert float((z64 - full).abs().max()) > 1e-6


def test_rows_do_not_depend_on_their_batch(cuda_device):
    """Row i of a B = 4099 inverse equals, bit for bit, the same row run alone and in a batch of 33."""
    flow = _gpu(make_flow(3, 16, "tanh", 1.8), cuda_device)
    x = make_inputs(4099, 3, seed=37).to(cuda_device)
    z, ld = _call(flow, x, -1)
    for i in (0, 31, 32, 2048, 4098):
        z1, l1 = _call(flow, x[i:i + 1], -1)
        assert torch.equal(z1[0], z[i]) and torch.equal(l1[0], ld[i])
    for lo in (0, 1000, 4066):
        z33, l33 = _call(flow, x[lo:lo + 33], -1)
        assert torch.equal(z33, z[lo:lo + 33]) and torch.equal(l33, ld[lo:lo + 33])


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("d,H,act", [(2, 64, "relu"), (3, 128, "tanh")])
def test_odd_rows_in_a_tile(cuda_device, d, H, act, direction):
    """A NaN row and an Inf row inside 32-row tiles: the NaN row comes back NaN in x and z, and every
    other row is bit-identical to the run with ordinary values in their place (in the inverse the
    NaN row never converges and keeps its wave iterating to max_iter while the others stay frozen).
    The log-det of the two odd rows, and x / z of the Inf row, are not pinned: the reference has no
    guards for them."""
    flow = _gpu(make_flow(d, H, act), cuda_device)
    clean = make_inputs(70, d, seed=5)
    x = clean.clone()
    x[5] = float("nan")
    x[40] = float("inf")
    y, ld = (t.cpu() for t in _call(flow, x.to(cuda_device), direction))
    yc, ldc = (t.cpu() for t in _call(flow, clean.to(cuda_device), direction))
    assert bool(torch.isnan(y[5]).all())
    keep = [r for r in range(70) if r not in (5, 40)]
    assert torch.equal(y[keep], yc[keep]) and torch.equal(ld[keep], ldc[keep])
    assert bool(torch.isfinite(yc).all()) and bool(torch.isfinite(ldc).all())


@pytest.mark.parametrize("d,H,act", [(2, 64, "relu"), (2, 128, "elu"), (5, 20, "tanh")])
def test_independent_of_stale_lds(cuda_device, d, H, act):
    flow = _gpu(make_flow(d, H, act), cuda_device)
    x = make_inputs(77, d, seed=13).to(cuda_device)
    outs = {}
    for bits in (0, 0x7FC00000, 0xFFFFFFFF):
        res = []
        for direction in (1, -1):
            _lib.check(_lib.lib().nfx_debug_fill_lds(bits, _lib.stream_of(x)), "nfx_debug_fill_lds")
            res += list(_call(flow, x, direction))
        torch.cuda.synchronize()
        outs[bits] = [t.clone() for t in res]
    for bits in (0x7FC00000, 0xFFFFFFFF):
        for a, b in zip(outs[bits], outs[0]):
            assert torch.equal(a, b), hex(bits)
    assert bool(torch.isfinite(outs[0][0]).all())


@pytest.mark.parametrize("direction", [1, -1])
def test_strided_and_offset_input(cuda_device, direction):
    flow = _gpu(make_flow(3, 16, "elu"), cuda_device)
    base = make_inputs(90, 8, seed=41).to(cuda_device)
    view = base[:, 1:7:2]
    assert not view.is_contiguous() and view.storage_offset() == 1
    y, ld = _call(flow, view, direction)
    yd, ldd = _call(flow, view.contiguous(), direction)
    assert torch.equal(y, yd) and torch.equal(ld, ldd) and float(ld.abs().max()) > 0


def _chain_model():
    m0, m1 = torch.tensor([1.0, 0.0]), torch.tensor([0.0, 1.0])
    torch.manual_seed(5)
    c0, c1 = nfs_amd.CouplingLayer(2, 64, m0), nfs_amd.CouplingLayer(2, 64, m1)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in list(c0.parameters()) + list(c1.parameters()):
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    return nfs_amd.NormalizingFlowModel([c0, make_flow(2, 64, "tanh"), c1]).eval()


def test_chain_and_accumulate(cuda_device):
    """A ResidualFlow between two coupling layers: the model's chain (log-det accumulated in place by
    the kernels) equals the per-layer calls summed in the same fp32 order, bit for bit."""
    model = _chain_model().to(cuda_device)
    x = make_inputs(1000, 2, seed=9).to(cuda_device)
    nfs_amd.reset_stats()
    with torch.no_grad():
        z, ld = model.inverse(x)
        logp = model.log_prob(x)
        xf, ldf = model.forward(x)
        cur, tot = x, None
        for f in reversed(model.flows):
            cur, l = f.inverse(cur)
            tot = l if tot is None else tot + l
        fwd, totf = x, None
        for f in model.flows:
            fwd, l = f.forward(fwd)
            totf = l if totf is None else totf + l
        lp_ref, _ = nfs_amd.gauss_logprob(cur, tot)
    assert nfs_amd.STATS["torch"] == 0, nfs_amd.STATS
    assert torch.equal(z, cur) and torch.equal(ld, tot)
    assert torch.equal(xf, fwd) and torch.equal(ldf, totf)
    assert torch.equal(logp, lp_ref)
    assert float(ld.abs().max()) > 0.1


def test_sequential_flow_and_sampling_on_the_device(cuda_device):
    f0, f1 = _gpu(make_flow(2, 64, "relu"), cuda_device), _gpu(make_flow(2, 24, "elu", seed=1), cuda_device)
    x = make_inputs(100, 2, seed=29).to(cuda_device)
    nfs_amd.reset_stats()
    with torch.no_grad():
        z, ld = nfs_amd.SequentialFlow([f0, f1]).inverse(x)
        z1, l1 = f1.inverse(x)
        z0, l0 = f0.inverse(z1)
        model = nfs_amd.NormalizingFlowModel([f0, f1]).eval()
        model.seed_sampler(3)
        xs, lds, zs = model.sample_on_device(100, cuda_device)
        xf, ldf = model.forward(zs)
    assert nfs_amd.STATS["torch"] == 0, nfs_amd.STATS
    assert torch.equal(z, z0) and torch.equal(ld, (torch.zeros_like(l1) + l1) + l0)
    assert torch.equal(xs, xf) and torch.equal(lds, ldf)
    assert abs(float(zs.mean())) < 0.5 and 0.5 < float(zs.std()) < 1.5


def test_graph_capture(cuda_device):
    flow = _gpu(make_flow(2, 64, "tanh", 1.8), cuda_device)
    x = make_inputs(300, 2, seed=17).to(cuda_device)
    eager = [t.clone() for t in _call(flow, x, -1)]
    static_x = x.clone()
    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        _call(flow, static_x, -1)  # the packed image exists before the capture
    torch.cuda.current_stream(cuda_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = flow.inverse(static_x)
    for _ in range(2):
        out[0].zero_()
        out[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


def _close_to_composite(flow_cpu, y, ld, x, direction):
    y32, ld32 = composite(flow_cpu, x, direction)
    return float(((y.cpu() - y32).abs() / (1 + y32.abs())).max()) <= 1e-5 and float((ld.cpu() - ld32).abs().max()) <= 1e-5


def test_pack_cache_follows_the_weights(cuda_device):
    """An in-place weight update and a load_state_dict that moves a layer across sigma = c both
    reach the next call, and eval-mode calls leave `u` and `v` alone."""
    cpu = make_flow(2, 64, "tanh")
    gpu = _gpu(cpu, cuda_device)
    x = make_inputs(128, 2, seed=43)
    xg = x.to(cuda_device)
    before = {k: v.clone() for k, v in gpu.state_dict().items()}
    y0, l0 = _call(gpu, xg, 1)
    _call(gpu, xg, -1)
    assert all(torch.equal(before[k], v) for k, v in gpu.state_dict().items())
    assert _close_to_composite(cpu, y0, l0, x, 1)
    noise = 0.2 * torch.randn(cpu.residual_block.layer1.module.weight.shape, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        cpu.residual_block.layer1.module.weight.add_(noise)
        gpu.residual_block.layer1.module.weight.add_(noise.to(cuda_device))
    y1, l1 = _call(gpu, xg, 1)
    assert float((y1 - y0).abs().max()) > 1e-3 and _close_to_composite(cpu, y1, l1, x, 1)
    sd = {k: v.clone() for k, v in cpu.state_dict().items()}
    sd["residual_block.layer2.module.weight"] *= 0.05  # sigma of layer 2 drops below its c
    cpu.load_state_dict(sd)
    (s1, c1), (s2, c2), (s3, c3) = sigmas(cpu)
    assert s1 > c1 and s2 < c2 and s3 > c3
    gpu.load_state_dict(sd)
    y2, l2 = _call(gpu, xg, 1)
    assert float((y2 - y1).abs().max()) > 1e-4 and _close_to_composite(cpu, y2, l2, x, 1)


@pytest.mark.parametrize("d,H", [(9, 64), (2, 130)])
def test_outside_the_kernel_family(cuda_device, d, H, monkeypatch):
    cpu = make_flow(d, H, "elu")
    flow = _gpu(cpu, cuda_device)
    x = make_inputs(40, d, seed=19)
    with pytest.raises(NotImplementedError):
        _call(flow, x.to(cuda_device), -1)
    monkeypatch.setattr(flow_mod, "ALLOW_TORCH_FALLBACK", True)
    nfs_amd.reset_stats()
    y, ld = _call(flow, x.to(cuda_device), -1)
    assert nfs_amd.STATS == {"hip": 0, "torch": 1}
    assert _close_to_composite(cpu, y, ld, x, -1)


def test_train_mode_runs_the_composite(cuda_device):
    cpu = make_flow(2, 64, "relu")
    flow = _gpu(cpu, cuda_device).train()
    x = make_inputs(40, 2, seed=21)
    u0 = flow.residual_block.layer2.u.clone()
    nfs_amd.reset_stats()
    y, ld = _call(flow, x.to(cuda_device), 1)
    assert nfs_amd.STATS == {"hip": 0, "torch": 1}
    assert not torch.equal(flow.residual_block.layer2.u, u0)
    cpu.train()
    y32, ld32 = composite(cpu, x, 1)
    assert float((y.cpu() - y32).abs().max()) <= 1e-5 and float((ld.cpu() - ld32).abs().max()) <= 1e-5
    assert float((flow.residual_block.layer2.u.cpu() - cpu.residual_block.layer2.u).abs().max()) <= 1e-5


def _gclose(a, b, what, ref32, frac=2e-4):
    """max|a - b| <= max(frac * max|b|, 4 * max|ref32 - b|) (as tests/test_gpu_cnf.py)."""
    a, b, r = (torch.as_tensor(np.asarray(t.detach().cpu())).double() for t in (a, b, ref32))
    err = (a - b).abs().max().item()
    bound = max(frac * max(b.abs().max().item(), 1e-30), 4 * (r - b).abs().max().item())
    print(f"[residual grad] {what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def _nll_grads(model, x):
    model.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    loss = -model.log_prob(xr).mean()
    loss.backward()
    return loss.detach(), xr.grad, [p.grad for p in model.parameters()]


def test_training_step(cuda_device):
    """One backward of the NLL through the eval-mode layer: the kernel computes the outputs, the
    gradients recompute through the composite on the GPU (STATS["torch"] == 1, the documented route)."""
    x = make_inputs(600, 2, seed=23)
    flow = make_flow(2, 64, "tanh")
    ref64 = _nll_grads(nfs_amd.NormalizingFlowModel([as_double(flow)]).eval(), x.double())
    ref32 = _nll_grads(nfs_amd.NormalizingFlowModel([copy.deepcopy(flow)]).eval(), x)
    model = nfs_amd.NormalizingFlowModel([_gpu(flow, cuda_device)]).eval()
    nfs_amd.reset_stats()
    loss, gx, gp = _nll_grads(model, x.to(cuda_device))
    torch.cuda.synchronize()
    assert nfs_amd.STATS["torch"] == 1 and nfs_amd.STATS["hip"] >= 1, nfs_amd.STATS
    _gclose(loss, ref64[0], "loss", ref32[0])
    _gclose(gx, ref64[1], "dL/dx", ref32[1])
    names = [n for n, _ in model.named_parameters()]
    for n, g, g64, g32 in zip(names, gp, ref64[2], ref32[2]):
        assert g is not None and float(g64.abs().max()) > 0
        _gclose(g, g64, n, g32)
