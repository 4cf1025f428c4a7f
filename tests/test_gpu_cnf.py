"""GPU: ContinuousFlow — the whole RK4 integration in one gfx950 kernel (csrc/nfx_cnf*.hip)
against the torch composite that test_cnf_cpu.py pins to the true ODE solution."""
import numpy as np
import pytest
import torch

from conftest import assert_fp32_parity
import nfs_amd
from nfs_amd import _lib
from nfs_amd.flows import flow as flow_mod
from cnf_cases import as_double, composite, make_flow, make_inputs, parity_case

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32), (2, 64), (3, 32), (4, 64), (8, 128), (2, 128)]


def _call(flow, x, direction, times=None):
    with torch.no_grad():
        if times is not None:
            return flow.forward(x, times) if direction > 0 else flow.inverse(x, times)
        return flow.forward(x) if direction > 0 else flow.inverse(x)


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("B", [1, 31, 33, 4099])
@pytest.mark.parametrize("d,H", SHAPES)
def test_parity_against_float64(cuda_device, d, H, B, direction):
    """Below, across and beyond one 32-row tile and an odd tail, both directions: the kernel against
    the fp32 CPU composite and the float64 composite, with conftest's fixed caps; and the proof
    that the fused kernel ran."""
    flow, x, (y32, ld32), (y64, ld64) = parity_case(d, H, direction)
    gpu = make_flow(d, H).to(cuda_device)  # the same weights; the cached case stays untouched
    nfs_amd.reset_stats()
    y, ld = _call(gpu, x[:B].to(cuda_device), direction)
    torch.cuda.synchronize()
    assert nfs_amd.STATS["torch"] == 0 and nfs_amd.STATS["hip"] > 0, nfs_amd.STATS
    assert _lib.last_kernel() == "cnf_kernel"
    assert y.shape == (B, d) and ld.shape == (B,)
    what = f"cnf d={d} H={H} B={B} dir={direction}"
    assert_fp32_parity(y.cpu().numpy(), y32[:B].numpy(), y64[:B].numpy(), what=what + " y", kind="y")
    assert_fp32_parity(ld.cpu().numpy(), ld32[:B].numpy(), ld64[:B].numpy(), what=what + " ld", kind="ld")


def test_round_trip_on_the_device(cuda_device):
    """inverse(forward(z)) against z and l_fwd + l_inv against 0: at most 4x what the fp32 CPU
    composite gives on the same rows, plus 1e-6."""
    flow = make_flow(2, 64)
    z = make_inputs(512, 2, seed=11)
    xc, lfc = composite(flow, z, 1)
    zc, lic = composite(flow, xc, -1)
    cpu_z, cpu_l = float((zc - z).abs().max()), float((lfc + lic).abs().max())
    gpu = make_flow(2, 64).to(cuda_device)
    zg = z.to(cuda_device)
    xg, lf = _call(gpu, zg, 1)
    zb, li = _call(gpu, xg, -1)
    gpu_z, gpu_l = float((zb - zg).abs().max()), float((lf + li).abs().max())
    print(f"[cnf round trip] z: gpu {gpu_z:.3e} cpu fp32 {cpu_z:.3e}; log-det: gpu {gpu_l:.3e} cpu fp32 {cpu_l:.3e}")
    assert gpu_z <= 4 * cpu_z + 1e-6
    assert gpu_l <= 4 * cpu_l + 1e-6


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("d,H", [(2, 64), (3, 128)])
def test_guards_in_a_tile(cuda_device, d, H, direction):
    """NaN, +Inf and |z| = 12 rows inside 32-row tiles: they follow the contract and every other
    row is bit-identical to the run with ordinary values in their place."""
    flow = make_flow(d, H, final_scale=0.5).to(cuda_device)  # gentle: the row at 12 stays beyond the clamp
    clean = make_inputs(70, d, seed=5)
    x = clean.clone()
    x[5] = float("nan")
    x[40] = float("inf")
    x[6] = 12.0
    y, ld = (t.cpu() for t in _call(flow, x.to(cuda_device), direction))
    yc, ldc = (t.cpu() for t in _call(flow, clean.to(cuda_device), direction))
    assert bool(torch.isnan(y[5]).all()) and float(ld[5]) == 0.0       # its input row; NaN log-det -> 0
    assert torch.equal(y[40], torch.full((d,), 10.0))                   # its input row, then the clamp
    assert bool(torch.isfinite(ld[40])) and abs(float(ld[40])) <= 10.0
    assert torch.equal(y[6], torch.full((d,), 10.0))
    assert bool(torch.isfinite(ld).all())
    keep = [r for r in range(70) if r not in (5, 6, 40)]
    assert torch.equal(y[keep], yc[keep]) and torch.equal(ld[keep], ldc[keep])
    # and the same rows through the composite on the CPU
    y32, ld32 = composite(make_flow(d, H, final_scale=0.5), x, direction)
    assert torch.equal(torch.isnan(y), torch.isnan(y32))
    assert torch.equal(y[[6, 40]], y32[[6, 40]]) and float(ld32[5]) == 0.0


@pytest.mark.parametrize("direction", [1, -1])
def test_non_default_times(cuda_device, direction):
    flow = make_flow(2, 64)
    x = make_inputs(77, 2, seed=7)
    times = torch.tensor([0.0, 0.505]) if direction > 0 else torch.tensor([0.505, 0.0])
    y32, ld32 = composite(flow, x, direction, times)
    y64, ld64 = composite(as_double(flow), x.double(), direction, times)
    assert float((y64 - x.double()).abs().max()) > 0.1
    gpu = make_flow(2, 64).to(cuda_device)
    nfs_amd.reset_stats()
    y, ld = _call(gpu, x.to(cuda_device), direction, times)
    assert nfs_amd.STATS == {"hip": 1, "torch": 0}
    assert_fp32_parity(y.cpu().numpy(), y32.numpy(), y64.numpy(), what="cnf [0, 0.505] y", kind="y")
    assert_fp32_parity(ld.cpu().numpy(), ld32.numpy(), ld64.numpy(), what="cnf [0, 0.505] ld", kind="ld")
    # equal times: the input itself (no guard, no clamp) and zeros
    x[3] = 12.0
    xg = x.to(cuda_device)
    y, ld = _call(gpu, xg, direction, torch.tensor([0.3, 0.3]))
    assert nfs_amd.STATS["torch"] == 0
    assert torch.equal(y, xg) and torch.equal(ld, torch.zeros(77, device=cuda_device))


def _chain_model():
    m0, m1 = torch.tensor([1.0, 0.0]), torch.tensor([0.0, 1.0])
    torch.manual_seed(5)
    c0, c1 = nfs_amd.CouplingLayer(2, 64, m0), nfs_amd.CouplingLayer(2, 64, m1)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in list(c0.parameters()) + list(c1.parameters()):
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    return nfs_amd.NormalizingFlowModel([c0, make_flow(2, 64), c1]).eval()


def test_chain_and_accumulate(cuda_device):
    """A ContinuousFlow between two coupling layers: the model's chain (log-det accumulated in place
    by the kernels) equals the per-layer calls summed in the same fp32 order, bit for bit."""
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
    """SequentialFlow chains the layer like any other HipFlow, and a model of ContinuousFlows draws
    its base on the device and runs the forward kernels on the draw."""
    f0, f1 = make_flow(2, 64).to(cuda_device), make_flow(2, 32, seed=1).to(cuda_device)
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


@pytest.mark.parametrize("d,H", [(2, 64), (2, 128), (5, 32)])
def test_independent_of_stale_lds(cuda_device, d, H):
    flow = make_flow(d, H).to(cuda_device)
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


def test_graph_capture(cuda_device):
    flow = make_flow(2, 64).to(cuda_device)
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


@pytest.mark.parametrize("d,H", [(9, 64), (2, 48)])
def test_outside_the_kernel_family(cuda_device, d, H, monkeypatch):
    flow = make_flow(d, H).to(cuda_device)
    x = make_inputs(40, d, seed=19)
    with pytest.raises(NotImplementedError):
        _call(flow, x.to(cuda_device), -1)
    monkeypatch.setattr(flow_mod, "ALLOW_TORCH_FALLBACK", True)
    nfs_amd.reset_stats()
    y, ld = _call(flow, x.to(cuda_device), -1)
    assert nfs_amd.STATS == {"hip": 0, "torch": 1}
    y32, ld32 = composite(make_flow(d, H), x, -1)
    assert float((y.cpu() - y32).abs().max()) <= 1e-4 and float((ld.cpu() - ld32).abs().max()) <= 1e-4


def _gclose(a, b, what, ref32, frac=2e-4):
    """max|a - b| <= max(frac * max|b|, 4 * max|ref32 - b|) (as tests/test_gpu_fig_models.py)."""
    a, b, r = (torch.as_tensor(np.asarray(t.detach().cpu())).double() for t in (a, b, ref32))
    err = (a - b).abs().max().item()
    bound = max(frac * max(b.abs().max().item(), 1e-30), 4 * (r - b).abs().max().item())
    print(f"[cnf grad] {what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def _nll_grads(model, x):
    model.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    loss = -model.log_prob(xr).mean()
    loss.backward()
    return loss.detach(), xr.grad, [p.grad for p in model.parameters()]


def test_training_step(cuda_device):
    """One backward of the NLL: the kernel computes the outputs, the gradients recompute through the
    composite on the GPU (STATS["torch"] == 1, the documented route)."""
    x = make_inputs(600, 2, seed=23)
    ref64 = _nll_grads(nfs_amd.NormalizingFlowModel([as_double(make_flow(2, 64))]), x.double())
    ref32 = _nll_grads(nfs_amd.NormalizingFlowModel([make_flow(2, 64)]), x)
    model = nfs_amd.NormalizingFlowModel([make_flow(2, 64)]).to(cuda_device)
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
