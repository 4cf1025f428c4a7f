"""GPU: NeuralAutoregressiveFlow — the DeepMADE conditioner and the affine transform, one pass
(inverse) or `dim` passes (forward), in one gfx950 kernel (csrc/nfx_naf*.hip) against the torch
composite that test_naf_cpu.py pins to the reference."""
import copy

import pytest
import torch

from conftest import assert_fp32_parity
import nfs_amd
from nfs_amd import _lib
from nfs_amd.flows import flow as flow_mod
from naf_cases import as_double, composite, hardest_row, make_flow, make_inputs, parity_case

pytestmark = pytest.mark.gpu

# (d, hidden_dims, activation, use_layer_norm, use_residual): every padded width (32, 64, 128; 96 runs
# the 128 kernel with three tiles), every activation, LayerNorm off, residual off, unequal widths,
# widths that are no multiple of 32, d in {1, 2, 3, 8, 16}, 1 to 4 hidden layers, and the largest
# image of the family ([128, 128, 128] at d = 16)
CASES = [(1, (8,), "relu", True, True), (2, (20, 20), "elu", True, True), (3, (48,), "leaky_relu", False, True),
         (3, (32, 32), "gelu", True, False), (4, (64, 64), "relu", True, True), (8, (128, 64, 32), "elu", True, True),
         (16, (128, 128), "gelu", True, True), (5, (64, 64, 64, 64), "leaky_relu", True, True),
         (16, (128, 128, 128), "relu", True, True), (12, (96, 96), "gelu", False, True)]


def _gpu(flow, dev):
    return copy.deepcopy(flow).to(dev)


def _call(flow, x, direction):
    with torch.no_grad():
        return flow.forward(x) if direction > 0 else flow.inverse(x)


def _assert_parity(y, ld, c32, c64, rows, what):
    assert_fp32_parity(y.cpu().numpy(), c32[0][rows].numpy(), c64[0][rows].numpy(), what=what + " y", kind="y")
    assert_fp32_parity(ld.cpu().numpy(), c32[1][rows].numpy(), c64[1][rows].numpy(), what=what + " ld", kind="ld")


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("B", [1, 31, 33, 4099])
@pytest.mark.parametrize("d,hidden,act,ln,res", CASES)
def test_parity_against_float64(cuda_device, d, hidden, act, ln, res, B, direction):
    """Below, across and beyond one 32-row tile and an odd tail, both directions: the kernel against
    the fp32 CPU composite and the float64 composite with conftest's fixed caps, and the proof that
    the fused kernel ran. The batches of 31, 33 and 4,099 rows are the rows as drawn.

    B = 1 makes two one-row launches. The helper's check is made on `naf_cases.hardest_row` (chosen
    from the CPU results alone), where its mean guard over a single element means something. The
    row drawn first is launched alone as well and must equal, bit for bit, row 0 of the 33-row launch,
    which the B = 33 case holds to the helper's guards. The helper itself on that single drawn row is
    a comparison of two rounding errors: with this kernel it misses the mean guard on the log-det in 3
    of the 20 cases (kernel 5.8e-7 against reference 2.5e-7 at d = 8 [128, 64, 32] inverse, 7.9e-7
    against 7.5e-8 at d = 16 [128, 128, 128] forward, 1.1e-6 against 2.6e-7 at d = 12 [96, 96] forward,
    each within 2 ulp of a log-det of magnitude 4 to 16) while every per-element tolerance holds."""
    flow, x, c32, c64 = parity_case(d, hidden, act, ln, res, direction)
    gpu = _gpu(flow, cuda_device)
    what = f"naf d={d} {list(hidden)} {act} ln={ln} res={res} B={B} dir={direction}"
    rows = slice(0, B)
    if B == 1:
        y0, l0 = _call(gpu, x[:1].to(cuda_device), direction)
        y33, l33 = _call(gpu, x[:33].to(cuda_device), direction)
        assert torch.equal(y0[0], y33[0]) and torch.equal(l0[0], l33[0])
        r = hardest_row(c32, c64)
        rows = slice(r, r + 1)
    nfs_amd.reset_stats()
    y, ld = _call(gpu, x[rows].to(cuda_device), direction)
    torch.cuda.synchronize()
    assert nfs_amd.STATS["torch"] == 0 and nfs_amd.STATS["hip"] > 0, nfs_amd.STATS
    assert _lib.last_kernel() == "naf_flow_kernel"
    assert y.shape == (B, d) and ld.shape == (B,)
    _assert_parity(y, ld, c32, c64, rows, what)
    assert float(c64[1].abs().max()) > 1e-2


@pytest.mark.parametrize("direction", [1, -1])
def test_parity_with_every_wave_of_a_workgroup_at_work(cuda_device, direction):
    """40,000 rows of (16, [128, 128]): 1,250 tiles, more than four rounds of resident workgroups on
    any CU count up to 312, so all four waves of a workgroup compute (a small batch leaves that to
    wave 0). Same helper, both directions."""
    flow, x, c32, c64 = parity_case(16, (128, 128), "gelu", True, True, direction, 40000)
    nfs_amd.reset_stats()
    y, ld = _call(_gpu(flow, cuda_device), x.to(cuda_device), direction)
    assert nfs_amd.STATS == {"hip": 1, "torch": 0}
    _assert_parity(y, ld, c32, c64, slice(0, 40000), f"naf 40,000 rows dir={direction}")


def _against_composite(flow, x, direction, dev, what):
    y32, ld32 = composite(flow, x, direction)
    y64, ld64 = composite(as_double(flow), x.double(), direction)
    nfs_amd.reset_stats()
    y, ld = _call(_gpu(flow, dev), x.to(dev), direction)
    assert nfs_amd.STATS == {"hip": 1, "torch": 0}
    assert_fp32_parity(y.cpu().numpy(), y32.numpy(), y64.numpy(), what=what + " y", kind="y")
    assert_fp32_parity(ld.cpu().numpy(), ld32.numpy(), ld64.numpy(), what=what + " ld", kind="ld")
    return y, ld, y64, ld64


def test_rows_do_not_depend_on_their_batch(cuda_device):
    """Row i of a B = 4099 call equals, bit for bit, the same row run alone and in a batch of 33."""
    flow = _gpu(make_flow(3, (20, 20), "gelu"), cuda_device)
    x = make_inputs(4099, 3, seed=37).to(cuda_device)
    for direction in (1, -1):
        z, ld = _call(flow, x, direction)
        for i in (0, 31, 32, 2048, 4098):
            z1, l1 = _call(flow, x[i:i + 1], direction)
            assert torch.equal(z1[0], z[i]) and torch.equal(l1[0], ld[i])
        for lo in (0, 1000, 4066):
            z33, l33 = _call(flow, x[lo:lo + 33], direction)
            assert torch.equal(z33, z[lo:lo + 33]) and torch.equal(l33, ld[lo:lo + 33])


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("d,hidden,act", [(2, (64, 64), "relu"), (3, (128,), "gelu")])
def test_odd_rows_in_a_tile(cuda_device, d, hidden, act, direction):
    """A NaN row and an Inf row inside 32-row tiles come back as the composite gives them (zeros,
    log-det 0), and every other row is bit-identical to the run with ordinary values in their place."""
    cpu = make_flow(d, hidden, act)
    flow = _gpu(cpu, cuda_device)
    clean = make_inputs(70, d, seed=5)
    x = clean.clone()
    x[5] = float("nan")
    x[40] = float("inf")
    y, ld = (t.cpu() for t in _call(flow, x.to(cuda_device), direction))
    yc, ldc = (t.cpu() for t in _call(flow, clean.to(cuda_device), direction))
    y32, ld32 = composite(cpu, x, direction)
    for r in (5, 40):
        assert torch.equal(y[r], y32[r]) and torch.equal(ld[r], ld32[r])
        assert bool((y[r] == 0).all()) and float(ld[r]) == 0.0
    keep = [r for r in range(70) if r not in (5, 40)]
    assert torch.equal(y[keep], yc[keep]) and torch.equal(ld[keep], ldc[keep])
    assert bool(torch.isfinite(yc).all()) and bool(torch.isfinite(ldc).all()) and float(ldc.abs().max()) > 0


@pytest.mark.parametrize("d,hidden,act", [(2, (64, 64), "relu"), (16, (128, 128, 128), "elu"), (5, (20,), "gelu")])
def test_independent_of_stale_lds(cuda_device, d, hidden, act):
    flow = _gpu(make_flow(d, hidden, act), cuda_device)
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
    assert bool(torch.isfinite(outs[0][0]).all()) and float(outs[0][1].abs().max()) > 0


@pytest.mark.parametrize("direction", [1, -1])
def test_strided_and_offset_input(cuda_device, direction):
    flow = _gpu(make_flow(3, (16, 16), "elu"), cuda_device)
    base = make_inputs(90, 8, seed=41).to(cuda_device)
    view = base[:, 1:7:2]
    assert not view.is_contiguous() and view.storage_offset() == 1
    y, ld = _call(flow, view, direction)
    yd, ldd = _call(flow, view.contiguous(), direction)
    assert torch.equal(y, yd) and torch.equal(ld, ldd) and float(ld.abs().max()) > 0
    off = base.reshape(-1)[3:3 + 3 * 60].view(60, 3)  # contiguous, but based at an odd float
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    y, ld = _call(flow, off, direction)
    yd, ldd = _call(flow, off.clone(), direction)
    assert torch.equal(y, yd) and torch.equal(ld, ldd)


def test_runtime_arguments_and_pack_cache(cuda_device):
    """clamp_alpha and clamp_log_scale are read at every call; an in-place weight update and a
    load_state_dict reach the next call."""
    dev = cuda_device
    x = make_inputs(200, 4, seed=31)
    cpu = make_flow(4, (64, 64), "relu")
    gpu = _gpu(cpu, dev)
    for direction in (1, -1):
        y0, _ = _call(gpu, x.to(dev), direction)
        for name, value in (("clamp_alpha", 0.5), ("clamp_log_scale", 0.25)):
            old = getattr(cpu, name)
            setattr(cpu, name, value)
            setattr(gpu, name, value)
            y1, _, _, _ = _against_composite(cpu, x, direction, dev, f"naf {name}={value}")
            y1g, _ = _call(gpu, x.to(dev), direction)  # the same module object, attribute changed
            assert torch.equal(y1g, y1) and float((y1 - y0).abs().max()) > 1e-2
            setattr(cpu, name, old)
            setattr(gpu, name, old)
    y0, l0 = _call(gpu, x.to(dev), -1)
    lin = cpu.conditioner.network[0]
    noise = 0.3 * torch.randn(lin.weight.shape, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        lin.weight.add_(noise)
        gpu.conditioner.network[0].weight.add_(noise.to(dev))
        cpu.conditioner.network[1].bias.add_(0.5)
        gpu.conditioner.network[1].bias.add_(0.5)
    y1, l1 = _call(gpu, x.to(dev), -1)
    ya, la, _, _ = _against_composite(cpu, x, -1, dev, "naf after an in-place update")
    assert float((y1 - y0).abs().max()) > 1e-2
    assert torch.equal(y1, ya) and torch.equal(l1, la)  # the cached image was rebuilt from the new weights
    other = make_flow(4, (64, 64), "relu", seed=3)
    gpu.load_state_dict(other.state_dict())
    y2, l2 = _call(gpu, x.to(dev), -1)
    ya, la, _, _ = _against_composite(other, x, -1, dev, "naf after load_state_dict")
    assert float((y2 - y1).abs().max()) > 1e-2
    assert torch.equal(y2, ya) and torch.equal(l2, la)


def test_train_mode_routes(cuda_device):
    """Train mode with dropout == 0 runs the kernel (LayerNorm has no train / eval difference); with
    dropout > 0 it runs the composite."""
    x = make_inputs(40, 3, seed=21).to(cuda_device)
    flow = _gpu(make_flow(3, (32, 32), "elu"), cuda_device)
    ye, le = _call(flow, x, -1)
    nfs_amd.reset_stats()
    yt, lt = _call(flow.train(), x, -1)
    assert nfs_amd.STATS == {"hip": 1, "torch": 0}
    assert torch.equal(yt, ye) and torch.equal(lt, le)
    drop = _gpu(make_flow(3, (32, 32), "elu", dropout=0.2), cuda_device)
    nfs_amd.reset_stats()
    yd, _ = _call(drop.eval(), x, -1)
    assert nfs_amd.STATS == {"hip": 1, "torch": 0}
    yt, _ = _call(drop.train(), x, -1)
    assert nfs_amd.STATS == {"hip": 1, "torch": 1}
    assert float((yt - yd).abs().max()) > 1e-3  # units were dropped


def _outside_flows():
    replaced = make_flow(3, (16, 16), "relu")
    replaced.conditioner.network[2] = torch.nn.Tanh()
    replaced.conditioner.network[3].activation = replaced.conditioner.network[2]
    return {"wide": make_flow(2, (256,), "relu"), "d17": make_flow(17, (32,), "relu"),
            "five": make_flow(2, (8, 8, 8, 8, 8), "relu"), "replaced": replaced}


@pytest.mark.parametrize("which", ["wide", "d17", "five", "replaced"])
def test_outside_the_kernel_family(cuda_device, which, monkeypatch):
    cpu = _outside_flows()[which]
    flow = _gpu(cpu, cuda_device)
    x = make_inputs(40, cpu.dim, seed=19)
    for direction in (1, -1):
        with pytest.raises(NotImplementedError, match="kernel family"):
            _call(flow, x.to(cuda_device), direction)
    monkeypatch.setattr(flow_mod, "ALLOW_TORCH_FALLBACK", True)
    nfs_amd.reset_stats()
    y, ld = _call(flow, x.to(cuda_device), -1)
    assert nfs_amd.STATS == {"hip": 0, "torch": 1}
    y32, ld32 = composite(cpu, x, -1)
    y64, ld64 = composite(as_double(cpu), x.double(), -1)
    assert_fp32_parity(y.cpu().numpy(), y32.numpy(), y64.numpy(), what=f"naf fallback {which} y", kind="y")
    assert_fp32_parity(ld.cpu().numpy(), ld32.numpy(), ld64.numpy(), what=f"naf fallback {which} ld", kind="ld")


def test_sequential_flow_is_two_launches(cuda_device):
    f0 = _gpu(make_flow(3, (32, 32), "relu"), cuda_device)
    f1 = _gpu(make_flow(3, (48,), "gelu", seed=1), cuda_device)
    x = make_inputs(100, 3, seed=29).to(cuda_device)
    seq = nfs_amd.SequentialFlow([f0, f1])
    with torch.no_grad():
        f0.inverse(x), f1.inverse(x)  # both images packed
        nfs_amd.reset_stats()
        z, ld = seq.inverse(x)
        assert nfs_amd.STATS == {"hip": 2, "torch": 0}
        nfs_amd.reset_stats()
        xf, lf = seq.forward(x)
        assert nfs_amd.STATS == {"hip": 2, "torch": 0}
        z1, l1 = f1.inverse(x)
        z0, l0 = f0.inverse(z1)
        x0, m0 = f0.forward(x)
        x1, m1 = f1.forward(x0)
    assert torch.equal(z, z0) and torch.equal(ld, (torch.zeros_like(l1) + l1) + l0)
    assert torch.equal(xf, x1) and torch.equal(lf, (torch.zeros_like(m0) + m0) + m1)
    assert float(ld.abs().max()) > 0.1


def _grads(flow, x, direction):
    flow.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    y, ld = flow.forward(xr) if direction > 0 else flow.inverse(xr)
    loss = (0.5 * (y * y).sum(dim=1) - ld).mean()
    loss.backward()
    return loss.detach(), xr.grad, [p.grad for p in flow.parameters()]


@pytest.mark.parametrize("direction", [1, -1])
def test_gradients_recompute_through_the_composite(cuda_device, direction):
    """x.requires_grad on the GPU: the kernel computes the outputs, the gradients recompute through
    the composite on the GPU (STATS["torch"] == 1, the documented route) and match the CPU composite's
    under the same helper as the outputs."""
    x = make_inputs(300, 3, seed=23)
    flow = make_flow(3, (32, 32), "elu")
    ref64 = _grads(as_double(flow), x.double(), direction)
    ref32 = _grads(copy.deepcopy(flow), x, direction)
    gpu = _gpu(flow, cuda_device)
    nfs_amd.reset_stats()
    loss, gx, gp = _grads(gpu, x.to(cuda_device), direction)
    torch.cuda.synchronize()
    assert nfs_amd.STATS == {"hip": 1, "torch": 1}, nfs_amd.STATS
    what = f"naf grad dir={direction} "
    assert bool(torch.isfinite(loss))
    assert_fp32_parity(gx.cpu().numpy(), ref32[1].numpy(), ref64[1].numpy(), what=what + "dL/dx", kind="y")
    assert all(g is not None for g in gp) and all(float(g.abs().max()) > 0 for g in ref64[2])

    def flat(gs):  # every parameter gradient in one vector: the helper's mean guard over 1,510 elements
        return torch.cat([g.detach().cpu().reshape(-1) for g in gs]).numpy()

    assert_fp32_parity(flat(gp), flat(ref32[2]), flat(ref64[2]), what=what + "dL/dparameters", kind="y")


def test_graph_capture(cuda_device):
    """One inverse call captured on a single stream after a warm call has packed the weights: a
    replay equals the eager call bit for bit."""
    flow = _gpu(make_flow(4, (64, 64), "gelu"), cuda_device)
    x = make_inputs(300, 4, seed=17).to(cuda_device)
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
    out[0].zero_()
    out[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
