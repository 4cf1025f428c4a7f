"""GPU: PlanarFlow, RadialFlow and SylvesterFlow — a single layer or a whole stack of any mix of them,
in either direction, in one launch of lowrank_stack_kernel (csrc/nfx_lowrank*.hip), against the
torch composite that test_lowrank_cpu.py pins to the reference."""
import copy

import pytest
import torch

from conftest import assert_fp32_parity
import nfs_amd
from nfs_amd import _lib
from nfs_amd.flows import flow as flow_mod
from lowrank_cases import as_double, composite, make_inputs, make_layer, mixed_stack, parity_case
from stale_memory import PATTERNS, poisoned_empty
from test_gpu_residual import _gclose

pytestmark = pytest.mark.gpu

KERNEL = "lowrank_stack_kernel"
# every padded width (2, 4, 8, 16, 32, 64) at an odd and at its full dim
DIMS = (1, 2, 3, 5, 8, 17, 33, 64)
CASES = ([("planar", d, 8, None) for d in DIMS] + [("radial", d, 8, None) for d in DIMS]
         + [("sylvester", d, nh, nt) for d, nh, nt in ((2, 2, 2), (3, 8, 1), (5, 3, 3), (8, 8, 8), (17, 4, 5), (64, 8, 8))])


def _gpu(flow, dev):
    return copy.deepcopy(flow).to(dev)


def _call(flow, x, direction):
    with torch.no_grad():
        return flow.forward(x) if direction > 0 else flow.inverse(x)


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("B", [1, 63, 65, 257])
@pytest.mark.parametrize("kind,dim,nh,nt", CASES)
def test_parity_against_float64(cuda_device, kind, dim, nh, nt, B, direction):
    """Below, across and beyond one wave, and 257 rows: five one-wave workgroups, the last with a
    single row. The kernel against the fp32 and float64 CPU composites with conftest's fixed caps,
    the log-det also directly against float64, and the proof that the fused kernel ran."""
    flow, x, (y32, ld32), (y64, ld64) = parity_case(kind, dim, nh, nt, direction)
    gpu = _gpu(flow, cuda_device)
    nfs_amd.reset_stats()
    y, ld = _call(gpu, x[:B].to(cuda_device), direction)
    torch.cuda.synchronize()
    assert nfs_amd.STATS["torch"] == 0 and nfs_amd.STATS["hip"] > 0, nfs_amd.STATS
    assert _lib.last_kernel() == KERNEL
    assert y.shape == (B, dim) and ld.shape == (B,)
    what = f"{kind} dim={dim} nh={nh} nt={nt} B={B} dir={direction}"
    assert_fp32_parity(y.cpu().numpy(), y32[:B].numpy(), y64[:B].numpy(), what=what + " y", kind="y")
    assert_fp32_parity(ld.cpu().numpy(), ld32[:B].numpy(), ld64[:B].numpy(), what=what + " ld", kind="ld")
    e_gpu = float((ld.cpu().double() - ld64[:B]).abs().max())
    e_cpu = float((ld32[:B].double() - ld64[:B]).abs().max())
    print(f"[{what}] log-det: gpu {e_gpu:.3e} cpu fp32 {e_cpu:.3e} of max {float(ld64[:B].abs().max()):.3e}")
    assert e_gpu <= 4 * e_cpu + 1e-6
    if B == 257:
        assert float(ld64.abs().max()) > 1e-3 and float((y64 - x.double()).abs().max()) > 1e-3


def _layerwise(flows, x, direction):
    """The same layers launched one at a time, the log-det accumulated in place from zeros."""
    ld = torch.zeros(x.shape[0], device=x.device)
    cur = x
    for f in (flows if direction > 0 else reversed(flows)):
        out = torch.empty_like(cur)
        f._hip_launch_counted(cur, out, ld, direction, accumulate=True)
        cur = out
    return cur, ld


def _close(y, ld, ref, what):
    y32, ld32 = ref
    ey = float(((y.cpu() - y32).abs() / (1 + y32.abs())).max())
    el = float((ld.cpu() - ld32).abs().max())
    print(f"[{what}] values {ey:.3e} log-det {el:.3e}")
    assert ey <= 1e-5 and el <= 1e-4, what


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("container", ["sequential", "model"])
@pytest.mark.parametrize("dim", [3, 17])
def test_stack_equals_its_layers(cuda_device, dim, container, direction):
    """Planar, Radial, Sylvester, Planar, Radial in ONE launch, bit-equal to five launches."""
    cpu = mixed_stack(dim)
    flows = [_gpu(f, cuda_device) for f in cpu]
    stack = (nfs_amd.SequentialFlow(flows) if container == "sequential" else nfs_amd.NormalizingFlowModel(flows)).eval()
    x = make_inputs(257, dim, seed=11)
    xg = x.to(cuda_device)
    nfs_amd.reset_stats()
    y, ld = _call(stack, xg, direction)
    assert nfs_amd.STATS == {"hip": 1, "torch": 0} and _lib.last_kernel() == KERNEL
    yl, ldl = _layerwise(flows, xg, direction)
    assert nfs_amd.STATS == {"hip": 6, "torch": 0}
    assert torch.equal(y, yl) and torch.equal(ld, ldl)
    _close(y, ld, composite(nfs_amd.SequentialFlow(cpu), x, direction), f"stack dim={dim} dir={direction}")
    assert float(ld.abs().max()) > 0.1
    if container == "model":
        with torch.no_grad():
            logp = stack.log_prob(xg)
            z, li = stack.inverse(xg)
            ref, _ = nfs_amd.gauss_logprob(z, li)
        assert torch.equal(logp, ref)


@pytest.mark.parametrize("direction", [1, -1])
def test_mixed_with_other_layers_falls_back_to_per_layer_launches(cuda_device, direction):
    x = make_inputs(100, 2, seed=12)
    torch.manual_seed(5)
    coupling = nfs_amd.CouplingLayer(2, 64, torch.tensor([1.0, 0.0]))
    cpu = nfs_amd.NormalizingFlowModel(mixed_stack(2) + [coupling]).eval()
    nfs_amd.reset_stats()
    y, ld = _call(_gpu(cpu, cuda_device), x.to(cuda_device), direction)
    assert nfs_amd.STATS == {"hip": 6, "torch": 0}
    _close(y, ld, composite(cpu, x, direction), "with a CouplingLayer")
    x3 = make_inputs(100, 3, seed=13)
    cpu = nfs_amd.NormalizingFlowModel(mixed_stack(3), batch_norm_between_layers=True).eval()
    g = torch.Generator().manual_seed(3)
    for bn in cpu.batch_norms:
        bn.running_mean.copy_(0.2 * torch.randn(3, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(3, generator=g))
    nfs_amd.reset_stats()
    y, ld = _call(_gpu(cpu, cuda_device), x3.to(cuda_device), direction)
    assert nfs_amd.STATS["hip"] >= 5 and nfs_amd.STATS["torch"] == 0
    _close(y, ld, composite(cpu, x3, direction), "with between-layer BatchNorm")


def _pack_spy(monkeypatch):
    ns, calls = _lib.checked(), []
    for name in ("nfx_lowrank_pack_planar", "nfx_lowrank_pack_radial", "nfx_lowrank_pack_sylvester"):
        fn = getattr(ns, name)
        monkeypatch.setattr(ns, name, lambda *a, _fn=fn, _n=name: (calls.append(_n), _fn(*a))[1])
    return calls


@pytest.mark.parametrize("kind", ["planar", "radial", "sylvester"])
def test_runtime_arguments(cuda_device, kind, monkeypatch):
    """max_iter and tol are the layer's own: honoured, and changing either re-packs."""
    calls = _pack_spy(monkeypatch)
    cpu = make_layer(kind, 5, num_householder=3, num_transforms=3)
    gpu = _gpu(cpu, cuda_device)
    x = make_inputs(130, 5, seed=14)
    xg = x.to(cuda_device)
    full = composite(cpu, x, -1)[0]
    for n, max_iter in enumerate((0, 1, 3)):
        cpu.max_iter = gpu.max_iter = max_iter
        z, li = _call(gpu, xg, -1)
        assert len(calls) == n + 1
        zc, lc = composite(cpu, x, -1)
        _close(z, li, (zc, lc), f"{kind} max_iter={max_iter}")
        # (the truncated iterate is further from the converged one than _close's tolerance twice over)
        assert float(((zc - full).abs() / (1 + full.abs())).max()) > 2e-5
        if max_iter == 0:
            assert torch.equal(z, xg) and torch.equal(li, -_call(gpu, xg, 1)[1])
    cpu.max_iter = gpu.max_iter = 50
    cpu.tol = gpu.tol = 1e-2
    z, li = _call(gpu, xg, -1)
    assert len(calls) == 4
    zc, lc = composite(cpu, x, -1)
    assert float((zc - full).abs().max()) > 1e-6
    # (which step a row stops at may differ by rounding: both exits are within tol of each other)
    assert float((z.cpu() - zc).abs().max()) <= 2e-2 and float((z.cpu() - full).abs().max()) > 1e-6
    _call(gpu, xg, -1)
    _call(gpu, xg, 1)
    assert len(calls) == 4  # nothing changed: no re-pack


def test_rows_do_not_depend_on_their_batch(cuda_device):
    """Row i of a 257-row inverse of the mixed stack equals the same row run alone, bit for bit."""
    for dim in (3, 17):
        stack = nfs_amd.SequentialFlow([_gpu(f, cuda_device) for f in mixed_stack(dim)]).eval()
        x = make_inputs(257, dim, seed=15).to(cuda_device)
        z, ld = _call(stack, x, -1)
        for i in (0, 63, 64, 200, 256):
            z1, l1 = _call(stack, x[i:i + 1], -1)
            assert torch.equal(z1[0], z[i]) and torch.equal(l1[0], ld[i])
        z33, l33 = _call(stack, x[100:133], -1)
        assert torch.equal(z33, z[100:133]) and torch.equal(l33, ld[100:133])


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("kind,dim", [("planar", 3), ("radial", 5), ("sylvester", 8), ("planar", 64)])
def test_non_finite_rows(cuda_device, kind, dim, direction):
    """A NaN row and an Inf row among finite ones: ordinary guarded inputs. The NaN pattern of the
    values is the composite's, their log-det exactly 0 (the guard), every other row bit-equal to the
    run without them (in the inverse the NaN row keeps its wave iterating to max_iter while the
    other lanes stay frozen)."""
    cpu = make_layer(kind, dim, num_householder=4, num_transforms=min(dim, 8))
    gpu = _gpu(cpu, cuda_device)
    clean = make_inputs(70, dim, seed=16)
    x = clean.clone()
    x[5] = float("nan")
    x[40] = float("inf")
    y, ld = (t.cpu() for t in _call(gpu, x.to(cuda_device), direction))
    yc, ldc = (t.cpu() for t in _call(gpu, clean.to(cuda_device), direction))
    y32, ld32 = composite(cpu, x, direction)
    assert torch.equal(torch.isnan(y), torch.isnan(y32)) and bool(torch.isnan(y[5]).all())
    assert float(ld[5]) == 0.0 and float(ld[40]) == 0.0 and float(ld32[5]) == 0.0 and float(ld32[40]) == 0.0
    keep = [r for r in range(70) if r not in (5, 40)]
    assert torch.equal(y[keep], yc[keep]) and torch.equal(ld[keep], ldc[keep])
    assert bool(torch.isfinite(yc).all()) and bool(torch.isfinite(ldc).all())


@pytest.mark.parametrize("direction", [1, -1])
def test_independent_of_stale_memory(cuda_device, direction):
    """Outputs, the packed image and LDS filled with NaN / Inf / huge patterns beforehand: the same
    bits as the plain run (the kernel uses no LDS and writes every word it later reads)."""
    dim = 5
    cpu = mixed_stack(dim)
    x = make_inputs(77, dim, seed=17).to(cuda_device)
    base = _call(nfs_amd.SequentialFlow([_gpu(f, cuda_device) for f in cpu]).eval(), x, direction)
    assert bool(torch.isfinite(base[0]).all())
    for bits in PATTERNS:
        stack = nfs_amd.SequentialFlow([_gpu(f, cuda_device) for f in cpu]).eval()  # (packs again)
        single = _gpu(cpu[2], cuda_device)
        _lib.check(_lib.lib().nfx_debug_fill_lds(bits, _lib.stream_of(x)), "nfx_debug_fill_lds")
        with poisoned_empty(bits) as count:
            y, ld = _call(stack, x, direction)
            ys, ls = _call(single, x, direction)
        assert count.cuda >= 4  # out and the image of each call, the single layer's log-det
        assert torch.equal(y, base[0]) and torch.equal(ld, base[1]), hex(bits)
        yb, lb = _call(_gpu(cpu[2], cuda_device), x, direction)
        assert torch.equal(ys, yb) and torch.equal(ls, lb), hex(bits)


@pytest.mark.parametrize("direction", [1, -1])
def test_strided_and_offset_input_and_parameter_views(cuda_device, direction):
    dim = 3
    cpu = mixed_stack(dim)
    flows = [_gpu(f, cuda_device) for f in cpu]
    base = make_inputs(90, 8, seed=18).to(cuda_device)
    view = base[:, 1:7:2]
    assert not view.is_contiguous() and view.storage_offset() == 1
    for target in (nfs_amd.SequentialFlow(flows).eval(), flows[0], flows[2]):
        y, ld = _call(target, view, direction)
        yd, ldd = _call(target, view.contiguous(), direction)
        assert torch.equal(y, yd) and torch.equal(ld, ldd) and float(ld.abs().max()) > 0
    # the same parameters as non-contiguous views (every other element of a wider buffer) and as a
    # column-major R
    dense = nfs_amd.SequentialFlow(flows).eval()
    yd, ldd = _call(dense, view, direction)
    views = [_gpu(f, cuda_device) for f in cpu]
    for f in views:
        for mod in f.modules():
            for name, p in list(mod._parameters.items()):
                if p.dim() == 2:
                    v = p.detach().t().contiguous().t()
                else:
                    wide = torch.zeros(2 * p.numel() + 1, device=p.device)
                    wide[1::2] = p.detach()
                    v = wide[1::2]
                assert not v.is_contiguous() or v.numel() == 1
                mod._parameters[name] = torch.nn.Parameter(v)
                assert torch.equal(mod._parameters[name], p)
    y, ld = _call(nfs_amd.SequentialFlow(views).eval(), view, direction)
    assert torch.equal(y, yd) and torch.equal(ld, ldd)


def test_pack_cache_follows_the_parameters(cuda_device, monkeypatch):
    """An in-place optimiser step, load_state_dict and an assigned max_iter each reach the next
    call, each re-packs the one layer that changed, and an unchanged stack does not re-pack."""
    calls = _pack_spy(monkeypatch)
    dim = 5
    cpu = mixed_stack(dim)
    flows = [_gpu(f, cuda_device) for f in cpu]
    stack = nfs_amd.SequentialFlow(flows).eval()
    cpu_stack = nfs_amd.SequentialFlow(cpu).eval()
    x = make_inputs(128, dim, seed=19)
    xg = x.to(cuda_device)
    y0, l0 = _call(stack, xg, 1)
    assert len(calls) == 5
    _close(y0, l0, composite(cpu_stack, x, 1), "packed")
    _call(stack, xg, 1)
    _call(stack, xg, -1)
    assert len(calls) == 5
    # an in-place step on layer 0 (Planar)
    opt = torch.optim.SGD(flows[0].parameters(), lr=1.0)
    for p, q in zip(flows[0].parameters(), cpu[0].parameters()):
        p.grad = 0.05 * torch.ones_like(p)
        with torch.no_grad():
            q.sub_(0.05 * torch.ones_like(q))
    opt.step()
    y1, l1 = _call(stack, xg, 1)
    assert calls[5:] == ["nfx_lowrank_pack_planar"]
    assert float((y1 - y0).abs().max()) > 1e-3
    _close(y1, l1, composite(cpu_stack, x, 1), "after an optimiser step")
    # load_state_dict on layer 2 (Sylvester)
    sd = {k: v.clone() for k, v in cpu[2].state_dict().items()}
    sd["R"] = sd["R"] * 0.5
    sd["b"] = sd["b"] + 0.3
    cpu[2].load_state_dict(sd)
    flows[2].load_state_dict(sd)
    y2, l2 = _call(stack, xg, 1)
    assert calls[6:] == ["nfx_lowrank_pack_sylvester"]
    assert float((y2 - y1).abs().max()) > 1e-3
    _close(y2, l2, composite(cpu_stack, x, 1), "after load_state_dict")
    # an assigned max_iter on layer 1 (Radial)
    z2, _ = _call(stack, xg, -1)
    assert len(calls) == 7
    cpu[1].max_iter = flows[1].max_iter = 1
    z3, li3 = _call(stack, xg, -1)
    assert calls[7:] == ["nfx_lowrank_pack_radial"]
    assert float((z3 - z2).abs().max()) > 1e-4
    _close(z3, li3, composite(cpu_stack, x, -1), "after max_iter = 1")
    # the single-layer image follows too
    ya, _ = _call(flows[1], xg, -1)
    flows[1].max_iter = 50
    yb, _ = _call(flows[1], xg, -1)
    assert float((ya - yb).abs().max()) > 1e-4 and len(calls) == 10


def test_graph_capture(cuda_device):
    stack = nfs_amd.SequentialFlow([_gpu(f, cuda_device) for f in mixed_stack(5)]).eval()
    x = make_inputs(300, 5, seed=20).to(cuda_device)
    eager = [t.clone() for t in _call(stack, x, -1)]
    static_x = x.clone()
    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        _call(stack, static_x, -1)  # the image exists before the capture
    torch.cuda.current_stream(cuda_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = stack.inverse(static_x)
    for _ in range(2):
        out[0].zero_()
        out[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


def test_sampling_on_the_device(cuda_device):
    model = nfs_amd.NormalizingFlowModel([_gpu(f, cuda_device) for f in mixed_stack(5)]).eval()
    nfs_amd.reset_stats()
    with torch.no_grad():
        model.seed_sampler(3)
        xs, lds, zs = (t.clone() for t in model.sample_on_device(100, cuda_device))
        xf, ldf = model.forward(zs)
        model.seed_sampler(3)
        xs2, lds2, zs2 = model.sample_on_device(100, cuda_device)
        xs3, _, _ = model.sample_on_device(100, cuda_device)
    assert nfs_amd.STATS["torch"] == 0, nfs_amd.STATS
    assert torch.equal(xs, xf) and torch.equal(lds, ldf)
    assert torch.equal(xs, xs2) and torch.equal(lds, lds2) and torch.equal(zs, zs2)
    assert not torch.equal(xs3, xs)
    assert abs(float(zs.mean())) < 0.5 and 0.5 < float(zs.std()) < 1.5
    graphed = nfs_amd.GraphedFlow(model, torch.empty(100, 5, device=cuda_device), mode="sample")
    x, ld = graphed()
    torch.cuda.synchronize()
    assert graphed.launches == 2 and not graphed.fused_draw  # the stand-alone draw, then the stack
    with torch.no_grad():
        xf, ldf = model.forward(graphed.static_in)
    assert torch.equal(x, xf) and torch.equal(ld, ldf) and bool(torch.isfinite(x).all())


@pytest.mark.parametrize("case", ["dim65", "transforms9", "max_iter1001"])
def test_outside_the_kernel_family(cuda_device, case, monkeypatch):
    if case == "dim65":
        cpu = make_layer("planar", 65)
    elif case == "transforms9":
        cpu = make_layer("sylvester", 10, num_householder=4, num_transforms=9)
    else:
        cpu = make_layer("radial", 4)
        cpu.max_iter = 1001
    flow = _gpu(cpu, cuda_device)
    x = make_inputs(40, cpu.dim, seed=21)
    for direction in (1, -1):
        with pytest.raises(NotImplementedError):
            _call(flow, x.to(cuda_device), direction)
    with pytest.raises(NotImplementedError):
        _call(nfs_amd.SequentialFlow([flow]), x.to(cuda_device), -1)
    monkeypatch.setattr(flow_mod, "ALLOW_TORCH_FALLBACK", True)
    nfs_amd.reset_stats()
    y, ld = _call(flow, x.to(cuda_device), -1)
    assert nfs_amd.STATS == {"hip": 0, "torch": 1}
    _close(y, ld, composite(cpu, x, -1), case)


def _grads(model, x, objective):
    model.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    if objective == "nll":
        loss = -model.log_prob(xr).mean()
    else:
        y, ld = model.forward(xr)
        loss = (0.5 * (y * y).sum(dim=1) - ld).mean()
    loss.backward()
    return loss.detach(), xr.grad, [p.grad for p in model.parameters()]


@pytest.mark.parametrize("objective", ["nll", "forward"])
def test_training_step(cuda_device, objective):
    """One backward and one Adam step on a 4-layer Planar stack, the NLL (through inverse) and a
    forward-direction objective: the kernel computes the outputs, the gradients recompute through
    the composite on the GPU (STATS["torch"] > 0, the documented route until a fused backward
    exists) and equal the CPU composite's autograd within test_gpu_residual.py's bound."""
    x = make_inputs(300, 5, seed=22)
    layers = [make_layer("planar", 5, seed=2 * i + (i % 2)) for i in range(4)]
    ref64 = _grads(nfs_amd.NormalizingFlowModel([as_double(f) for f in layers]).eval(), x.double(), objective)
    ref32 = _grads(nfs_amd.NormalizingFlowModel([copy.deepcopy(f) for f in layers]).eval(), x, objective)
    model = nfs_amd.NormalizingFlowModel([_gpu(f, cuda_device) for f in layers]).eval()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    xg = x.to(cuda_device)
    with torch.no_grad():
        before = model.forward(xg)[0].clone()
    nfs_amd.reset_stats()
    loss, gx, gp = _grads(model, xg, objective)
    torch.cuda.synchronize()
    assert nfs_amd.STATS["torch"] == 4 and nfs_amd.STATS["hip"] >= 4, nfs_amd.STATS
    _gclose(loss, ref64[0], "loss", ref32[0])
    _gclose(gx, ref64[1], "dL/dx", ref32[1])
    names = [n for n, _ in model.named_parameters()]
    for n, g, g64, g32 in zip(names, gp, ref64[2], ref32[2]):
        assert g is not None and float(g64.abs().max()) > 0
        _gclose(g, g64, n, g32)
    opt.step()
    with torch.no_grad():
        after = model.forward(xg)[0]
    assert float((after - before).abs().max()) > 1e-4 and bool(torch.isfinite(after).all())
