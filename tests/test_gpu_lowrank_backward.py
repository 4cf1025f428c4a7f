"""GPU: the fused backward of PlanarFlow, RadialFlow and SylvesterFlow (csrc/nfx_lowrank_bwd*.hip,
`fused_backward = True`): a single layer in either direction and a whole stack's inverse as one launch
each way, against float64 autograd of the composite run to convergence
(lowrank_backward_cases.references) by the project's criterion for gradients (gclose)."""
import copy
import functools
import json

import pytest
import torch

from conftest import load_golden
import nfs_amd
from nfs_amd import _lib
from nfs_amd.flows import lowrank
from lowrank_cases import as_double, make_inputs, make_layer, mixed_stack
from lowrank_backward_cases import autograd_grads, converged, cotangents, gclose, names, references
from test_gpu_lowrank import CASES
from test_lowrank_backward_cpu import golden_case

pytestmark = pytest.mark.gpu

FWD_KERNEL = "lowrank_stack_kernel"
STACK_BWD = "lowrank_bwd_reduce_kernel"  # the second of nfx_lrbwd_stack's two launches (after lowrank_bwd_kernel)
PARAM_BWD = "lowrank_param_grads_kernel"


def _fused(flow, dev):
    flow = copy.deepcopy(flow).to(dev)
    flow.fused_backward = True  # on the instance: the class default stays off
    return flow


@pytest.fixture
def launched(monkeypatch):
    """[(entry point, nfx_last_kernel after it)] of the backward's C calls, recorded on the thread that
    made them (autograd runs backward on its own thread, and nfx_last_kernel is per thread)."""
    ns, calls = _lib.checked(), []
    for name in ("nfx_lrbwd_stack", "nfx_lrbwd_param_grads", "nfx_lowrank_stack"):
        fn = getattr(ns, name)

        def spy(*a, _fn=fn, _n=name):
            out = _fn(*a)
            calls.append((_n, _lib.last_kernel()))
            return out
        monkeypatch.setattr(ns, name, spy)
    return calls


def _grads(target, x, gz, gld, direction):
    """[gx, one per parameter] through the public forward / inverse and autograd."""
    target.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    y, ld = target.forward(xr) if direction > 0 else target.inverse(xr)
    torch.autograd.backward([y, ld], [gz, gld])
    return [xr.grad] + [p.grad for p in target.parameters()]


def _compare(got, g64, g32, nm, what, floor=1e-3):
    assert len(got) == len(g64) == len(nm)
    for name, g, a, b in zip(nm, got, g64, g32):
        assert g is not None and g.shape == a.shape, f"{what} {name}"
        assert float(a.abs().max()) > floor, f"{what} {name}: the reference gradient is (nearly) zero"
        gclose(g, a, f"{what} {name}", b)


@functools.lru_cache(maxsize=None)
def _layer_case(kind, dim, nh, nt, B, direction):
    """(flow, x, gz, gld, g64, g32), computed once per session and never modified."""
    flow = make_layer(kind, dim, num_householder=nh, num_transforms=nt)
    x = make_inputs(B, dim, seed=41 + (direction > 0))
    # (a seed at which no reference gradient is below the 1e-3 floor of _compare: with one row, the
    # gradient of a scalar parameter is a single random number)
    gz, gld = cotangents(B, dim, seed=7 * dim + B + 2)
    return (flow, x, gz, gld) + references(flow, x, gz, gld, direction)


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("B", [1, 65, 257])
@pytest.mark.parametrize("kind,dim,nh,nt", CASES)
def test_single_layer_parity(cuda_device, launched, kind, dim, nh, nt, B, direction):
    """Every padded width at an odd and a full dim; one row, a second chunk with one row, five chunks.
    gx and every parameter against the converged float64 oracle; no composite call anywhere."""
    flow, x, gz, gld, g64, g32 = _layer_case(kind, dim, nh, nt, B, direction)
    gpu = _fused(flow, cuda_device)
    nfs_amd.reset_stats()
    got = _grads(gpu, x.to(cuda_device), gz.to(cuda_device), gld.to(cuda_device), direction)
    torch.cuda.synchronize()
    assert nfs_amd.STATS == {"torch": 0, "hip": 2}, nfs_amd.STATS
    assert [c for c in launched if c[0] != "nfx_lrbwd_param_grads"] == [("nfx_lowrank_stack", FWD_KERNEL),
                                                                        ("nfx_lrbwd_stack", STACK_BWD)]
    assert launched[-1] == ("nfx_lrbwd_param_grads", PARAM_BWD) and len(launched) == 3
    _compare(got, g64, g32, names(flow), f"{kind} dim={dim} nh={nh} nt={nt} B={B} dir={direction}")


@pytest.mark.parametrize("i", range(11))
def test_forward_against_the_references_own_gradients(cuda_device, launched, i):
    """mean(0.5 |y|^2 - ld) through forward, the 11 configurations of g23_lowrank.npz: against the
    gradients the reference itself computed, by the same criterion."""
    arrs = load_golden("g23_lowrank.npz")
    flow, x, ref = golden_case(arrs, json.loads(bytes(arrs["meta"]).decode()), i)

    def objective(f, xin):
        f.zero_grad(set_to_none=True)
        xr = xin.clone().requires_grad_(True)
        y, ld = f.forward(xr)
        (0.5 * (y * y).sum(dim=1) - ld).mean().backward()
        return {"x": xr.grad, **{k: p.grad for k, p in f.named_parameters()}}

    g32 = objective(copy.deepcopy(flow), x)
    gpu = _fused(flow, cuda_device)
    nfs_amd.reset_stats()
    got = objective(gpu, x.to(cuda_device))
    torch.cuda.synchronize()
    assert nfs_amd.STATS == {"torch": 0, "hip": 2}, nfs_amd.STATS
    assert ("nfx_lrbwd_stack", STACK_BWD) in launched and ("nfx_lowrank_stack", FWD_KERNEL) in launched
    assert set(got) == set(ref)
    for k, g in got.items():
        assert float(ref[k].abs().max()) > 0
        gclose(g, ref[k], f"g23 c{i} {k}", g32[k])


# ---- a whole stack: one launch each way -------------------------------------------------------------
def _nll_grads(model, x):
    model.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    loss = model.log_prob(xr).mean()
    loss.backward()
    return [xr.grad] + [p.grad for p in model.parameters()]


@functools.lru_cache(maxsize=None)
def _stack_case(dim, container):
    flows = mixed_stack(dim)
    x = make_inputs(257, dim, seed=43)
    gz, gld = cotangents(257, dim, seed=dim)
    if container == "model":
        g64 = _nll_grads(nfs_amd.NormalizingFlowModel([converged(f) for f in flows]).eval(), x.double())
        g32 = _nll_grads(nfs_amd.NormalizingFlowModel([converged(f, torch.float32) for f in flows]).eval(), x)
    else:
        g64, g32 = references(flows, x, gz, gld, -1)
    return flows, x, gz, gld, g64, g32


@pytest.mark.parametrize("container", ["model", "sequential"])
@pytest.mark.parametrize("dim", [3, 8, 33])
def test_stack_is_one_launch_each_way(cuda_device, launched, dim, container):
    """Planar, Radial, Sylvester, Planar, Radial through NormalizingFlowModel.log_prob(...).mean() and
    through SequentialFlow.inverse: exactly one forward-stack and one backward-stack launch."""
    flows, x, gz, gld, g64, g32 = _stack_case(dim, container)
    gpu = [_fused(f, cuda_device) for f in flows]
    xg = x.to(cuda_device)
    nfs_amd.reset_stats()
    if container == "model":
        model = nfs_amd.NormalizingFlowModel(gpu).eval()
        got = _nll_grads(model, xg)
    else:
        model = nfs_amd.SequentialFlow(gpu).eval()
        got = _grads(model, xg, gz.to(cuda_device), gld.to(cuda_device), -1)
    torch.cuda.synchronize()
    # the stack forward, the stack backward (and, for the model, the Gaussian epilogue each way)
    assert nfs_amd.STATS["torch"] == 0 and nfs_amd.STATS["hip"] == (4 if container == "model" else 2), nfs_amd.STATS
    assert [c for c in launched if c[0] != "nfx_lrbwd_param_grads"] == [("nfx_lowrank_stack", FWD_KERNEL),
                                                                        ("nfx_lrbwd_stack", STACK_BWD)]
    assert [c for c in launched if c[0] == "nfx_lrbwd_param_grads"] == [("nfx_lrbwd_param_grads", PARAM_BWD)] * 5
    _compare(got, g64, g32, names(flows), f"stack dim={dim} {container}", floor=1e-3 if container == "sequential" else 1e-5)


def test_stack_over_the_budget_runs_layer_by_layer(cuda_device, launched):
    """One layer more than the stack backward's LDS budget at DP 64: every layer runs its own fused
    backward, still without a composite call; at the budget it is one launch each way."""
    dim = 33
    cap = lowrank.max_fused_backward_layers(dim)
    assert cap == _lib.lib().nfx_lrbwd_max_layers(dim) and 16 <= cap < 64
    layers = [make_layer("planar", dim, seed=2 * i + (i % 2), bound=0.31) for i in range(cap + 1)]
    x = make_inputs(70, dim, seed=44)
    gz, gld = cotangents(70, dim, seed=1)
    g64, g32 = references(layers, x, gz, gld, -1)
    gpu = [_fused(f, cuda_device) for f in layers]
    nfs_amd.reset_stats()
    got = _grads(nfs_amd.SequentialFlow(gpu).eval(), x.to(cuda_device), gz.to(cuda_device), gld.to(cuda_device), -1)
    torch.cuda.synchronize()
    assert nfs_amd.STATS == {"torch": 0, "hip": 2 * (cap + 1)}, nfs_amd.STATS
    assert launched.count(("nfx_lrbwd_stack", STACK_BWD)) == cap + 1
    _compare(got, g64, g32, names(layers), f"{cap + 1} planar layers", floor=1e-5)
    del launched[:]
    nfs_amd.reset_stats()
    _grads(nfs_amd.SequentialFlow(gpu[:cap]).eval(), x.to(cuda_device), gz.to(cuda_device), gld.to(cuda_device), -1)
    torch.cuda.synchronize()
    assert nfs_amd.STATS == {"torch": 0, "hip": 2} and launched.count(("nfx_lrbwd_stack", STACK_BWD)) == 1


@pytest.mark.parametrize("container", ["layer", "stack"])
def test_gradients_scale_with_the_cotangents(cuda_device, container):
    """The gradient is linear in (gz, gld): with both scaled by 2^-20, what a mean over 2^20 rows hands
    to backward, every gradient is 2^-20 times the oracle's by the same criterion. (A stopping rule of
    the Sylvester adjoint iteration with an absolute floor would stop at once here.)"""
    dim, scale = 8, 2.0 ** -20
    if container == "layer":
        flow, x, gz, gld, g64, g32 = _layer_case("sylvester", dim, 8, 8, 257, -1)
        target, nm = _fused(flow, cuda_device), names(flow)
    else:
        flows, x, gz, gld, g64, g32 = _stack_case(dim, "sequential")
        target = nfs_amd.SequentialFlow([_fused(f, cuda_device) for f in flows]).eval()
        nm = names(flows)
    got = _grads(target, x.to(cuda_device), (gz * scale).to(cuda_device), (gld * scale).to(cuda_device), -1)
    for name, g, a, b in zip(nm, got, g64, g32):
        gclose(g.double() / scale, a, f"scaled cotangents, {container} {name}", b)


# ---- regrouping -------------------------------------------------------------------------------------
def test_regrouping_and_determinism(cuda_device):
    """The smallest batch at which one workgroup owns two chunks and the last chunk is partly filled:
    gx rows are bitwise those of two half-batch calls, the parameter gradients the sum of the halves,
    and two runs of the full batch give the same bits."""
    dim = 3
    L = _lib.lib()
    rows = L.nfx_lrbwd_chunk_rows(dim)
    slots = L.nfx_lrbwd_slots(1 << 40, dim, 5)
    B = rows * slots + 1
    assert L.nfx_lrbwd_slots(B, dim, 5) == slots == L.nfx_lrbwd_slots(B - 1, dim, 5) and B % rows == 1
    flows = mixed_stack(dim)
    stack = nfs_amd.SequentialFlow([_fused(f, cuda_device) for f in flows]).eval()
    x = make_inputs(B, dim, seed=45).to(cuda_device)
    gz, gld = (t.to(cuda_device) for t in cotangents(B, dim, seed=2))
    full = [g.clone() for g in _grads(stack, x, gz, gld, -1)]
    again = _grads(stack, x, gz, gld, -1)
    for name, a, b in zip(names(flows), full, again):
        assert torch.equal(a, b), name
    h = (B // 2 // rows) * rows + 7  # the halves' chunks do not line up with the full batch's
    lo = [g.clone() for g in _grads(stack, x[:h], gz[:h], gld[:h], -1)]
    hi = [g.clone() for g in _grads(stack, x[h:], gz[h:], gld[h:], -1)]
    assert torch.equal(full[0], torch.cat([lo[0], hi[0]]))
    for name, f, a, b in zip(names(flows)[1:], full[1:], lo[1:], hi[1:]):
        s64 = a.double() + b.double()
        assert float(s64.abs().max()) > 0, name
        gclose(f, s64, f"halves {name}", (a + b))


# ---- routing and guards -----------------------------------------------------------------------------
def test_switch_off_keeps_the_composite_route(cuda_device):
    x = make_inputs(40, 5, seed=46).to(cuda_device)
    gz, gld = (t.to(cuda_device) for t in cotangents(40, 5, seed=3))
    for kind in ("planar", "radial", "sylvester"):
        plain = copy.deepcopy(make_layer(kind, 5, num_householder=3, num_transforms=3)).to(cuda_device)
        for direction in (1, -1):
            nfs_amd.reset_stats()
            _grads(plain, x, gz, gld, direction)
            assert nfs_amd.STATS == {"hip": 1, "torch": 1}, (kind, nfs_amd.STATS)
    flows = [copy.deepcopy(f).to(cuda_device) for f in mixed_stack(5)]
    flows[3].fused_backward = True  # one layer of five: the stack stays layer by layer
    nfs_amd.reset_stats()
    _grads(nfs_amd.SequentialFlow(flows).eval(), x, gz, gld, -1)
    assert nfs_amd.STATS == {"hip": 6, "torch": 4}, nfs_amd.STATS


def test_train_mode_and_frozen_parameters(cuda_device, launched):
    x = make_inputs(40, 5, seed=47).to(cuda_device)
    gz, gld = (t.to(cuda_device) for t in cotangents(40, 5, seed=4))
    flow = _fused(make_layer("sylvester", 5, num_householder=3, num_transforms=3), cuda_device)
    ref = [g.clone() for g in _grads(flow, x, gz, gld, -1)]
    nfs_amd.reset_stats()
    got = _grads(flow.train(), x, gz, gld, -1)
    assert nfs_amd.STATS == {"hip": 2, "torch": 0}
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    params = list(flow.parameters())
    params[0].requires_grad_(False)
    params[-1].requires_grad_(False)
    got = _grads(flow, x, gz, gld, -1)
    assert got[1] is None and got[-1] is None and sum(g is None for g in got) == 2
    assert all(torch.equal(a, b) for a, b in zip(got, ref) if a is not None)
    # only x needs a gradient: no parameter launch at all
    for p in params:
        p.requires_grad_(False)
    del launched[:]
    got = _grads(flow, x, gz, gld, -1)
    assert torch.equal(got[0], ref[0]) and all(g is None for g in got[1:])
    assert [c[0] for c in launched] == ["nfx_lowrank_stack", "nfx_lrbwd_stack"]


@pytest.mark.parametrize("direction", [1, -1])
def test_a_nan_row_adds_nothing(cuda_device, direction):
    """A NaN input row: gx = 0 there, finite parameter gradients equal to those of the batch without
    that row (the other rows' chunk positions differ, so equal under gclose, not bitwise)."""
    dim = 5
    flows = mixed_stack(dim)
    x = make_inputs(70, dim, seed=48)
    gz, gld = cotangents(70, dim, seed=5)
    bad = x.clone()
    bad[9] = float("nan")
    keep = [i for i in range(70) if i != 9]
    targets = [nfs_amd.SequentialFlow([_fused(f, cuda_device) for f in flows]).eval()] if direction < 0 else []
    targets += [_fused(f, cuda_device) for f in flows[:3]]
    for target in targets:
        got = _grads(target, bad.to(cuda_device), gz.to(cuda_device), gld.to(cuda_device), direction)
        ref = _grads(target, x[keep].to(cuda_device), gz[keep].to(cuda_device), gld[keep].to(cuda_device), direction)
        ref = [g.clone() for g in ref]
        assert all(bool(torch.isfinite(g).all()) for g in got)
        assert float(got[0][9].abs().max()) == 0.0 and torch.equal(got[0][keep], ref[0])
        for n, (a, b) in enumerate(zip(got[1:], ref[1:])):
            assert float(b.abs().max()) > 0
            gclose(a, b.double(), f"{type(target).__name__} parameter {n}", b)


@pytest.mark.parametrize("direction", [1, -1])
def test_strided_input_and_cotangent(cuda_device, direction):
    dim = 3
    flows = [_fused(f, cuda_device) for f in mixed_stack(dim)]
    base = make_inputs(90, 8, seed=49).to(cuda_device)
    view = base[:, 1:7:2]
    gbase = make_inputs(90, 8, seed=50).to(cuda_device)
    gview = gbase[:, 0:6:2]
    gld = make_inputs(180, 1, seed=51).to(cuda_device)[::2, 0]
    assert not view.is_contiguous() and not gview.is_contiguous() and not gld.is_contiguous()
    for target in ([nfs_amd.SequentialFlow(flows).eval()] if direction < 0 else []) + [flows[0], flows[2]]:
        a = [g.clone() for g in _grads(target, view, gview, gld, direction)]
        b = _grads(target, view.contiguous(), gview.contiguous(), gld.contiguous(), direction)
        assert all(torch.equal(u, v) for u, v in zip(a, b)) and float(a[0].abs().max()) > 0


# ---- a training step ----------------------------------------------------------------------------------
def test_adam_nll_step_captured_in_a_graph(cuda_device):
    """One Adam step of the NLL of a 4-layer Planar stack, captured by GraphedTrainStep (one stream, a
    linear chain of launches: no parallel branches) and replayed once, equals the eager step bit for bit,
    and neither runs a composite layer."""
    dim = 5
    layers = [make_layer("planar", dim, seed=2 * i + (i % 2)) for i in range(4)]
    x = make_inputs(300, dim, seed=52).to(cuda_device)
    a = nfs_amd.NormalizingFlowModel([_fused(f, cuda_device) for f in layers]).eval()
    b = nfs_amd.NormalizingFlowModel([_fused(f, cuda_device) for f in layers]).eval()
    start = [p.detach().clone() for p in a.parameters()]
    opt_a = torch.optim.Adam(a.parameters(), lr=1e-2, capturable=True)
    opt_b = torch.optim.Adam(b.parameters(), lr=1e-2, capturable=True)
    nfs_amd.reset_stats()
    for _ in range(2):  # the warm-up step, then the step under test
        opt_a.zero_grad(set_to_none=True)
        loss_a = -a.log_prob(x).mean()
        loss_a.backward()
        opt_a.step()
    torch.cuda.synchronize()
    assert nfs_amd.STATS["torch"] == 0, nfs_amd.STATS
    step = nfs_amd.GraphedTrainStep(b, x, opt_b, warmup=1)
    loss_b = step()
    torch.cuda.synchronize()
    assert nfs_amd.STATS["torch"] == 0, nfs_amd.STATS
    assert torch.equal(loss_a.detach(), loss_b)
    for (n, p), q, s in zip(b.named_parameters(), a.parameters(), start):
        assert torch.equal(p, q), n
        assert float((p.detach() - s).abs().max()) > 1e-3, n
