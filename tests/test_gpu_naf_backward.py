"""GPU: NeuralAutoregressiveFlow's fused backward (csrc/nfx_naf_bwd*.hip,
NeuralAutoregressiveFlow.fused_backward) — the reverse sweep of the density direction against float64
autograd on the CPU composite, by the project's criterion for these gradients
(naf_backward_cases.gclose)."""
import ctypes

import pytest
import torch

import nfs_amd
from nfs_amd import _lib
from naf_backward_cases import away_from_kinks, cotangents, gclose, names, references, trace
from naf_cases import as_double, make_flow, make_inputs
from stale_memory import poisoned_empty

pytestmark = pytest.mark.gpu

BWD_KERNELS = ("naf_bwd_kernel", "naf_bwd_reduce_kernel", "naf_bwd_finish_kernel")


def _fused(flow, device):
    flow = flow.to(device)
    flow.fused_backward = True  # on the instance: the class default stays off
    return flow


def _grads(flow, x, gz, gld, direction=-1):
    """[gx, one per parameter] through the public inverse (or forward) and autograd."""
    flow.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    y, ld = flow.inverse(xr) if direction < 0 else flow.forward(xr)
    torch.autograd.backward([y, ld], [gz, gld])
    return [xr.grad] + [p.grad for p in flow.parameters()]


def _check(cuda_device, flow_cpu, x, seed, what):
    gz, gld = cotangents(x.shape[0], x.shape[1], seed=seed)
    g64, g32 = references(flow_cpu, x, gz, gld)
    gpu = _fused(as_float(flow_cpu), cuda_device)
    launched, fused_backward = [], gpu._hip_backward

    def spy(*args, **kwargs):  # (nfx_last_kernel is per thread, and autograd runs backward on its own)
        out = fused_backward(*args, **kwargs)
        launched.append(_lib.last_kernel())
        return out
    gpu._hip_backward = spy
    nfs_amd.reset_stats()
    got = _grads(gpu, x.to(cuda_device), gz.to(cuda_device), gld.to(cuda_device))
    torch.cuda.synchronize()
    assert nfs_amd.STATS == {"torch": 0, "hip": 2}, nfs_amd.STATS
    assert len(launched) == 1 and launched[0] in BWD_KERNELS, launched
    nm = names(flow_cpu)
    for name, g, a, b in zip(nm, got, g64, g32):
        assert g is not None and g.shape == a.shape, name
        if flow_cpu.dim == 1 and name not in ("gx", nm[-1]):
            # dim 1: mu_0 and alpha_0 see no hidden unit (DeepMADE's output mask), so everything below
            # the output bias has an exactly zero gradient, in the reference and here
            assert float(a.abs().max()) == 0.0 and float(g.abs().max()) == 0.0, name
            continue
        assert float(a.abs().max()) > 0, name
        gclose(g, a, f"{what} {name}", b)
    return got


def as_float(flow_cpu):
    """A fresh fp32 copy of `flow_cpu` (weights, settings and mode)."""
    f = as_double(flow_cpu).float()
    f.load_state_dict(flow_cpu.state_dict())
    return f.train(flow_cpu.training)


CASES = [
    (1, (32,), "leaky_relu", False, True, 1),
    (2, (8, 8), "relu", False, True, 33),
    (3, (40, 40), "elu", True, True, 70),
    (5, (33, 64, 20), "leaky_relu", True, True, 33),
    (9, (64, 64), "gelu", True, False, 33),
    (16, (64, 64, 64), "relu", True, True, 70),
    (16, (64, 64, 64, 64), "relu", True, True, 70),
]


@pytest.mark.parametrize("d,hidden,act,ln,res,B", CASES)
def test_parity_against_float64_autograd(cuda_device, d, hidden, act, ln, res, B):
    """gx and every parameter gradient: one row, a partial second tile, three tiles, both padded
    widths, ragged and unequal widths, the [0, 0, 1, 1] degree pattern of dim 2, the second input quad
    (dim 9, 16), every activation, LayerNorm off and on, residual blocks and none, four layers."""
    keep, wp = (ctypes.c_int * len(hidden))(*hidden), None
    wp = ctypes.addressof(keep)
    assert _lib.lib().nfx_naf_backward_supported(B, d, len(hidden), wp, 0, 0) == 1  # ([64] * 4 at 16 fits)
    flow = make_flow(d, hidden, act, ln, res)
    x = away_from_kinks(flow, make_inputs(B, d, seed=41))
    _check(cuda_device, flow, x, d + B, f"d={d} hidden={list(hidden)} {act} ln={ln} res={res} B={B}")


def test_custom_clamps(cuda_device):
    """clamp_alpha = 1.5 and clamp_log_scale = 1.0: each clamp is reached on at least 10 rows and
    missed on at least 10, so both masks take part on both sides."""
    flow = make_flow(4, (40, 40), "elu", True, True, clamp_alpha=1.5, clamp_log_scale=1.0)
    x = away_from_kinks(flow, make_inputs(200, 4, seed=43))
    t = trace(as_double(flow), x.double())
    for reached in ((t["alpha"].abs() > 1.5).any(1), (t["nls"].abs() > 1.0).any(1)):
        assert int(reached.sum()) >= 10 and int((~reached).sum()) >= 10
    _check(cuda_device, flow, x, 7, "custom clamps")


def test_many_tiles_per_wave_and_the_cross_wave_reduction(cuda_device):
    """A batch beyond the slot cap: four-wave workgroups, several tiles per wave, a partial last
    tile, and partial sums of every slot reduced; and one between the two launch shapes' threshold
    and the cap."""
    d, hidden = 2, (8, 8)
    L = _lib.lib()
    keep = (ctypes.c_int * 2)(*hidden)
    wp = ctypes.addressof(keep)
    cap = L.nfx_naf_backward_slots(1 << 40, d, 2, wp)
    B = 32 * (2 * cap + 5) + 7
    assert L.nfx_naf_backward_block_threads(B, d, 2, wp) == 256 and L.nfx_naf_backward_slots(B, d, 2, wp) == cap
    assert (B + 31) // 32 > 2 * cap
    B2 = 32 * (cap // 2) + 3
    assert L.nfx_naf_backward_block_threads(B2, d, 2, wp) == 256
    assert cap // 2 < L.nfx_naf_backward_slots(B2, d, 2, wp) <= cap
    flow = make_flow(d, hidden, "relu", False, True)
    for batch, seed in ((B, 47), (B2, 53)):
        x = away_from_kinks(flow, make_inputs(batch, d, seed=seed))
        _check(cuda_device, flow, x, 3, f"B={batch}")


def test_forward_is_bit_equal_to_the_plain_route(cuda_device):
    for d, hidden in [(4, (64, 64)), (5, (33, 64, 20))]:
        plain = make_flow(d, hidden).to(cuda_device)
        fused = _fused(make_flow(d, hidden), cuda_device)
        x = make_inputs(77, d, seed=59).to(cuda_device)  # a partial third tile
        with torch.no_grad():
            y, ld = plain.inverse(x)
        yg, ldg = plain.inverse(x.clone().requires_grad_(True))  # the recompute route's forward
        nfs_amd.reset_stats()
        yf, ldf = fused.inverse(x.clone().requires_grad_(True))
        assert _lib.last_kernel() == "naf_flow_kernel"  # (the launch site's name for naf_kernel<HTM>)
        assert type(yf.grad_fn).__name__.startswith("_NafFunction"), type(yf.grad_fn).__name__
        assert nfs_amd.STATS == {"torch": 0, "hip": 1}
        assert torch.equal(y, yf) and torch.equal(ld, ldf) and torch.equal(yg, yf) and torch.equal(ldg, ldf)


def test_dead_rows(cuda_device):
    """A NaN row and an Inf row add nothing: finite gradients everywhere, gx = 0 on those rows,
    parameter gradients bit-equal to the batch with those rows and their cotangents zeroed."""
    d = 4
    flow = _fused(make_flow(d, (64, 64)), cuda_device)
    x = make_inputs(40, d, seed=61)
    gz, gld = cotangents(40, d, seed=13)
    bad = x.clone()
    bad[7, 1] = float("nan")
    bad[35] = float("inf")
    zx, zgz, zgld = x.clone(), gz.clone(), gld.clone()
    zx[[7, 35]] = 0.0
    zgz[[7, 35]] = 0.0
    zgld[[7, 35]] = 0.0
    got = _grads(flow, bad.to(cuda_device), gz.to(cuda_device), gld.to(cuda_device))
    ref = _grads(flow, zx.to(cuda_device), zgz.to(cuda_device), zgld.to(cuda_device))
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert float(got[0][[7, 35]].abs().max()) == 0.0
    live = [i for i in range(40) if i not in (7, 35)]
    assert torch.equal(got[0][live], ref[0][live])
    for name, a, b in zip(names(flow)[1:], got[1:], ref[1:]):
        assert torch.equal(a, b), name
        assert float(a.abs().max()) > 0, name


def test_determinism(cuda_device):
    d = 5
    flow = _fused(make_flow(d, (64, 64, 64)), cuda_device)
    x = make_inputs(300, d, seed=67).to(cuda_device)
    gz, gld = (t.to(cuda_device) for t in cotangents(300, d, seed=17))
    a = [g.clone() for g in _grads(flow, x, gz, gld)]
    b = _grads(flow, x, gz, gld)
    for name, u, v in zip(names(flow), a, b):
        assert torch.equal(u, v), name


def test_flag_and_family(cuda_device):
    """The default keeps the composite route; so do [128, 128], the sampling direction and train mode
    with dropout > 0 with the flag on; train mode with dropout == 0 is fused; frozen parameters get no
    gradient on the fused route."""
    assert nfs_amd.NeuralAutoregressiveFlow.fused_backward is False
    d = 3
    x = make_inputs(20, d, seed=73).to(cuda_device)
    gz, gld = (t.to(cuda_device) for t in cotangents(20, d, seed=23))

    def stats_of(flow, direction=-1):
        nfs_amd.reset_stats()
        got = _grads(flow, x, gz, gld, direction)
        torch.cuda.synchronize()
        return dict(nfs_amd.STATS), got

    stats, plain = stats_of(make_flow(d, (32, 32)).to(cuda_device))
    assert stats == {"hip": 1, "torch": 1}, stats
    stats, _ = stats_of(_fused(make_flow(d, (128, 128)), cuda_device))
    assert stats == {"hip": 1, "torch": 1}, stats
    stats, _ = stats_of(_fused(make_flow(d, (32, 32)), cuda_device), direction=1)
    assert stats == {"hip": 1, "torch": 1}, stats
    stats, got = stats_of(_fused(make_flow(d, (32, 32)), cuda_device).train())
    assert stats == {"hip": 2, "torch": 0}, stats
    for a, b in zip(got, plain):
        assert a.shape == b.shape
    stats, _ = stats_of(_fused(make_flow(d, (32, 32), dropout=0.2), cuda_device).train())
    assert stats["hip"] == 0 and stats["torch"] >= 1, stats
    fused = _fused(make_flow(d, (32, 32)), cuda_device)
    params = list(fused.parameters())
    params[0].requires_grad_(False)
    params[3].requires_grad_(False)
    params[-1].requires_grad_(False)
    stats, got = stats_of(fused)
    assert stats == {"hip": 2, "torch": 0}, stats
    assert got[1] is None and got[4] is None and got[-1] is None
    assert all(g is not None and g.shape == p.shape for g, p in zip(got, plain) if g is not None)
    assert sum(g is not None for g in got) == len(got) - 3


def _nll_grads(model, x):
    model.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    loss = -model.log_prob(xr).mean()
    loss.backward()
    return loss.detach(), xr.grad, [p.grad for p in model.parameters()]


def test_training_step(cuda_device):
    """One backward of the NLL on the fused route: no composite call at all."""
    d, hidden = 4, (64, 64)
    flow = make_flow(d, hidden)
    x = away_from_kinks(flow, make_inputs(600, d, seed=23))
    ref64 = _nll_grads(nfs_amd.NormalizingFlowModel([as_double(flow)]), x.double())
    ref32 = _nll_grads(nfs_amd.NormalizingFlowModel([as_float(flow)]), x)
    model = nfs_amd.NormalizingFlowModel([_fused(as_float(flow), cuda_device)]).to(cuda_device)
    nfs_amd.reset_stats()
    loss, gx, gp = _nll_grads(model, x.to(cuda_device))
    torch.cuda.synchronize()
    assert nfs_amd.STATS["torch"] == 0 and nfs_amd.STATS["hip"] >= 2, nfs_amd.STATS
    gclose(loss, ref64[0], "loss", ref32[0])
    gclose(gx, ref64[1], "dL/dx", ref32[1])
    for n, g, g64, g32 in zip([n for n, _ in model.named_parameters()], gp, ref64[2], ref32[2]):
        assert g is not None and float(g64.abs().max()) > 0
        gclose(g, g64, n, g32)


def test_stale_memory(cuda_device):
    """The workspace (slots, totals, kept activations), the image and every output come from
    torch.empty: filled with NaN bits before the run, the results are the same bits. 77 rows leave a
    ragged tile; LayerNorm off leaves the dgamma / dbeta sums of the slots unwritten."""
    for ln in (True, False):
        d, hidden = 5, (33, 64, 20)
        x = make_inputs(77, d, seed=79).to(cuda_device)
        gz, gld = (t.to(cuda_device) for t in cotangents(77, d, seed=29))
        ref = [g.clone() for g in _grads(_fused(make_flow(d, hidden, "gelu", ln), cuda_device), x, gz, gld)]
        for bits in (0xFFFFFFFF, 0x7F800000):
            with poisoned_empty(bits) as count:
                got = _grads(_fused(make_flow(d, hidden, "gelu", ln), cuda_device), x, gz, gld)
                torch.cuda.synchronize()
            assert count.cuda >= 4  # the image, gx, the gradients, the workspace
            for name, a, b in zip(names(make_flow(d, hidden, "gelu", ln)), got, ref):
                assert torch.equal(a, b), (name, hex(bits), ln)
