"""GPU: NeuralAutoregressiveFlow's wide kernel family (csrc/nfx_naf_wide*.hip; hidden widths up to
512, opt-in through `wide_kernel = True`) against the torch composite that test_naf_cpu.py pins to the
reference, under the helper and the rules test_gpu_naf.py uses for the narrow family."""
import copy
import functools

import pytest
import torch

from conftest import assert_fp32_parity
import nfs_amd
from nfs_amd import _lib
from nfs_amd.flows import flow as flow_mod
from naf_cases import as_double, composite, hardest_row, make_flow, make_inputs, parity_case, redraw
from stale_memory import PATTERNS, poisoned_empty, same_bits
from test_gpu_naf import _assert_parity, _call, _grads

pytestmark = pytest.mark.gpu

B_MAX = 97  # four workgroups and a 1-row partial tile

# (d, hidden_dims, activation, use_layer_norm, use_residual), the smallest shapes that reach each path:
#   one row past the narrow family (129 pads to 160) with the d == 2 first-layer degree pattern;
#   the shape test_gpu_naf.py pins as outside; a residual block over five tiles, which do not divide
#   among four waves; unequal widths with LayerNorm's true-width variance at 136 (no block is made);
#   the default network at the largest dim; four layers without LayerNorm (autoregressive by the masks);
#   and four 128-wide layers, whose image (220 KiB) is what keeps them out of the narrow family: the one
#   shape class that runs naf_wide_kernel<1> (the others run <2>, and <4> from width 257)
CASES = [(2, (129,), "relu", True, True), (2, (256,), "gelu", False, True), (3, (160, 160), "elu", True, True),
         (5, (512, 136, 512), "leaky_relu", True, True), (16, (512, 512, 512), "relu", True, True),
         (16, (136, 136, 136, 136), "relu", False, True), (16, (128, 128, 128, 128), "gelu", True, True)]


def _wide(flow, dev, on=True):
    g = copy.deepcopy(flow).to(dev)
    if on:
        g.wide_kernel = True
    return g


@functools.lru_cache(maxsize=None)
def _default_case(direction):
    """NeuralAutoregressiveFlow(2) as the constructor builds it ([512, 512, 512], dropout 0.1), redrawn,
    in eval mode: (flow, x, fp32 composite, float64 composite), computed once."""
    torch.manual_seed(11)
    flow = redraw(nfs_amd.NeuralAutoregressiveFlow(2), 9091).eval()
    x = make_inputs(B_MAX, 2, seed=3 + (direction > 0))
    return flow, x, composite(flow, x, direction), composite(as_double(flow), x.double(), direction)


def _parity_rows(gpu, x, c32, c64, B, direction, dev, what):
    """test_gpu_naf.test_parity_against_float64's body: B rows as drawn; B == 1 is the hardest row, and
    the first row alone equals row 0 of the 33-row launch bit for bit."""
    rows = slice(0, B)
    if B == 1:
        y0, l0 = _call(gpu, x[:1].to(dev), direction)
        y33, l33 = _call(gpu, x[:33].to(dev), direction)
        assert torch.equal(y0[0], y33[0]) and torch.equal(l0[0], l33[0])
        r = hardest_row(c32, c64)
        rows = slice(r, r + 1)
    nfs_amd.reset_stats()
    y, ld = _call(gpu, x[rows].to(dev), direction)
    torch.cuda.synchronize()
    assert nfs_amd.STATS == {"hip": 1, "torch": 0}, nfs_amd.STATS
    assert _lib.last_kernel() == "naf_wide_kernel"
    assert y.shape == (B, x.shape[1]) and ld.shape == (B,)
    _assert_parity(y, ld, c32, c64, rows, what)
    assert float(c64[1].abs().max()) > 1e-2


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("B", [1, 31, 33, 97])
@pytest.mark.parametrize("d,hidden,act,ln,res", CASES)
def test_parity_against_float64(cuda_device, d, hidden, act, ln, res, B, direction):
    flow, x, c32, c64 = parity_case(d, hidden, act, ln, res, direction, B_MAX)
    what = f"naf wide d={d} {list(hidden)} {act} ln={ln} res={res} B={B} dir={direction}"
    _parity_rows(_wide(flow, cuda_device), x, c32, c64, B, direction, cuda_device, what)


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("B", [1, 31, 33, 97])
def test_default_constructor_parity(cuda_device, B, direction):
    """NeuralAutoregressiveFlow(2), every argument the constructor's default (dropout 0.1: eval mode)."""
    flow, x, c32, c64 = _default_case(direction)
    assert flow.conditioner.hidden_dims == [512, 512, 512] and flow.conditioner.dropout == 0.1
    _parity_rows(_wide(flow, cuda_device), x, c32, c64, B, direction, cuda_device,
                 f"naf wide default constructor B={B} dir={direction}")


def test_default_constructor_runs_in_hip_with_the_switch(cuda_device):
    """The model that raised NotImplementedError runs one launch per direction once its instance
    has `wide_kernel = True`."""
    for direction in (-1, 1):
        flow, x, c32, c64 = _default_case(direction)
        gpu = copy.deepcopy(flow).to(cuda_device).eval()
        gpu.wide_kernel = True
        nfs_amd.reset_stats()
        y, ld = _call(gpu, x.to(cuda_device), direction)
        torch.cuda.synchronize()
        assert nfs_amd.STATS == {"hip": 1, "torch": 0}, nfs_amd.STATS
        _assert_parity(y, ld, c32, c64, slice(0, B_MAX), f"naf wide default model dir={direction}")


def test_switch_off_keeps_raising(cuda_device):
    flow, x, _, _ = _default_case(-1)
    gpu = _wide(flow, cuda_device, on=False)
    for direction in (1, -1):
        with pytest.raises(NotImplementedError, match="kernel family"):
            _call(gpu, x.to(cuda_device), direction)
    far = _wide(make_flow(17, (256,), "relu"), cuda_device)
    with pytest.raises(NotImplementedError, match="wide kernel family"):
        _call(far, make_inputs(8, 17).to(cuda_device), -1)


def test_narrow_family_is_untouched(cuda_device):
    """(3, [32, 32]) runs naf_flow_kernel with the switch on or off, to the same bits, also when the
    image is packed again in between."""
    cpu = make_flow(3, (32, 32), "elu")
    x = make_inputs(70, 3, seed=61).to(cuda_device)
    off, on = _wide(cpu, cuda_device, on=False), _wide(cpu, cuda_device)
    for direction in (1, -1):
        a = _call(off, x, direction)
        b = _call(on, x, direction)
        assert _lib.last_kernel() == "naf_flow_kernel"
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        flow_mod.drop_pack_caches(on)
        on.wide_kernel = False
        c = _call(on, x, direction)
        on.wide_kernel = True
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and float(a[1].abs().max()) > 0


def test_train_mode_routes(cuda_device):
    x = make_inputs(40, 3, seed=21).to(cuda_device)
    flow = _wide(make_flow(3, (160, 160), "elu"), cuda_device)
    ye, le = _call(flow, x, -1)
    nfs_amd.reset_stats()
    yt, lt = _call(flow.train(), x, -1)
    assert nfs_amd.STATS == {"hip": 1, "torch": 0}
    assert torch.equal(yt, ye) and torch.equal(lt, le)
    drop = _wide(make_flow(3, (160, 160), "elu", dropout=0.2), cuda_device)
    nfs_amd.reset_stats()
    _call(drop.eval(), x, -1)
    assert nfs_amd.STATS == {"hip": 1, "torch": 0}
    _call(drop.train(), x, -1)
    assert nfs_amd.STATS == {"hip": 1, "torch": 1}


def test_gradients_recompute_through_the_composite(cuda_device):
    """Under grad the wide kernel computes the outputs and the gradients recompute through the
    composite on the GPU (the wide family has no fused backward, with or without fused_backward)."""
    x = make_inputs(150, 3, seed=23)
    flow = make_flow(3, (160, 160), "elu")
    ref64 = _grads(as_double(flow), x.double(), -1)
    ref32 = _grads(copy.deepcopy(flow), x, -1)

    def flat(gs):
        return torch.cat([g.detach().cpu().reshape(-1) for g in gs]).numpy()

    for fused in (False, True):
        gpu = _wide(flow, cuda_device)
        gpu.fused_backward = fused
        nfs_amd.reset_stats()
        loss, gx, gp = _grads(gpu, x.to(cuda_device), -1)
        torch.cuda.synchronize()
        assert nfs_amd.STATS == {"hip": 1, "torch": 1}, nfs_amd.STATS
        assert _lib.last_kernel() == "naf_wide_kernel" and bool(torch.isfinite(loss))
        what = f"naf wide grad fused_backward={fused} "
        assert_fp32_parity(gx.cpu().numpy(), ref32[1].numpy(), ref64[1].numpy(), what=what + "dL/dx", kind="y")
        assert all(g is not None for g in gp) and all(float(g.abs().max()) > 0 for g in ref64[2])
        assert_fp32_parity(flat(gp), flat(ref32[2]), flat(ref64[2]), what=what + "dL/dparameters", kind="y")


@pytest.mark.parametrize("d,hidden,act", [(3, (160, 160), "elu"), (2, (512, 512, 512), "relu")])
def test_independent_of_stale_memory_and_layout(cuda_device, d, hidden, act):
    """The same bits whatever LDS held before the launch and whatever `torch.empty` hands out for
    the image, the outputs and the log-det; for a strided and an offset view of the input; and for a
    row run alone."""
    cpu = make_flow(d, hidden, act)
    base = make_inputs(33, 2 * d + 2, seed=13).to(cuda_device)
    x = base[:, 1:2 * d + 1:2]
    assert not x.is_contiguous() and x.storage_offset() == 1
    dense = x.contiguous()
    ref = {}
    for direction in (1, -1):
        ref[direction] = [t.clone() for t in _call(_wide(cpu, cuda_device), dense, direction)]
        assert bool(torch.isfinite(ref[direction][0]).all()) and float(ref[direction][1].abs().max()) > 0
    for bits in PATTERNS:
        for direction in (1, -1):
            with poisoned_empty(bits) as count:
                flow = _wide(cpu, cuda_device)  # a fresh copy: its image is packed into poisoned memory
                _lib.check(_lib.lib().nfx_debug_fill_lds(bits, _lib.stream_of(dense)), "nfx_debug_fill_lds")
                y, ld = _call(flow, dense, direction)
                _lib.check(_lib.lib().nfx_debug_fill_lds(bits, _lib.stream_of(dense)), "nfx_debug_fill_lds")
                yv, ldv = _call(flow, x, direction)
                y1, ld1 = _call(flow, dense[:1], direction)
            assert count.cuda >= 3, count.cuda
            assert same_bits(y, ref[direction][0]) == [] and same_bits(ld, ref[direction][1]) == [], hex(bits)
            assert torch.equal(yv, y) and torch.equal(ldv, ld)
            assert torch.equal(y1[0], y[0]) and torch.equal(ld1[0], ld[0])
    off = base.reshape(-1)[3:3 + d * 20].view(20, d)  # contiguous, but based at an odd float
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    flow = _wide(cpu, cuda_device)
    for direction in (1, -1):
        y, ld = _call(flow, off, direction)
        yd, ldd = _call(flow, off.clone(), direction)
        assert torch.equal(y, yd) and torch.equal(ld, ldd)


@pytest.mark.parametrize("direction", [1, -1])
def test_non_finite_rows(cuda_device, direction):
    """(3, [160, 160]), 33 rows: row 5 has a NaN in column 0, which every hidden unit sees, and comes
    back as the composite's zeros with a zero log-det; row 32 (the 1-row partial tile) has 3e38 in
    column 2, which the masks let through to the one first-layer unit of degree 2: the guards zero the
    elements that the composite's guards zero, and the rest agree with it. Every other row is
    bit-equal to the clean run.

    (Column 2, because a huge value that reaches MANY units of a layer is outside what the kernels
    mirror: LayerNorm's mean is a sum here, which overflows to Inf and turns the row into NaN, hence
    zeros, where ATen's running moments stay finite, the variance alone overflows, and the row comes
    out as act(beta). The narrow kernel has the same rule; DESIGN.md notes it.)"""
    cpu = make_flow(3, (160, 160), "elu")
    flow = _wide(cpu, cuda_device)
    clean = make_inputs(33, 3, seed=5)
    x = clean.clone()
    x[5, 0] = float("nan")
    x[32, 2] = 3e38
    y, ld = (t.cpu() for t in _call(flow, x.to(cuda_device), direction))
    yc, ldc = (t.cpu() for t in _call(flow, clean.to(cuda_device), direction))
    y32, ld32 = composite(cpu, x, direction)
    print(f"[naf wide non-finite] dir={direction} row 5 {y[5].tolist()} {float(ld[5])} composite {y32[5].tolist()} "
          f"{float(ld32[5])}; row 32 {y[32].tolist()} {float(ld[32])} composite {y32[32].tolist()} {float(ld32[32])}")
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(ld).all())
    assert torch.equal(y[5], y32[5]) and torch.equal(ld[5], ld32[5])
    assert bool((y[5] == 0).all()) and float(ld[5]) == 0.0
    assert torch.equal(y[32] == 0, y32[32] == 0) and bool(ld[32] == 0) == bool(ld32[32] == 0)
    assert bool((y32[32] == 0).any()) or float(y32[32].abs().max()) > 1e37  # the value reached the transform
    assert bool(((y[32] - y32[32]).abs() <= 1e-4 * (1 + y32[32].abs())).all()) and abs(float(ld[32] - ld32[32])) <= 1e-4
    keep = [r for r in range(33) if r not in (5, 32)]
    assert torch.equal(y[keep], yc[keep]) and torch.equal(ld[keep], ldc[keep])
    assert bool(torch.isfinite(yc).all()) and bool(torch.isfinite(ldc).all()) and float(ldc.abs().max()) > 0


def test_graph_capture(cuda_device):
    flow = _wide(make_flow(2, (512, 512, 512), "relu"), cuda_device)
    x = make_inputs(B_MAX, 2, seed=17).to(cuda_device)
    eager = [t.clone() for t in _call(flow, x, -1)]
    graphed = nfs_amd.GraphedFlow(flow, x, mode="inverse")
    assert graphed.launches == 1
    graphed.static_out[0].zero_()
    graphed.static_out[1].zero_()
    out = graphed()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1]) and float(eager[1].abs().max()) > 0


def test_toggling_never_reuses_a_stale_image(cuda_device, monkeypatch):
    """On, off, on again on one instance, with a weight update while it is off: every wide call
    gives what a fresh instance gives, and the calls while off raise."""
    cpu = make_flow(2, (256,), "gelu", ln=False)
    x = make_inputs(40, 2, seed=71).to(cuda_device)
    flow = _wide(cpu, cuda_device)
    first = _call(flow, x, -1)
    fresh = _call(_wide(cpu, cuda_device), x, -1)
    assert torch.equal(first[0], fresh[0]) and torch.equal(first[1], fresh[1])
    flow.wide_kernel = False
    with pytest.raises(NotImplementedError, match="kernel family"):
        _call(flow, x, -1)
    with torch.no_grad():
        cpu.conditioner.network[0].weight.mul_(1.25)
        flow.conditioner.network[0].weight.mul_(1.25)
    flow.wide_kernel = True
    second = _call(flow, x, -1)
    fresh = _call(_wide(cpu, cuda_device), x, -1)
    assert torch.equal(second[0], fresh[0]) and torch.equal(second[1], fresh[1])
    assert float((second[0] - first[0]).abs().max()) > 1e-3
    # a shape inside both families keeps one image per family
    both = _wide(make_flow(3, (32, 32), "relu"), cuda_device)
    x3 = make_inputs(40, 3, seed=73).to(cuda_device)
    a = _call(both, x3, -1)
    assert "_nfx_pack_cache" in both.__dict__ and "_nfx_wide_pack_cache" not in both.__dict__
    assert "_nfx_wide_pack_cache" in flow.__dict__ and "_nfx_pack_cache" not in flow.__dict__
    both.wide_kernel = False
    b = _call(both, x3, -1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
