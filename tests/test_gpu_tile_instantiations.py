"""GPU: every compiled instantiation of the tile-owner kernels (csrc/nfx_tile_mlp.h) runs once
against float64.

The CNF forward, the saving forward, the fused CNF backward and the residual flow are templates
over (padded hidden width, d): 24 + 16 + 16 + 24 kernels, each with a register allocation of its
own (ten of the residual ones spill to scratch, and `res_jacobian` ends on a ragged tangent group at
d = 5, 6, 7 of the 32-wide kernels and at every odd d >= 3 of the wider ones). With the NAF's three
widths that is 83 kernels. The family suites (test_gpu_cnf.py, test_gpu_cnf_backward.py,
test_gpu_residual.py) sweep batches, guards and runtime arguments at a few shapes; here every cell
of the grid runs one case of 33 rows (a full 32-row tile and a one-row tile, so both the tile body
and the range-checked tail) in both directions, under the family suite's own assertions and
tolerances. `test_the_tables_are_the_compiled_families` keeps the tables below equal to what the
library dispatches: a wider family, or a fourth width, fails it until the tables grow.
"""
import copy
import ctypes

import pytest
import torch

from conftest import assert_fp32_parity
import nfs_amd
from nfs_amd import _lib
import cnf_cases
import residual_cases
from cnf_backward_cases import NAMES
from test_gpu_cnf_backward import _check as check_cnf_backward
from test_gpu_cnf_backward import _fused
from test_gpu_naf import CASES as NAF_CASES

pytestmark = pytest.mark.gpu

B = 33
WIDTHS = (32, 64, 128)  # padded hidden widths: pick_of<1, 2, 4> tiles of 32

# (d, padded width) per kernel family
RESIDUAL_CELLS = [(d, w) for w in WIDTHS for d in range(1, 9)]     # residual_kernel<HT, D>
CNF_CELLS = [(d, w) for w in WIDTHS for d in range(1, 9)]          # cnf_kernel<HT, D>
CNF_BACKWARD_CELLS = [(d, w) for w in (32, 64) for d in range(1, 9)]  # cnf_kernel<HT, D, SAVE>, cnf_bwd_kernel<HT, D>
NAF_WIDTHS = list(WIDTHS)                                          # naf_kernel<HTM>


def padded_width(H):
    """The width of the kernel that runs hidden_dim = H (H itself beyond the widest)."""
    return next((w for w in WIDTHS if H <= w), H)


def residual_hidden(d, width):
    """One hidden_dim per residual cell, none a multiple of 32 except the largest: 24 and 40 in the
    32- and 64-wide kernels; in the 128-wide ones 72 (three of four tiles in use) at odd d and 128
    at even d."""
    return {32: 24, 64: 40, 128: 72 if d % 2 else 128}[width]


def _call(flow, x, direction):
    with torch.no_grad():
        return flow.forward(x) if direction > 0 else flow.inverse(x)


# ---- ResidualFlow -------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("d,width", RESIDUAL_CELLS)
def test_residual_cell_against_float64(cuda_device, d, width, direction):
    """test_gpu_residual.py::test_parity_against_float64 at every (d, padded width): the activation
    and the Lipschitz constant change with d, so each of the four activations and both constants
    meet every width."""
    H = residual_hidden(d, width)
    act, lipschitz = residual_cases.ACTIVATIONS[d % 4], (0.9, 1.8)[d % 2]
    assert padded_width(H) == width
    flow, x, (y32, ld32), (y64, ld64) = residual_cases.parity_case(d, H, act, lipschitz, direction, B_max=B)
    assert all(abs(s - c) > 1e-3 * c for s, c in residual_cases.sigmas(flow))  # no rounding flips a layer's regime
    assert float(ld64.abs().max()) > 1e-3  # a log-det of zero would not pass
    gpu = copy.deepcopy(flow).to(cuda_device)
    nfs_amd.reset_stats()
    y, ld = _call(gpu, x.to(cuda_device), direction)
    torch.cuda.synchronize()
    assert nfs_amd.STATS == {"hip": 1, "torch": 0}, nfs_amd.STATS
    assert _lib.last_kernel() == "residual_flow_kernel"
    assert y.shape == (B, d) and ld.shape == (B,)
    what = f"residual cell d={d} H={H} ({width}-wide) {act} L={lipschitz} dir={direction}"
    assert_fp32_parity(y.cpu().numpy(), y32.numpy(), y64.numpy(), what=what + " y", kind="y")
    assert_fp32_parity(ld.cpu().numpy(), ld32.numpy(), ld64.numpy(), what=what + " ld", kind="ld")
    e_gpu = float((ld.cpu().double() - ld64).abs().max())
    e_cpu = float((ld32.double() - ld64).abs().max())
    print(f"[{what}] log-det: gpu {e_gpu:.3e} cpu fp32 {e_cpu:.3e} of max {float(ld64.abs().max()):.3e}")
    assert e_gpu <= 4 * e_cpu + 1e-6


# ---- ContinuousFlow, forward kernel -------------------------------------------------------------
@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("d,H", CNF_CELLS)
def test_cnf_cell_against_float64(cuda_device, d, H, direction):
    """test_gpu_cnf.py::test_parity_against_float64 at every (d, H)."""
    flow, x, (y32, ld32), (y64, ld64) = cnf_cases.parity_case(d, H, direction, B_max=B)
    gpu = cnf_cases.make_flow(d, H).to(cuda_device)  # the same weights; the cached case stays untouched
    nfs_amd.reset_stats()
    y, ld = _call(gpu, x.to(cuda_device), direction)
    torch.cuda.synchronize()
    assert nfs_amd.STATS["torch"] == 0 and nfs_amd.STATS["hip"] > 0, nfs_amd.STATS
    assert _lib.last_kernel() == "cnf_kernel"
    assert y.shape == (B, d) and ld.shape == (B,)
    what = f"cnf cell d={d} H={H} dir={direction}"
    assert_fp32_parity(y.cpu().numpy(), y32.numpy(), y64.numpy(), what=what + " y", kind="y")
    assert_fp32_parity(ld.cpu().numpy(), ld32.numpy(), ld64.numpy(), what=what + " ld", kind="ld")


# ---- ContinuousFlow, saving forward and fused backward ------------------------------------------
@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("d,H", CNF_BACKWARD_CELLS)
def test_cnf_backward_cell_against_float64_autograd(cuda_device, d, H, direction):
    """test_gpu_cnf_backward.py's check (the backward kernel names, two HIP calls, gx and the six
    parameter gradients against float64 autograd under `gclose`) at every (d, H)."""
    got = check_cnf_backward(cuda_device, cnf_cases.make_flow(d, H), cnf_cases.make_inputs(B, d, seed=41), direction,
                             d + B, f"cell d={d} H={H} dir={direction}")
    assert len(got) == len(NAMES)


@pytest.mark.parametrize("d,H", CNF_BACKWARD_CELLS)
def test_cnf_saving_forward_cell_is_bit_equal_to_the_plain_one(cuda_device, d, H):
    """cnf_kernel<HT, D, true> against cnf_kernel<HT, D, false>, both directions: (y, ld) bit for
    bit, and the saved final state is the output before the guards."""
    flow = _fused(cnf_cases.make_flow(d, H), cuda_device)
    x = cnf_cases.make_inputs(B, d, seed=59).to(cuda_device)
    for direction in (1, -1):
        with torch.no_grad():
            y, ld = flow._hip_call(x, direction)
            assert _lib.last_kernel() == "cnf_kernel"
            ys, lds, traj = flow._hip_forward_save(x, direction)
            assert _lib.last_kernel() == "cnf_save_kernel"
        assert torch.equal(y, ys) and torch.equal(ld, lds), (d, H, direction)
        assert float(ld.abs().max()) > 1e-3 and float((y - x).abs().max()) > 1e-3
        n = 100
        assert traj.numel() == n * B * d + B
        yn, ldn = traj[(n - 1) * B * d:n * B * d].view(B, d), traj[n * B * d:]
        assert bool(torch.isfinite(yn).all()) and bool(torch.isfinite(ldn).all())
        assert torch.equal(yn.clamp(-10, 10), y) and torch.equal(ldn.clamp(-10, 10), ld)


# ---- the tables are the compiled families -------------------------------------------------------
def _one_function_of_the_cell(image, what):
    """image: {(d, H): packed floats}. The packed size is what the library derives from the padded
    width, so it pins this file's `padded_width` to the library's: one value inside a cell, and three
    different values across the widths at a fixed d."""
    per_cell = {}
    for (d, H), n in image.items():
        assert n > 0, (what, d, H)
        per_cell.setdefault((d, padded_width(H)), set()).add(n)
    split = {c: sorted(v) for c, v in per_cell.items() if len(v) != 1}
    assert not split, f"{what}: the packed size changes inside a cell (a width this file does not know): {split}"
    for d in sorted({d for d, _ in per_cell}):
        sizes = [next(iter(v)) for (dd, _), v in sorted(per_cell.items()) if dd == d]
        assert len(set(sizes)) == len(sizes), f"{what}: d={d}: two widths share a packed size {sizes}"


def test_the_tables_are_the_compiled_families():
    """Launches nothing. Every (d, H) that the host-side family checks accept, over d = 1..32 and
    H = 1..256, maps onto the cells the tests above run, and onto nothing else: 24 + 16 + 16 + 24 + 3
    = 83 kernels."""
    L = _lib.lib()
    residual, cnf, backward = {}, {}, {}
    for d in range(1, 33):
        for H in range(1, 257):
            acts = [L.nfx_residual_supported(1, d, H, a) for a in range(_lib.NFX_RESIDUAL_RELU, _lib.NFX_RESIDUAL_TANH + 1)]
            assert len(set(acts)) == 1, (d, H, acts)  # the activation is a runtime argument, not a kernel
            if acts[0]:
                residual[d, H] = L.nfx_residual_packed_floats(d, H)
            else:
                assert L.nfx_residual_packed_floats(d, H) == 0, (d, H)
            if L.nfx_cnf_supported(1, d, H):
                cnf[d, H] = L.nfx_cnf_packed_floats(d, H)
            if L.nfx_cnf_backward_supported(1, d, H):
                backward[d, H] = L.nfx_cnf_backward_packed_floats(d, H)
    assert {(d, padded_width(H)) for d, H in residual} == set(RESIDUAL_CELLS)
    _one_function_of_the_cell(residual, "residual")
    # every residual cell is entered by the hidden_dim its test uses
    assert all((d, residual_hidden(d, w)) in residual and padded_width(residual_hidden(d, w)) == w
               for d, w in RESIDUAL_CELLS)
    # the CNF takes its three widths exactly: a supported (d, H) is a cell as it stands
    assert set(cnf) == set(CNF_CELLS)
    assert set(backward) == set(CNF_BACKWARD_CELLS)
    _one_function_of_the_cell(cnf, "cnf")
    _one_function_of_the_cell(backward, "cnf backward")

    # The NAF: one kernel per padded width of the widest layer, whatever d. Its image is laid out per
    # layer in tiles of 32 units (naf_layout: nt = ceil(width / 32)), so it has four sizes where the
    # dispatch (hidden_tiles) has three kernels: three tiles run the four-tile kernel, and the size
    # is constant inside each block of 32 widths, not inside a cell. Pinned here: the widths the
    # family takes, and that the image knows no tile count beyond the four that those three kernels run.
    naf = {}
    for d in range(1, 33):
        for H in range(1, 257):
            widths = (ctypes.c_int * 1)(H)
            if L.nfx_naf_supported(1, d, 1, widths, _lib.NFX_NAF_RELU, 0):
                naf[d, H] = L.nfx_naf_packed_floats(d, 1, widths)
            else:
                assert L.nfx_naf_packed_floats(d, 1, widths) == 0, (d, H)
    assert {padded_width(H) for _, H in naf} == set(NAF_WIDTHS)
    assert {H for _, H in naf} == set(range(1, 129))
    for d in sorted({d for d, _ in naf}):
        sizes = {}
        for H in range(1, 129):
            sizes.setdefault((H + 31) // 32, set()).add(naf[d, H])
        assert all(len(v) == 1 for v in sizes.values()), (d, sizes)
        assert len({next(iter(v)) for v in sizes.values()}) == 4, (d, sizes)
    # test_gpu_naf.py's parity cases run all three
    assert {padded_width(max(hidden)) for _, hidden, *_ in NAF_CASES} == set(NAF_WIDTHS)

    n = len(CNF_CELLS) + 2 * len(CNF_BACKWARD_CELLS) + len(RESIDUAL_CELLS) + len(NAF_WIDTHS)
    print(f"[tile instantiations] cnf {len(CNF_CELLS)} + cnf save {len(CNF_BACKWARD_CELLS)} + cnf backward "
          f"{len(CNF_BACKWARD_CELLS)} + residual {len(RESIDUAL_CELLS)} + naf {len(NAF_WIDTHS)} = {n}")
    assert n == 83
