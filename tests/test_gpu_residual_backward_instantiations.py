"""GPU: every compiled residual_bwd_kernel<HT, D> once. 2 padded widths x 8 dims = 16 kernels,
each entered by a hidden_dim that pads (20 -> 32, 40 -> 64): B = 33 (a partial second tile), the
inverse direction (both value passes and the solve), tanh (act'' is not zero), against float64
autograd of the converged CPU composite. With test_residual_backward_cpu.py's family test (the
backward is supported exactly on these cells) this leaves no compiled kernel unrun."""
import pytest

from nfs_amd import _lib
from residual_cases import make_flow, make_inputs
from test_gpu_residual_backward import _check

pytestmark = pytest.mark.gpu

CELLS = [(d, H) for H in (20, 40) for d in range(1, 9)]


def test_the_cells_are_the_compiled_family():
    L = _lib.lib()
    sizes = {L.nfx_residual_backward_packed_floats(d, H) for d, H in CELLS}
    assert len(sizes) == 16 and 0 not in sizes  # one image size per (d, padded width)
    assert all(L.nfx_residual_backward_supported(33, d, H, _lib.NFX_RESIDUAL_TANH) == 1 for d, H in CELLS)


@pytest.mark.parametrize("d,H", CELLS)
def test_cell_against_float64_autograd(cuda_device, d, H):
    _check(cuda_device, make_flow(d, H, "tanh", seed=5), make_inputs(33, d, seed=71), -1, d + H, f"cell d={d} H={H}")
