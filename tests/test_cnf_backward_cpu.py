"""ContinuousFlow's fused backward on the CPU: the reverse sweep the gfx950 kernel implements,
written out in float64 torch, against autograd on the composite; and the host-only behaviour of
the backward's C entry points."""
import pytest
import torch

import conftest  # noqa: F401  (sys.path)
from cnf_backward_cases import NAMES, autograd_grads, cotangents, recurrence_grads
from cnf_cases import as_double, make_flow, make_inputs


@pytest.mark.parametrize("d,H", [(1, 32), (2, 32), (5, 32), (3, 64)])
@pytest.mark.parametrize("direction", [1, -1, [0.0, 0.505], [0.7, 0.2]])
def test_reverse_sweep_equals_autograd_of_the_discrete_scheme(d, H, direction):
    """Differentiating the discrete 3/8-rule steps (not the ODE) by hand gives autograd's gradients
    of `_torch_call` to rounding: 1e-10 relative per gradient (about 2e-15 measured). One row is
    clamped in y (its input is 12), so the start masks take part."""
    flow = as_double(make_flow(d, H))
    if not isinstance(direction, int):
        direction = torch.tensor(direction)
        flow.step_size = 0.05  # 11 and 10 steps, the first interval with a short last step
    else:
        flow.step_size = 0.1
    x = make_inputs(9, d, seed=31).double()
    x[4, 0] = 12.0
    gy, gld = cotangents(9, d, seed=d + H)
    gx, gp = recurrence_grads(flow, x, direction, gy.double(), gld.double())
    rx, rp = autograd_grads(flow, x, direction, gy, gld)
    with torch.no_grad():
        y, _ = flow._torch_call(x, direction)
    assert float(y[4, 0]) == 10.0  # the clamped element
    for name, a, b in zip(NAMES, [gx] + gp, [rx] + rp):
        scale = float(b.abs().max())
        assert scale > 0, name
        assert float((a - b).abs().max()) <= 1e-10 * scale, name


def test_reverse_sweep_at_the_solver_step_and_a_clamped_log_det():
    """The default step (100 steps) with the log-det of most rows at the -10 bound."""
    flow = as_double(make_flow(2, 32))
    with torch.no_grad():
        w1 = flow.ode_func.net[0].weight
        flow.ode_func.net[2].weight.copy_(torch.eye(32, dtype=torch.float64))
        flow.ode_func.net[4].weight.copy_(4 * w1[:, :2].t())
    x = make_inputs(12, 2, seed=5).double()
    gy, gld = cotangents(12, 2, seed=9)
    _, ld = flow._torch_call(x, -1)
    assert 2 <= int((ld == -10.0).sum()) <= 10
    gx, gp = recurrence_grads(flow, x, -1, gy.double(), gld.double())
    rx, rp = autograd_grads(flow, x, -1, gy, gld)
    for name, a, b in zip(NAMES, [gx] + gp, [rx] + rp):
        assert float((a - b).abs().max()) <= 1e-10 * float(b.abs().max()), name


def test_equal_times():
    flow = as_double(make_flow(2, 32))
    gy, gld = cotangents(5, 2)
    gx, gp = recurrence_grads(flow, make_inputs(5, 2).double(), torch.tensor([0.3, 0.3]), gy, gld)
    assert torch.equal(gx, gy.double()) and all(float(g.abs().max()) == 0.0 for g in gp)


def test_c_abi_validates_on_the_host():
    """Family, sizes and argument checks of the backward's entry points answer without a GPU."""
    from nfs_amd import _lib
    L = _lib.lib()
    assert L.nfx_cnf_backward_supported(1, 2, 64) == 1 and L.nfx_cnf_backward_supported(1 << 36, 8, 32) == 1
    assert L.nfx_cnf_backward_supported(1, 1, 32) == 1
    for B, d, H in [(1, 2, 128), (1, 9, 64), (1, 2, 48), (0, 2, 64), (1, 0, 64)]:
        assert L.nfx_cnf_backward_supported(B, d, H) == 0, (B, d, H)
    # the backward image begins with the forward image and adds the two transposed H x H operands
    n = L.nfx_cnf_backward_packed_floats(2, 64)
    assert n >= L.nfx_cnf_packed_floats(2, 64) + 2 * 64 * 64 and n % 4 == 0
    assert L.nfx_cnf_backward_packed_floats(2, 128) == 0 and L.nfx_cnf_backward_packed_floats(9, 64) == 0
    # trajectory: y_1 .. y_{n-1}, then the unclamped y_n and log-det
    assert L.nfx_cnf_trajectory_floats(10, 2, 0.0, 1.0, 0.01) == 100 * 10 * 2 + 10
    assert L.nfx_cnf_trajectory_floats(10, 2, 0.0, 0.505, 0.01) == 51 * 10 * 2 + 10
    assert L.nfx_cnf_trajectory_floats(10, 2, 0.7, 0.2, 0.01) == L.nfx_cnf_trajectory_floats(10, 2, 0.2, 0.7, 0.01)
    assert L.nfx_cnf_trajectory_floats(10, 2, 0.3, 0.3, 0.01) == 0
    assert L.nfx_cnf_trajectory_floats(0, 2, 0.0, 1.0, 0.01) == 0
    # one wave per 32-row tile up to the slot cap; 64 threads per workgroup for few tiles, 256 beyond
    assert L.nfx_cnf_backward_slots(1, 2, 64) == 1 and L.nfx_cnf_backward_slots(33, 2, 64) == 2
    cap = L.nfx_cnf_backward_slots(1 << 30, 2, 64)
    assert cap % 4 == 0 and L.nfx_cnf_backward_slots(1 << 31, 2, 64) == cap
    assert L.nfx_cnf_backward_block_threads(33, 2, 64) == 64
    assert L.nfx_cnf_backward_block_threads(1 << 30, 2, 64) == 256
    assert L.nfx_cnf_backward_slots(33, 2, 128) == 0 and L.nfx_cnf_backward_block_threads(33, 9, 64) == 0
    w = L.nfx_cnf_backward_workspace_floats(33, 2, 64)
    assert w >= 2 * (2 * 64 * 64 + 64 * 3 + 2 * 64 + 2 * 64 + 2) and L.nfx_cnf_backward_workspace_floats(33, 2, 128) == 0
    assert L.nfx_cnf_backward_workspace_floats(1 << 31, 2, 64) == L.nfx_cnf_backward_workspace_floats(1 << 30, 2, 64)

    E, U = _lib.NFX_EINVAL, _lib.NFX_EUNSUPPORTED
    nul6 = (None,) * 6
    assert L.nfx_cnf_pack_backward(*nul6, 2, 128, None, None) == U and b"H=128" in L.nfx_last_error()
    assert L.nfx_cnf_pack_backward(*nul6, 9, 64, None, None) == U
    assert L.nfx_cnf_pack_backward(*nul6, 0, 64, None, None) == E
    assert L.nfx_cnf_pack_backward(*nul6, 2, 64, None, None) == E and b"null" in L.nfx_last_error()

    def save(B, d, H, step=0.01):
        return L.nfx_cnf_integrate_save(None, None, None, None, None, B, d, H, 1.0, 0.0, step, 0, None)
    assert save(16, 2, 128) == U and save(16, 9, 64) == U and save(16, 2, 48) == U
    assert save(16, 2, 64, 0.0) == E and save(-1, 2, 64) == E
    assert save(16, 2, 64) == E and b"null" in L.nfx_last_error()
    assert save(0, 2, 64) == 0

    def bwd(B, d, H, step=0.01, t1=0.0):
        return L.nfx_cnf_backward(None, None, None, None, None, None, None, None, None, *nul6, None,
                                  B, d, H, 1.0, t1, step, None)
    assert bwd(16, 2, 128) == U and b"H=128" in L.nfx_last_error()
    assert bwd(16, 9, 64) == U and bwd(16, 2, 48) == U
    assert bwd(16, 2, 64, 0.0) == E and bwd(-1, 2, 64) == E and bwd(16, 0, 64) == E
    assert bwd(16, 2, 64) == E and b"null" in L.nfx_last_error()
    assert bwd(16, 2, 64, t1=1.0) == E  # equal times still need gy, gx and the six gradients
    assert bwd(0, 2, 64) == 0
