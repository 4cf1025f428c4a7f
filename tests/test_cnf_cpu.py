"""ContinuousFlow on the CPU: the torch composite (the scheme nfs_amd/flows/continuous.py states,
which the gfx950 kernel is tested against in test_gpu_cnf.py) pinned to the true ODE solution,
to the log-det of its own map, to the 3/8-rule tableau, and to the reference's surface."""
import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (sys.path)
import nfs_amd
from cnf_cases import as_double, composite, make_flow, make_inputs


def _np_weights(flow):
    return [p.detach().double().numpy() for lin in flow.ode_func.linears() for p in (lin.weight, lin.bias)]


def _np_field(weights, d):
    """d/dt [z, l] of one sample, written independently of the package: time is the LAST input
    column, and the divergence is the trace of the full Jacobian W3 diag(1-h2^2) W2 diag(1-h1^2)
    W1[:, :d], with sign +."""
    w1, b1, w2, b2, w3, b3 = weights

    def f(t, y):
        h1 = np.tanh(w1 @ np.concatenate([y[:d], [t]]) + b1)
        h2 = np.tanh(w2 @ h1 + b2)
        jac = (w3 * (1 - h2 ** 2)) @ (w2 * (1 - h1 ** 2)) @ w1[:, :d]
        return np.concatenate([w3 @ h2 + b3, [np.trace(jac)]])
    return f


def _scipy_solve(flow, x, t0, t1):
    integrate = pytest.importorskip("scipy.integrate")
    d = flow.dim
    f = _np_field(_np_weights(flow), d)
    out = []
    for row in x.double().numpy():
        sol = integrate.solve_ivp(f, (t0, t1), np.concatenate([row, [0.0]]), method="DOP853", rtol=1e-12, atol=1e-13)
        assert sol.success
        out.append(sol.y[:, -1])
    out = np.stack(out)
    return out[:, :d], out[:, d]


@pytest.mark.parametrize("direction,times", [(1, None), (-1, None), (1, [0.0, 0.505])])
def test_solver_matches_the_true_ode_solution(direction, times):
    """float64 composite vs scipy DOP853 (rtol 1e-12) of the same field with the closed-form trace:
    pins the field, the time column, the trace formula and its sign, and the direction handling."""
    pytest.importorskip("scipy")
    flow = as_double(make_flow(2, 64))
    x = make_inputs(8, 2).double()
    y, ld = composite(flow, x, direction, None if times is None else torch.tensor(times))
    # (the times tensor is float32: the solver integrates to fp32(0.505))
    t0, t1 = torch.tensor(times).tolist() if times is not None else ((0.0, 1.0) if direction > 0 else (1.0, 0.0))
    ys, lds = _scipy_solve(flow, x, t0, t1)
    assert float(np.abs(y.numpy()).max()) < 9.0  # far from the clamp
    assert float(np.abs(lds).max()) > 1e-3       # a vacuous field would pass anything
    assert np.abs(y.numpy() - ys).max() <= 1e-8
    assert np.abs(ld.numpy() - lds).max() <= 1e-8


@pytest.mark.parametrize("d", [2, 4])
@pytest.mark.parametrize("direction", [1, -1])
def test_log_det_is_the_log_det_of_the_discrete_map(d, direction):
    flow = as_double(make_flow(d, 32))
    x = make_inputs(3, d).double()
    _, ld = composite(flow, x, direction)
    for i in range(x.shape[0]):
        fn = (lambda r: (flow.forward(r[None]) if direction > 0 else flow.inverse(r[None]))[0][0])
        jac = torch.autograd.functional.jacobian(fn, x[i])
        sign, logabs = torch.linalg.slogdet(jac)
        assert float(sign) == 1.0
        assert abs(float(logabs) - float(ld[i])) <= 1e-8


def _steps(f, y, ld, grid, classic):
    for t0, t1 in zip(grid[:-1], grid[1:]):
        dt = t1 - t0
        if classic:
            k1, l1 = f(t0, y)
            k2, l2 = f(t0 + dt / 2, y + dt * k1 / 2)
            k3, l3 = f(t0 + dt / 2, y + dt * k2 / 2)
            k4, l4 = f(t1, y + dt * k3)
            y = y + (k1 + 2 * (k2 + k3) + k4) * dt / 6
            ld = ld + (l1 + 2 * (l2 + l3) + l4) * dt / 6
        else:
            k1, l1 = f(t0, y)
            k2, l2 = f(t0 + dt / 3, y + dt * k1 / 3)
            k3, l3 = f(t0 + 2 * dt / 3, y + dt * (k2 - k1 / 3))
            k4, l4 = f(t1, y + dt * (k1 - k2 + k3))
            y = y + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
            ld = ld + (l1 + 3 * (l2 + l3) + l4) * dt * 0.125
    return y, ld


@pytest.mark.parametrize("direction", [1, -1])
def test_tableau_is_the_three_eighths_rule(direction):
    """Four coarse steps (step_size 0.25 on the instance): the composite equals a literal
    transcription of the 3/8 rule and is NOT the classic RK4 tableau."""
    flow = as_double(make_flow(2, 64))
    flow.step_size = 0.25
    assert nfs_amd.ContinuousFlow.step_size == 0.01
    x = make_inputs(16, 2).double()
    y, ld = composite(flow, x, direction)
    grid = [0.0, 0.25, 0.5, 0.75, 1.0] if direction > 0 else [1.0, 0.75, 0.5, 0.25, 0.0]
    grid = [torch.tensor(g, dtype=torch.float64) for g in grid]
    with torch.no_grad():
        f = flow.ode_func.velocity_and_trace
        y38, ld38 = _steps(f, x, torch.zeros(16, dtype=torch.float64), grid, classic=False)
        ycl, ldcl = _steps(f, x, torch.zeros(16, dtype=torch.float64), grid, classic=True)
    assert float(y.abs().max()) < 9.0
    assert float((y - y38).abs().max()) <= 1e-12
    assert float((ld - ld38).abs().max()) <= 1e-12
    assert float((y - ycl).abs().max()) > 1e-9
    assert float((ld - ldcl).abs().max()) > 1e-9


def test_short_last_step_and_equal_times():
    flow = make_flow(2, 64)
    grid = flow.time_grid(torch.tensor([0.0, 0.505]))
    assert grid.dtype == torch.float32 and grid.shape == (52,)
    assert float(grid[0]) == 0.0 and float(grid[-1]) == float(torch.tensor(0.505))
    assert abs(float(grid[-1] - grid[-2]) - 0.005) < 1e-6
    assert float((grid[1:-1] - grid[:-2] - 0.01).abs().max()) < 1e-6
    assert flow.time_grid(torch.tensor([0.0, 1.0])).shape == (101,)
    down = flow.time_grid(torch.tensor([1.0, 0.0]))
    assert down.shape == (101,) and float(down[0]) == 1.0 and float(down[-1]) == 0.0
    assert bool((down[1:] < down[:-1]).all())
    x = make_inputs(5, 2)
    x[0] = 12.0  # equal times return the input itself: no guard, no clamp
    for call in (flow.forward, flow.inverse):
        y, ld = call(x, torch.tensor([0.3, 0.3]))
        assert torch.equal(y, x) and torch.equal(ld, torch.zeros(5))


def test_drop_in_surface():
    torch.manual_seed(0)
    flow = nfs_amd.ContinuousFlow(3)
    assert isinstance(flow, nfs_amd.flows.HipFlow) and isinstance(flow.ode_func, nfs_amd.ODEFunc)
    assert nfs_amd.flows.ContinuousFlow is nfs_amd.ContinuousFlow
    assert (flow.dim, flow.data_dim, flow.ode_func.dim, flow.hidden_dim) == (3, 3, 3, 64)
    sd = flow.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "ode_func.net.0.weight": (64, 4), "ode_func.net.0.bias": (64,),
        "ode_func.net.2.weight": (64, 64), "ode_func.net.2.bias": (64,),
        "ode_func.net.4.weight": (3, 64), "ode_func.net.4.bias": (3,)}
    # the reference initialisation: Xavier-normal weights, zero biases, zero final layer
    assert float(sd["ode_func.net.4.weight"].abs().max()) == 0.0
    assert all(float(sd[f"ode_func.net.{i}.bias"].abs().max()) == 0.0 for i in (0, 2, 4))
    assert abs(float(sd["ode_func.net.2.weight"].std()) - (2.0 / 128) ** 0.5) < 0.01
    # a fresh model is the identity with zero log-det, in both directions
    x = make_inputs(7, 3)
    for call in (flow.forward, flow.inverse):
        with torch.no_grad():
            y, ld = call(x)
        assert y.shape == (7, 3) and ld.shape == (7,)
        assert float((y - x).abs().max()) <= 1e-6 and float(ld.abs().max()) == 0.0
    flow5 = nfs_amd.ContinuousFlow(5, hidden_dim=32)
    assert flow5.ode_func.net[0].weight.shape == (32, 6) and flow5.ode_func.net[4].weight.shape == (5, 32)
    # the augmented dynamics keep the reference's ODEFunc.forward(t, [z, l]) form
    f = make_flow(2, 32)
    out = f.ode_func(torch.tensor(0.25), torch.cat([x[:, :2], torch.zeros(7, 1)], dim=1))
    assert out.shape == (7, 3)


@pytest.mark.parametrize("direction", [1, -1])
def test_guards(direction):
    flow = make_flow(2, 64, final_scale=0.5)  # gentle: the row at 12 stays beyond the clamp
    x = make_inputs(6, 2)
    x[1] = float("nan")
    x[3] = float("inf")
    x[4] = torch.tensor([12.0, -12.0])
    y, ld = composite(flow, x, direction)
    clean = x.clone()
    clean[[1, 3, 4]] = 0.0
    yc, ldc = composite(flow, clean, direction)
    assert bool(torch.isnan(y[1]).all()) and float(ld[1]) == 0.0          # NaN row: its input row, log-det 0
    assert torch.equal(y[3], torch.tensor([10.0, 10.0]))                   # Inf row: its input row, clamped
    assert bool(torch.isfinite(ld[3])) and abs(float(ld[3])) <= 10.0
    assert torch.equal(y[4], torch.tensor([10.0, -10.0]))                  # |z| = 12 is clamped
    assert bool(torch.isfinite(ld).all())
    keep = [0, 2, 5]
    assert torch.equal(y[keep], yc[keep]) and torch.equal(ld[keep], ldc[keep])  # rows never mix


def test_c_abi_validates_on_the_host():
    """The kernel family and argument checks of the C entry points answer without a GPU."""
    from nfs_amd import _lib
    L = _lib.lib()
    assert L.nfx_cnf_supported(1, 2, 64) == 1 and L.nfx_cnf_supported(1 << 40, 8, 128) == 1
    assert L.nfx_cnf_supported(1, 1, 32) == 1
    assert L.nfx_cnf_supported(1, 9, 64) == 0 and L.nfx_cnf_supported(1, 2, 48) == 0
    assert L.nfx_cnf_supported(0, 2, 64) == 0 and L.nfx_cnf_supported(1, 0, 64) == 0
    n = L.nfx_cnf_packed_floats(2, 64)
    assert n >= 64 * 64 + 64 * 3 + 64 + 64 + 2 * 64 + 2 and n % 4 == 0
    assert L.nfx_cnf_packed_floats(9, 64) == 0 and L.nfx_cnf_packed_floats(2, 48) == 0
    assert L.nfx_cnf_integrate(None, None, None, None, 16, 9, 64, 1.0, 0.0, 0.01, 0, None) == _lib.NFX_EUNSUPPORTED
    assert b"d=9" in L.nfx_last_error()
    assert L.nfx_cnf_integrate(None, None, None, None, 16, 2, 48, 1.0, 0.0, 0.01, 0, None) == _lib.NFX_EUNSUPPORTED
    assert L.nfx_cnf_integrate(None, None, None, None, 16, 2, 64, 1.0, 0.0, 0.0, 0, None) == _lib.NFX_EINVAL
    assert L.nfx_cnf_integrate(None, None, None, None, 16, 2, 64, 1.0, 0.0, 0.01, 0, None) == _lib.NFX_EINVAL
    assert b"null" in L.nfx_last_error()
    assert L.nfx_cnf_integrate(None, None, None, None, 0, 2, 64, 1.0, 0.0, 0.01, 0, None) == 0
    assert L.nfx_cnf_pack(None, None, None, None, None, None, 9, 64, None, None) == _lib.NFX_EUNSUPPORTED
