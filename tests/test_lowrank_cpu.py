"""PlanarFlow, RadialFlow and SylvesterFlow on the CPU: the torch composite
(nfs_amd/flows/lowrank.py, which the gfx950 kernel is tested against in test_gpu_lowrank.py)
against the reference's own results (tests/golden/g23_lowrank.npz, written by
tests/golden/make_golden_lowrank.py), against autograd in float64, and the host-side checks of the
C entry points."""
import ctypes
import json
import re

import pytest
import torch

from conftest import ROOT, load_golden
import nfs_amd
from nfs_amd import _lib
from lowrank_cases import (HI, KINDS, LO, as_double, composite, construct, contraction_bound, make_inputs, make_layer)

N_CONFIGS = 11
NEW_SYMBOLS = ("nfx_lowrank_supported", "nfx_lowrank_record_floats", "nfx_lowrank_pack_planar",
               "nfx_lowrank_pack_radial", "nfx_lowrank_pack_sylvester", "nfx_lowrank_stack")


@pytest.fixture(scope="module")
def golden():
    arrs = load_golden("g23_lowrank.npz")
    return arrs, json.loads(bytes(arrs["meta"]).decode())


def _construct(m):
    nh = m["num_householder"] if m["num_householder"] is not None else 8
    return construct(m["kind"], m["dim"], num_householder=nh, num_transforms=m["num_transforms"])


def _sub(arrs, prefix):
    return {k[len(prefix):]: torch.from_numpy(v.copy()) for k, v in arrs.items() if k.startswith(prefix)}


def _flow(arrs, meta, i):
    flow = _construct(meta[i])
    flow.load_state_dict(_sub(arrs, f"c{i}.sd."))
    return flow.eval()


def _t(arrs, key):
    return torch.from_numpy(arrs[key].copy())


def test_fixture_covers_the_three_kinds_inside_the_contraction_band(golden):
    arrs, meta = golden
    assert len(meta) == N_CONFIGS and {m["kind"] for m in meta} == set(KINDS)
    for i, m in enumerate(meta):
        b = contraction_bound(_flow(arrs, meta, i))
        assert LO <= b <= HI and abs(b - m["bound"]) <= 1e-6, (i, b)


@pytest.mark.parametrize("i", range(N_CONFIGS))
def test_state_dict_keys_shapes_and_seeded_construction(golden, i):
    """The reference's keys and shapes; a construction under the fixture's seed draws the same
    initial state, bit for bit (same parameters, created and initialised in the same order)."""
    arrs, meta = golden
    init = _sub(arrs, f"c{i}.init.")
    torch.manual_seed(meta[i]["seed"])
    flow = _construct(meta[i])
    sd = flow.state_dict()
    assert list(sd) == list(init)
    for k, v in sd.items():
        assert v.shape == init[k].shape and torch.equal(v, init[k]), k
    assert flow.dim == flow.data_dim == meta[i]["dim"] and (flow.max_iter, flow.tol) == (50, 1e-6)
    if meta[i]["kind"] == "sylvester":
        assert flow.num_householder == len(flow.Q.reflections) == min(meta[i]["num_householder"], flow.dim)
        assert flow.num_transforms == flow.R.shape[0]


@pytest.mark.parametrize("i", range(N_CONFIGS))
def test_outputs_match_the_reference(golden, i):
    """forward and the row-wise inverse against the reference's fp32 results at the project's fixed
    tolerances: values 1e-5 (1 + |ref|), log-dets 1e-4."""
    arrs, meta = golden
    flow, x = _flow(arrs, meta, i), _t(arrs, f"c{i}.x")
    for direction, tag, out in ((1, "fwd", "y"), (-1, "inv", "z")):
        y, ld = composite(flow, x, direction)
        yr, ldr = _t(arrs, f"c{i}.{tag}.{out}"), _t(arrs, f"c{i}.{tag}.ld")
        ey = float(((y - yr).abs() / (1 + yr.abs())).max())
        el = float((ld - ldr).abs().max())
        print(f"[lowrank c{i} {meta[i]['kind']} {tag}] values {ey:.3e} log-det {el:.3e} "
              f"(max |log-det| {float(ldr.abs().max()):.3e})")
        assert ey <= 1e-5 and el <= 1e-4
        assert float(ldr.abs().max()) > 1e-3 and float((yr - x).abs().max()) > 1e-2


@pytest.mark.parametrize("i", range(N_CONFIGS))
def test_gradients_match_the_reference(golden, i):
    """Gradients of mean(0.5 |y|^2 - ld) through forward, with respect to x and every parameter,
    within 2e-5 of max|ref| per tensor (the bound of test_residual_cpu.py's like-for-like
    comparison)."""
    arrs, meta = golden
    flow, x = _flow(arrs, meta, i), _t(arrs, f"c{i}.x")
    xr = x.clone().requires_grad_(True)
    y, ld = flow.forward(xr)
    (0.5 * (y * y).sum(dim=1) - ld).mean().backward()
    grads = {"x": xr.grad, **{k: p.grad for k, p in flow.named_parameters()}}
    assert set(grads) == {k for k in _sub(arrs, f"c{i}.grad.")}
    for k, g in grads.items():
        ref = _t(arrs, f"c{i}.grad.{k}")
        err, scale = float((g - ref).abs().max()), float(ref.abs().max())
        print(f"[lowrank c{i} grad] {k}: {err:.3e} of {scale:.3e}")
        assert scale > 0 and err <= 2e-5 * scale, k


def _dim3(kind):
    return make_layer(kind, 3, num_householder=3, num_transforms=2)


@pytest.mark.parametrize("kind", KINDS)
def test_float64_under_no_grad_and_gradcheck(kind):
    """The composite runs in float64 under torch.no_grad(); gradcheck on forward with the settings of
    the reference's test_gradcheck (eps 1e-6, atol 1e-4, rtol 1e-3)."""
    flow = as_double(_dim3(kind))
    x = make_inputs(6, 3, seed=1).double()
    with torch.no_grad():
        for direction in (1, -1):
            y, ld = flow.forward(x) if direction > 0 else flow.inverse(x)
            assert y.dtype == ld.dtype == torch.float64 and not y.requires_grad
        z, li = flow.inverse(flow.forward(x)[0])
    assert float((z - x).abs().max()) <= 1e-4
    xr = x[:3].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: flow.forward(t), (xr,), eps=1e-6, atol=1e-4, rtol=1e-3)


@pytest.mark.parametrize("dim", [1, 3, 8])
@pytest.mark.parametrize("kind", ["planar", "radial"])
def test_log_det_is_the_jacobians(kind, dim):
    """Analytic log-det against log|det| of autograd's Jacobian, rel / abs 1e-4 as in the reference's
    test_logdet_autodiff. Sylvester is excluded on purpose: its log-det is the reference's formula
    log|det(I + R R^T diag(psi))|, which is not its Jacobian's (Q is applied twice as Q, never as
    Q^T); the composite reproduces that formula and test_outputs_match_the_reference pins it."""
    flow = as_double(make_layer(kind, dim))
    x = make_inputs(5, dim, seed=2).double()
    _, ld = composite(flow, x, 1)
    for r in range(5):
        jac = torch.autograd.functional.jacobian(lambda t: flow.forward(t.unsqueeze(0))[0].squeeze(0), x[r])
        ref = torch.log(torch.abs(torch.det(jac)))
        assert torch.allclose(ld[r], ref, rtol=1e-4, atol=1e-4), (kind, dim, r, float(ld[r]), float(ref))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [3, 12])
def test_a_rows_inverse_does_not_depend_on_its_batch(kind, dim):
    """The per-sample stopping rule: bit for bit."""
    flow = make_layer(kind, dim, num_householder=4, num_transforms=min(dim, 5))
    x = make_inputs(40, dim, seed=4)
    z, ld = composite(flow, x, -1)
    for r in (0, 7, 39):
        z1, l1 = composite(flow, x[r:r + 1], -1)
        assert torch.equal(z1[0], z[r]) and torch.equal(l1[0], ld[r])
    z9, l9 = composite(flow, x[11:20], -1)
    assert torch.equal(z9, z[11:20]) and torch.equal(l9, ld[11:20])
    y, _ = composite(flow, x, 1)
    assert float((composite(flow, y, -1)[0] - x).abs().max()) <= 5e-5


@pytest.mark.parametrize("kind", KINDS)
def test_stopping_rule_edges(kind):
    """max_iter = 0 returns z = x with minus the forward log-det there; a Radial row at x = z0 has
    g = 0, so it stops at the first step with z = x."""
    flow = _dim3(kind)
    x = make_inputs(9, 3, seed=5)
    flow.max_iter = 0
    z, li = composite(flow, x, -1)
    _, lf = composite(flow, x, 1)
    assert torch.equal(z, x) and torch.equal(li, -lf)
    flow.max_iter = 50
    if kind == "radial":
        x0 = flow.z0.detach().clone().unsqueeze(0)
        z, _ = composite(flow, x0, -1)
        assert torch.equal(z, x0)
    # one step from a contraction is not yet the fixed point; a loose tol stops earlier
    full = composite(flow, x, -1)[0]
    flow.max_iter = 1
    assert float((composite(flow, x, -1)[0] - full).abs().max()) > 1e-4
    flow.max_iter, flow.tol = 50, 1e-2
    assert float((composite(flow, x, -1)[0] - full).abs().max()) > 1e-6


def test_helper_methods():
    p, r, s = _dim3("planar"), _dim3("radial"), make_layer("sylvester", 5, num_householder=8, num_transforms=3)
    u = p._get_u()
    assert u.shape == (3,) and float(torch.dot(u, p.w).detach()) >= -1
    alpha = r._get_alpha()
    alpha = alpha.detach()
    assert float(alpha) > 0 and float(r._get_beta(alpha).detach()) > -float(alpha)
    assert s.num_householder == 5 and s.num_transforms == 3 and s.R.shape == (3, 5)
    q = s.get_orthogonal_matrix()
    assert q.shape == (5, 5) and float(s.check_orthogonality()) <= 1e-5 and float(s.Q.log_det()) == 0.0
    h = s.Q.reflections[0]
    v = torch.randn(5)
    assert torch.allclose(h(v), h.get_matrix() @ v, atol=1e-6)
    rows = torch.randn(4, 5)
    assert torch.allclose(s.Q(rows), rows @ q.t(), atol=1e-5)
    assert nfs_amd.SylvesterFlow(3).num_transforms == 3 and nfs_amd.OrthogonalMatrix(3).num_householder == 3


# ---- the C entry points, on the host --------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    header = open(f"{ROOT}/include/nfx.h").read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert hasattr(lib, name) and name in _lib._SIGNATURES and hasattr(_lib.checked(), name), name
    assert "nfx_lowrank_supported" in _lib._VALUE_RETURNING
    assert [n for n in _lib.EXPORTED_SYMBOLS if n.startswith("nfx_lowrank")] == list(NEW_SYMBOLS)
    assert _lib.lib().nfx_abi_version() == 3


def test_supported_and_record_floats_agree_with_the_documented_family():
    L = _lib.lib()
    for dim in range(0, 81):
        inside = 1 <= dim <= 64
        rec = L.nfx_lowrank_record_floats(dim)
        if inside:
            dp = next(p for p in (2, 4, 8, 16, 32, 64) if p >= dim)
            assert rec == 80 + 16 * dp and rec % 4 == 0
        else:
            assert rec == 0
        for n in range(0, 301):
            assert L.nfx_lowrank_supported(16, dim, n) == int(inside and 1 <= n <= 256), (dim, n)
    assert L.nfx_lowrank_supported(0, 8, 4) == 0 and L.nfx_lowrank_supported(1 << 40, 8, 4) == 1
    assert L.nfx_lowrank_record_floats(-3) == 0


def test_invalid_arguments_fail_on_the_host():
    L = _lib.lib()
    EINVAL, EUNSUP = _lib.NFX_EINVAL, _lib.NFX_EUNSUPPORTED
    one = ctypes.c_void_p(16)  # never dereferenced: every call below returns before a launch
    assert L.nfx_lowrank_stack(None, 4, None, None, None, 16, 8, 0, 0, None) == EINVAL
    assert b"direction" in L.nfx_last_error()
    assert L.nfx_lowrank_stack(None, 4, None, None, None, -1, 8, 1, 0, None) == EINVAL
    assert L.nfx_lowrank_stack(None, 0, None, None, None, 16, 8, 1, 0, None) == EINVAL
    assert L.nfx_lowrank_stack(None, 4, None, None, None, 16, 65, 1, 0, None) == EUNSUP
    assert L.nfx_lowrank_stack(None, 257, None, None, None, 16, 8, 1, 0, None) == EUNSUP
    assert L.nfx_lowrank_stack(None, 4, None, None, None, 16, 8, 1, 0, None) == EINVAL  # null pointers
    assert L.nfx_lowrank_stack(one, 4, one, one, one, 16, 8, -1, 0, None) == EINVAL and b"alias" in L.nfx_last_error()
    assert L.nfx_lowrank_stack(None, 4, None, None, None, 0, 8, 1, 0, None) == 0  # B == 0 is a no-op
    assert L.nfx_lowrank_pack_planar(None, None, None, 8, 50, 1e-6, None, None) == EINVAL
    assert L.nfx_lowrank_pack_planar(one, one, one, 65, 50, 1e-6, one, None) == EUNSUP
    assert L.nfx_lowrank_pack_planar(one, one, one, 8, 1001, 1e-6, one, None) == EUNSUP
    assert L.nfx_lowrank_pack_radial(one, one, one, 8, -1, 1e-6, one, None) == EINVAL
    assert L.nfx_lowrank_pack_radial(one, one, one, 0, 50, 1e-6, one, None) == EINVAL
    assert L.nfx_lowrank_pack_sylvester(one, one, one, 8, 8, 9, 50, 1e-6, one, None) == EUNSUP
    assert b"num_transforms=9" in L.nfx_last_error()
    assert L.nfx_lowrank_pack_sylvester(one, one, one, 8, 8, 0, 50, 1e-6, one, None) == EINVAL
    assert L.nfx_lowrank_pack_sylvester(one, one, None, 8, 8, 8, 50, 1e-6, one, None) == EINVAL
