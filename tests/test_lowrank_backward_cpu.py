"""The references of the Planar / Radial / Sylvester fused backward, on the CPU: the hand-written sweep
and record-to-parameter adjoint (lowrank_backward_cases.recurrence_grads, what csrc/nfx_lowrank_bwd*
implement) against float64 autograd of the composite run to convergence, the composite's
forward-direction gradients against the reference's own (tests/golden/g23_lowrank.npz), the measured
distance between the unrolled and the converged gradient, and the host-side checks of the new C entry
points."""
import copy
import ctypes
import json

import pytest
import torch

from conftest import load_golden
import nfs_amd
from nfs_amd import _lib
from lowrank_cases import construct, make_inputs, make_layer, mixed_stack
from lowrank_backward_cases import (autograd_grads, converged, cotangents, gclose, names, recurrence_grads, references)

B = 65
# (kind, dim, num_householder, num_transforms)
LAYERS = ([("planar", d, 8, None) for d in (1, 3, 8, 17)] + [("radial", d, 8, None) for d in (1, 3, 8, 17)]
          + [("sylvester", 3, 8, 1), ("sylvester", 8, 8, 8), ("sylvester", 17, 4, 5), ("sylvester", 17, 17, 5)])


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("bound", [0.31, 0.6])
@pytest.mark.parametrize("kind,dim,nh,nt", LAYERS)
def test_recurrences_equal_converged_float64_autograd(kind, dim, nh, nt, bound, direction):
    """gx and every parameter to 1e-9 relative, every kind, both directions; num_householder = dim = 17
    runs the peeled Householder adjoint over 17 reflections. Prints (does not assert) how far the
    unrolled gradient at the layer's own max_iter = 50, tol = 1e-6 is from the converged one."""
    flow = make_layer(kind, dim, bound=bound, num_householder=nh, num_transforms=nt)
    x = make_inputs(B, dim, seed=31)
    gz, gld = cotangents(B, dim, seed=dim)
    ref = autograd_grads(converged(flow), x, gz, gld, direction)
    got = recurrence_grads(flow, x, gz, gld, direction)
    for name, a, b in zip(names(flow), got, ref):
        assert a.shape == b.shape and float(b.abs().max()) > 0, name
        assert _rel(a, b) <= 1e-9, (name, _rel(a, b))
    if direction < 0:
        own = autograd_grads(_own_settings(flow).double(), x, gz, gld, -1)
        worst = max((_rel(a, b), n) for n, a, b in zip(names(flow), own, ref))
        print(f"[lowrank bwd] {kind} dim={dim} nh={nh} nt={nt} bound={bound}: unrolled (50 steps, tol 1e-6) vs "
              f"converged, worst max|d|/max|grad| = {worst[0]:.3e} ({worst[1]})")


def _own_settings(flow):
    """A copy that keeps the layer's own max_iter and tol."""
    return copy.deepcopy(flow)


def test_mixed_stack_inverse():
    """Planar, Radial, Sylvester, Planar, Radial swept first to last from the stack's output alone."""
    flows = mixed_stack(3)
    x = make_inputs(B, 3, seed=32)
    gz, gld = cotangents(B, 3, seed=5)
    ref = autograd_grads([converged(f) for f in flows], x, gz, gld, -1)
    got = recurrence_grads(flows, x, gz, gld, -1)
    for name, a, b in zip(names(flows), got, ref):
        assert float(b.abs().max()) > 0 and _rel(a, b) <= 1e-9, (name, _rel(a, b))
    own = autograd_grads([_own_settings(f).double() for f in flows], x, gz, gld, -1)
    worst = max((_rel(a, b), n) for n, a, b in zip(names(flows), own, ref))
    print(f"[lowrank bwd] mixed_stack(3): unrolled vs converged, worst max|d|/max|grad| = {worst[0]:.3e} ({worst[1]})")


@pytest.fixture(scope="module")
def golden():
    arrs = load_golden("g23_lowrank.npz")
    return arrs, json.loads(bytes(arrs["meta"]).decode())


def golden_case(arrs, meta, i):
    """(flow, x, {name: the reference's gradient}) of configuration i of g23_lowrank.npz."""
    m = meta[i]
    nh = m["num_householder"] if m["num_householder"] is not None else 8
    flow = construct(m["kind"], m["dim"], num_householder=nh, num_transforms=m["num_transforms"])
    pre = f"c{i}.sd."
    flow.load_state_dict({k[len(pre):]: torch.from_numpy(v.copy()) for k, v in arrs.items() if k.startswith(pre)})
    pre = f"c{i}.grad."
    grads = {k[len(pre):]: torch.from_numpy(v.copy()) for k, v in arrs.items() if k.startswith(pre)}
    return flow.eval(), torch.from_numpy(arrs[f"c{i}.x"].copy()), grads


@pytest.mark.parametrize("i", range(11))
def test_float64_forward_gradients_match_the_reference(golden, i):
    """mean(0.5 |y|^2 - ld) through forward: the float64 composite and the hand-written sweep (with the
    objective's cotangents) against the reference's fp32 gradients, 2e-5 of max|ref| per tensor."""
    arrs, meta = golden
    flow, x, ref = golden_case(arrs, meta, i)
    f64 = converged(flow)
    xr = x.double().requires_grad_(True)
    y, ld = f64.forward(xr)
    (0.5 * (y * y).sum(dim=1) - ld).mean().backward()
    got = {"x": xr.grad, **{k: p.grad for k, p in f64.named_parameters()}}
    n = x.shape[0]
    by_hand = recurrence_grads(flow, x, y.detach() / n, torch.full((n,), -1.0 / n, dtype=torch.float64), 1)
    assert set(got) == set(ref)
    for (k, g), h in zip(got.items(), by_hand):
        scale = float(ref[k].abs().max())
        assert scale > 0 and float((g - ref[k].double()).abs().max()) <= 2e-5 * scale, k
        assert _rel(h, g) <= 1e-9, k


def test_gclose_uses_the_converged_composite():
    flow = make_layer("planar", 3)
    x = make_inputs(9, 3, seed=33)
    gz, gld = cotangents(9, 3)
    g64, g32 = references(flow, x, gz, gld, -1)
    assert all(a.dtype == torch.float64 for a in g64) and all(a.dtype == torch.float32 for a in g32)
    for name, a, b in zip(names(flow), g64, g32):
        gclose(b, a, name, b)
    with pytest.raises(AssertionError):
        gclose(g64[0] * 1.001, g64[0], "gx", g32[0])


# ---- the C entry points, on the host --------------------------------------------------------------
NEW_SYMBOLS = ("nfx_lrbwd_supported", "nfx_lrbwd_max_layers", "nfx_lrbwd_chunk_rows", "nfx_lrbwd_slots",
               "nfx_lrbwd_workspace_floats", "nfx_lrbwd_stack", "nfx_lrbwd_param_grads")


def test_switch_and_symbols():
    for cls in (nfs_amd.PlanarFlow, nfs_amd.RadialFlow, nfs_amd.SylvesterFlow):
        assert cls.fused_backward is False
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.checked(), name), name
    assert "nfx_lrbwd_supported" in _lib._VALUE_RETURNING and _lib.lib().nfx_abi_version() == 3


def test_family_budget_and_geometry():
    from nfs_amd.flows import lowrank
    L = _lib.lib()
    FWD, INV = _lib.NFX_FORWARD, _lib.NFX_INVERSE
    for dim in range(0, 70):
        inside = 1 <= dim <= 64
        cap = L.nfx_lrbwd_max_layers(dim)
        assert L.nfx_lrbwd_chunk_rows(dim) == (64 if inside else 0)
        if not inside:
            assert cap == 0 and L.nfx_lrbwd_supported(16, dim, 1, INV) == 0
            continue
        rec = L.nfx_lowrank_record_floats(dim)
        dp = (rec - 80) // 16
        stage = 4 * (2 * 64 * (dp + 1) + 64 * 17 + 64 * 65)
        # the gradient image of `cap` layers and one wave's staging fit 160 KiB, one more layer does not
        assert cap == lowrank.max_fused_backward_layers(dim) == min(256, (160 * 1024 - stage) // (4 * rec))
        assert cap >= 16
        assert L.nfx_lrbwd_supported(16, dim, cap, INV) == 1 and L.nfx_lrbwd_supported(16, dim, cap + 1, INV) == 0
        assert L.nfx_lrbwd_supported(16, dim, 1, FWD) == 1 and L.nfx_lrbwd_supported(16, dim, 2, FWD) == 0
        assert L.nfx_lrbwd_supported(0, dim, 1, INV) == 0 and L.nfx_lrbwd_supported(16, dim, 1, 0) == 0
    assert L.nfx_lrbwd_max_layers(64) == 24
    # slots: a workgroup per 64-row chunk up to the cap; the workspace is bounded whatever B
    cap = L.nfx_lrbwd_slots(1 << 40, 8, 4)
    assert cap == 1024 and L.nfx_lrbwd_slots(1, 8, 4) == 1 and L.nfx_lrbwd_slots(65, 8, 4) == 2
    assert L.nfx_lrbwd_slots(64 * cap + 1, 8, 4) == cap
    rec = L.nfx_lowrank_record_floats(8)
    assert L.nfx_lrbwd_workspace_floats(1 << 40, 8, 4) == (cap + 2) * 4 * rec
    assert L.nfx_lrbwd_workspace_floats(65, 8, 4) == (2 + 2) * 4 * rec
    assert L.nfx_lrbwd_workspace_floats(65, 65, 4) == 0 and L.nfx_lrbwd_slots(65, 8, 300) == 0


def test_invalid_arguments_fail_on_the_host():
    L = _lib.lib()
    EINVAL, EUNSUP = _lib.NFX_EINVAL, _lib.NFX_EUNSUPPORTED
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)
    assert L.nfx_lrbwd_stack(None, 1, None, None, None, None, None, 16, 8, 0, None) == EINVAL
    assert L.nfx_lrbwd_stack(None, 1, None, None, None, None, None, -1, 8, 1, None) == EINVAL
    assert L.nfx_lrbwd_stack(None, 1, None, None, None, None, None, 16, 65, 1, None) == EUNSUP
    assert L.nfx_lrbwd_stack(None, 2, None, None, None, None, None, 16, 8, 1, None) == EUNSUP  # a forward stack
    assert L.nfx_lrbwd_stack(None, 25, None, None, None, None, None, 16, 64, -1, None) == EUNSUP  # over the budget
    assert L.nfx_lrbwd_stack(None, 1, None, None, None, None, None, 16, 8, -1, None) == EINVAL  # null pointers
    assert L.nfx_lrbwd_stack(one, 1, two, one, one, two, one, 16, 8, -1, None) == EINVAL and b"alias" in L.nfx_last_error()
    assert L.nfx_lrbwd_stack(None, 1, None, None, None, None, None, 0, 8, -1, None) == 0  # B == 0 is a no-op
    assert L.nfx_lrbwd_param_grads(one, 16, 8, 4, 4, 0, one, one, one, None, None, None, 0, 0, None) == EINVAL
    assert L.nfx_lrbwd_param_grads(one, 16, 8, 4, 0, 3, one, one, one, None, None, None, 0, 0, None) == EINVAL
    assert L.nfx_lrbwd_param_grads(one, 16, 8, 4, 0, 2, one, one, one, None, None, None, 8, 9, None) == EUNSUP
    assert L.nfx_lrbwd_param_grads(None, 16, 8, 4, 0, 0, one, one, one, None, None, None, 0, 0, None) == EINVAL
