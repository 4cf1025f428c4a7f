"""ResidualFlow on the CPU: the torch composite (nfs_amd/flows/residual.py, which the gfx950 kernel
is tested against in test_gpu_residual.py) against the reference's own results
(tests/golden/g21_residual.npz, written by tests/golden/make_golden_residual.py), against a float64
closed form, and the host-side checks of the C entry points."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
import nfs_amd
from residual_cases import ACTIVATIONS, as_double, composite, make_flow, make_inputs, sigmas


@pytest.fixture(scope="module")
def golden():
    arrs = load_golden("g21_residual.npz")
    return arrs, json.loads(bytes(arrs["meta"]).decode())


def _flow(arrs, meta, i):
    m = meta[i]
    flow = nfs_amd.ResidualFlow(m["dim"], m["hidden_dim"], activation=m["activation"])
    p = f"c{i}.sd."
    flow.load_state_dict({k[len(p):]: torch.from_numpy(v.copy()) for k, v in arrs.items() if k.startswith(p)})
    return flow.eval()


def _t(arrs, key):
    return torch.from_numpy(arrs[key].copy())


N_CONFIGS = 6


def test_fixture_covers_both_regimes_and_every_activation(golden):
    arrs, meta = golden
    assert len(meta) == N_CONFIGS
    assert {m["activation"] for m in meta} == set(ACTIVATIONS)
    assert {m["engaged"] for m in meta} == {True, False}
    assert {m["dim"] for m in meta} == {2, 3, 4} and {m["hidden_dim"] for m in meta} == {8, 16}
    for i, m in enumerate(meta):
        for (s, c), (s64, _) in zip(m["sigma_c"], sigmas(_flow(arrs, meta, i))):
            assert (s > c) == m["engaged"] and abs(s - c) > 1e-3 * c
            assert abs(s - s64) <= 1e-5 * c  # the package reads the same sigma out of the state dict


@pytest.mark.parametrize("i", range(N_CONFIGS))
def test_outputs_match_the_reference(golden, i):
    """forward and inverse against the reference's fp32 results: 1e-6 (1 + |ref|) for x and z, 1e-6
    absolute for the log-det. (The inverse stops per sample where the reference stops per batch: a row
    may keep an iterate a step or more earlier than the reference's, both within tol of each other.)"""
    arrs, meta = golden
    flow, x = _flow(arrs, meta, i), _t(arrs, f"c{i}.x")
    for direction, tag, out in ((1, "fwd", "y"), (-1, "inv", "z")):
        y, ld = composite(flow, x, direction)
        yr, ldr = _t(arrs, f"c{i}.{tag}.{out}"), _t(arrs, f"c{i}.{tag}.ld")
        ey = float(((y - yr).abs() / (1 + yr.abs())).max())
        el = float((ld - ldr).abs().max())
        print(f"[residual c{i} {tag}] x/z {ey:.3e} log-det {el:.3e} (max |log-det| {float(ldr.abs().max()):.3e})")
        assert ey <= 1e-6 and el <= 1e-6
        assert float(ldr.abs().max()) > 1e-4


def _nll_grads(flow, x):
    flow.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    z, ld = flow.inverse(xr)
    (0.5 * (z * z).sum(dim=1) - ld).mean().backward()
    return {"x": xr.grad, **{k: p.grad for k, p in flow.named_parameters()}}


@pytest.mark.parametrize("i", range(N_CONFIGS))
def test_gradients_match_the_reference(golden, i):
    """Gradients of mean(0.5 |z|^2 - ld) through the inverse, with respect to x and every
    parameter, within 2e-5 of max|ref| per tensor, in both regimes: the Jacobian of the effective
    weights and straight-through parameter gradients. The fixture takes them at tol = 0 and
    max_iter = 8, where every row runs every iteration, so that the per-sample stopping rule and the
    reference's batch-global one unroll the same graph (at the default tol a row that stops an
    iteration earlier differentiates one iteration fewer, a relative difference of the order of
    the contraction factor to the power of the iteration count, about tol / |f|)."""
    arrs, meta = golden
    flow, x = _flow(arrs, meta, i), _t(arrs, f"c{i}.x")
    flow.tol, flow.max_iter = 0.0, meta[i]["grad_iters"]
    grads = _nll_grads(flow, x)
    assert len(grads) == 7
    for k, g in grads.items():
        ref = _t(arrs, f"c{i}.grad.{k}")
        err, scale = float((g - ref).abs().max()), float(ref.abs().max())
        print(f"[residual c{i} grad] {k}: {err:.3e} of {scale:.3e}")
        assert scale > 0 and err <= 2e-5 * scale, k


@pytest.mark.parametrize("i", range(N_CONFIGS))
def test_train_mode_advances_u_and_v_as_the_reference(golden, i, monkeypatch):
    """One train-mode forward makes 1 + dim SpectralNorm calls per layer, one train-mode inverse one
    per iteration and dim more; after each the buffers equal the reference's."""
    arrs, meta = golden
    x = _t(arrs, f"c{i}.x")
    for name, tag in (("forward", "train_fwd"), ("inverse", "train_inv")):
        flow = _flow(arrs, meta, i).train()
        with torch.no_grad():
            getattr(flow, name)(x)
        uv = torch.cat([v for k, v in flow.state_dict().items() if k.endswith((".u", ".v"))])
        assert float((uv - _t(arrs, f"c{i}.{tag}.uv")).abs().max()) <= 1e-6
    # the call count itself: three layers, 1 + dim calls each
    flow = _flow(arrs, meta, i).train()
    orig = nfs_amd.SpectralNorm.effective_weight
    count = [0]

    def counting(self, dtype=None):
        count[0] += 1
        return orig(self, dtype)

    monkeypatch.setattr(nfs_amd.SpectralNorm, "effective_weight", counting)
    with torch.no_grad():
        flow.forward(x)
    assert count[0] == 3 * (1 + meta[i]["dim"])


def test_eval_mode_leaves_the_buffers_alone(golden):
    arrs, meta = golden
    flow, x = _flow(arrs, meta, 0), _t(arrs, "c0.x")
    before = {k: v.clone() for k, v in flow.state_dict().items()}
    composite(flow, x, 1)
    composite(flow, x, -1)
    assert all(torch.equal(before[k], v) for k, v in flow.state_dict().items())


@pytest.mark.parametrize("i", [0, 1])
def test_seeded_construction_is_the_reference_bit_for_bit(golden, i):
    arrs, meta = golden
    m = meta[i]
    torch.manual_seed(m["seed"])
    flow = nfs_amd.ResidualFlow(m["dim"], hidden_dim=m["hidden_dim"], activation=m["activation"])
    sd = flow.state_dict()
    p = f"c{i}.init."
    assert list(sd) == [f"residual_block.layer{l}.{k}" for l in (1, 2, 3) for k in ("u", "v", "module.weight", "module.bias")]
    assert sorted(sd) == sorted(k[len(p):] for k in arrs if k.startswith(p))
    for k, v in sd.items():
        assert torch.equal(v, _t(arrs, p + k)), k


def test_drop_in_surface():
    flow = nfs_amd.ResidualFlow(3)
    assert isinstance(flow, nfs_amd.flows.HipFlow) and nfs_amd.flows.ResidualFlow is nfs_amd.ResidualFlow
    assert isinstance(flow.residual_block, nfs_amd.ResidualBlock)
    assert isinstance(flow.residual_block.layer1, nfs_amd.SpectralNorm)
    assert (flow.dim, flow.data_dim, flow.hidden_dim, flow.lipschitz_constant, flow.max_iter, flow.tol,
            flow.neumann_terms) == (3, 3, 64, 0.9, 100, 1e-6, 3)
    block = flow.residual_block
    assert (block.dim, block.hidden_dim, block.lipschitz_constant) == (3, 64, 0.9)
    assert [l.lipschitz_constant for l in block.layers()] == [0.45] * 3
    assert [l.n_power_iterations for l in block.layers()] == [1] * 3
    assert block.layer1.module.weight.shape == (64, 3) and block.layer3.module.weight.shape == (3, 64)
    with pytest.raises(ValueError):
        nfs_amd.ResidualFlow(2, activation="gelu")
    assert flow._torch_only() is True and flow.eval()._torch_only() is False


@pytest.mark.parametrize("act", ACTIVATIONS)
@pytest.mark.parametrize("lipschitz", [0.9, 1.8])
def test_round_trip(act, lipschitz):
    """inverse(forward(z)) returns z within a few tol / (1 - L), and the log-dets cancel to the same
    order (both are the Neumann sum at the same point up to that distance)."""
    flow = make_flow(3, 16, act, lipschitz)
    z = make_inputs(40, 3, seed=2)
    x, lf = composite(flow, z, 1)
    zb, li = composite(flow, x, -1)
    assert float((x - z).abs().max()) > 1e-3
    assert float((zb - z).abs().max()) <= 8e-6
    assert float((lf + li).abs().max()) <= 8e-6
    # under torch.no_grad() above; the same values, to fp32 rounding, with grad mode on
    x2, lf2 = flow.forward(z)
    assert lf2.requires_grad and torch.equal(x2.detach(), x) and float((lf2.detach() - lf).abs().max()) <= 1e-7


def _closed_form_neumann(flow, z, n):
    """The Neumann sum of W3 D2 W2 D1 W1 per row, in numpy float64, written independently of the
    package: effective weights from one power iteration, masks from the pre-activations."""
    ws = []
    for layer in flow.residual_block.layers():
        w, u = layer.module.weight.detach().double().numpy(), layer.u.double().numpy()
        b = layer.module.bias.detach().double().numpy()
        v = w.T @ u
        v = v / max(np.linalg.norm(v), 1e-12)
        u = w @ v
        u = u / max(np.linalg.norm(u), 1e-12)
        s = u @ (w @ v)
        ws.append((w * (layer.lipschitz_constant / s) if s > layer.lipschitz_constant else w, b))
    name = type(flow.residual_block.activation).__name__
    act = {"ReLU": lambda a: np.maximum(a, 0), "ELU": lambda a: np.where(a > 0, a, np.expm1(a)),
           "LeakyReLU": lambda a: np.where(a > 0, a, 0.1 * a), "Tanh": np.tanh}[name]
    der = {"ReLU": lambda a: (a > 0) * 1.0, "ELU": lambda a: np.where(a > 0, 1.0, np.exp(a)),
           "LeakyReLU": lambda a: np.where(a > 0, 1.0, 0.1), "Tanh": lambda a: 1 - np.tanh(a) ** 2}[name]
    (w1, b1), (w2, b2), (w3, _) = ws
    out = []
    for row in z.double().numpy():
        a1 = w1 @ row + b1
        a2 = w2 @ act(a1) + b2
        jac = (w3 * der(a2)) @ (w2 * der(a1)) @ w1
        p, s = np.eye(len(row)), 0.0
        for k in range(1, n + 1):
            p = p @ jac
            s += (-1) ** (k + 1) * np.trace(p) / k
        out.append(s)
    return np.array(out)


@pytest.mark.parametrize("act", ACTIVATIONS)
@pytest.mark.parametrize("n", [1, 3, 5])
def test_float64_log_det_is_the_neumann_sum_of_the_closed_form_jacobian(act, n):
    """lipschitz_constant = 1.8: the second and third Neumann terms are large enough for a mistake
    in them to show (asserted)."""
    flow = as_double(make_flow(4, 16, act, 1.8, neumann_terms=n))
    z = make_inputs(12, 4, seed=6).double()
    _, ld = composite(flow, z, 1)
    ref = _closed_form_neumann(flow, z, n)
    assert np.abs(ld.numpy() - ref).max() <= 1e-10
    if n > 1:
        first = _closed_form_neumann(flow, z, 1)
        assert np.abs(ref - first).max() > 1e-4
    if n > 3:
        assert np.abs(ref - _closed_form_neumann(flow, z, 3)).max() > 1e-7
    _, li = composite(flow, z, -1)
    assert float(li.abs().max()) > 1e-3


def test_c_abi_validates_on_the_host():
    """The kernel family and argument checks of the C entry points answer without a GPU."""
    from nfs_amd import _lib
    L = _lib.lib()
    relu, tanh = _lib.NFX_RESIDUAL_RELU, _lib.NFX_RESIDUAL_TANH
    assert L.nfx_residual_supported(1, 2, 64, relu) == 1 and L.nfx_residual_supported(1 << 40, 8, 128, tanh) == 1
    assert L.nfx_residual_supported(1, 1, 1, relu) == 1 and L.nfx_residual_supported(1, 4, 48, tanh) == 1
    assert L.nfx_residual_supported(1, 9, 64, relu) == 0 and L.nfx_residual_supported(1, 2, 130, relu) == 0
    assert L.nfx_residual_supported(0, 2, 64, relu) == 0 and L.nfx_residual_supported(1, 0, 64, relu) == 0
    assert L.nfx_residual_supported(1, 2, 64, 4) == 0 and L.nfx_residual_supported(1, 2, 64, -1) == 0
    n = L.nfx_residual_packed_floats(2, 64)
    assert n >= 64 * 64 + 2 * 64 * 3 + 64 + 64 + 2 and n % 4 == 0
    assert L.nfx_residual_packed_floats(2, 48) == n  # padded to the same width
    assert L.nfx_residual_packed_floats(9, 64) == 0 and L.nfx_residual_packed_floats(2, 130) == 0
    args = (relu, _lib.NFX_INVERSE, 3, 100, 1e-6, 0, None)
    assert L.nfx_residual_flow(None, None, None, None, 16, 9, 64, *args) == _lib.NFX_EUNSUPPORTED
    assert b"d=9" in L.nfx_last_error()
    assert L.nfx_residual_flow(None, None, None, None, 16, 2, 130, *args) == _lib.NFX_EUNSUPPORTED
    assert L.nfx_residual_flow(None, None, None, None, 16, 2, 64, 7, _lib.NFX_INVERSE, 3, 100, 1e-6, 0,
                               None) == _lib.NFX_EUNSUPPORTED
    assert L.nfx_residual_flow(None, None, None, None, 16, 2, 64, relu, 0, 3, 100, 1e-6, 0, None) == _lib.NFX_EINVAL
    assert b"direction" in L.nfx_last_error()
    assert L.nfx_residual_flow(None, None, None, None, 16, 2, 64, relu, 1, -1, 100, 1e-6, 0, None) == _lib.NFX_EINVAL
    assert L.nfx_residual_flow(None, None, None, None, 16, 2, 64, relu, 1, 3, -1, 1e-6, 0, None) == _lib.NFX_EINVAL
    assert L.nfx_residual_flow(None, None, None, None, -1, 2, 64, *args) == _lib.NFX_EINVAL
    assert L.nfx_residual_flow(None, None, None, None, 16, 2, 64, *args) == _lib.NFX_EINVAL
    assert b"null" in L.nfx_last_error()
    assert L.nfx_residual_flow(None, None, None, None, 0, 2, 64, *args) == 0
    none5 = (None, None, None, None, 0.45)
    assert L.nfx_residual_pack(*none5, *none5, *none5, 9, 64, None, None) == _lib.NFX_EUNSUPPORTED
    assert L.nfx_residual_pack(*none5, *none5, *none5, 2, 64, None, None) == _lib.NFX_EINVAL
    assert L.nfx_residual_pack(*none5, *none5, *none5, 0, 64, None, None) == _lib.NFX_EINVAL
