"""ResidualFlow's fused backward on the CPU: the recurrences the gfx950 kernel implements, written
out in float64 torch, against autograd on the converged composite; the switch; and the host-only
behaviour of the backward's C entry points."""
import pytest
import torch

import conftest  # noqa: F401  (sys.path)
import nfs_amd
from residual_backward_cases import NAMES, autograd_grads, converged, cotangents, recurrence_grads
from residual_cases import ACTIVATIONS, as_double, make_flow, make_inputs, sigmas

SHAPES = [(2, 64), (8, 64), (5, 20), (3, 33), (1, 7), (4, 64)]
# Every shape with every activation; lipschitz_constant, neumann_terms and the weight scale cycle
# over the cases so that each value meets each activation and each shape.
CASES = [(d, H, act, (0.9, 1.8)[(k + a) % 2], 1 + (2 * k + a) % 5, (1.0, 0.1)[((k + a) // 2) % 2])
         for k, (d, H) in enumerate(SHAPES) for a, act in enumerate(ACTIVATIONS)]


def test_the_case_list_covers_every_setting():
    assert {c[3] for c in CASES} == {0.9, 1.8} and {c[4] for c in CASES} == {1, 2, 3, 4, 5}
    assert {c[5] for c in CASES} == {1.0, 0.1}
    for act in ACTIVATIONS:
        assert {c[3] for c in CASES if c[2] == act} == {0.9, 1.8}
        assert {c[5] for c in CASES if c[2] == act} == {1.0, 0.1}


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("d,H,act,lipschitz,nterms,scale", CASES)
def test_recurrences_equal_autograd_of_the_converged_composite(d, H, act, lipschitz, nterms, scale, direction):
    """1e-10 of max|grad| per gradient (about 1e-15 measured). The gap to the gradient unrolled at
    the layer's own max_iter = 100, tol = 1e-6 is printed: it is what the implicit gradient of the
    fused route differs by from the composite route's."""
    B = 70
    flow = make_flow(d, H, act, lipschitz, seed=3, weight_scale=scale, neumann_terms=nterms)
    engaged = [s > c for s, c in sigmas(flow)]
    assert all(engaged) if scale == 1.0 else not any(engaged), (engaged, sigmas(flow))
    x = make_inputs(B, d, seed=11 + d)
    gy, gld = cotangents(B, d, seed=d + H)
    conv = converged(flow, torch.float64, x)
    gx, gp = recurrence_grads(conv, x, direction, gy, gld)
    rx, rp = autograd_grads(conv, x, direction, gy, gld)
    ux, up = autograd_grads(as_double(flow), x, direction, gy, gld)
    gap = 0.0
    for name, a, b, u in zip(NAMES, [gx] + gp, [rx] + rp, [ux] + up):
        scale_ = float(b.abs().max())
        assert scale_ > 0, name
        assert float((a - b).abs().max()) <= 1e-10 * scale_, (name, float((a - b).abs().max()), scale_)
        gap = max(gap, float((u - b).abs().max()) / scale_)
    print(f"[residual bwd] d={d} H={H} {act} L={lipschitz} n={nterms} scale={scale} dir={direction}: "
          f"converged vs unrolled at max_iter=100, tol=1e-6: {gap:.2e} of max|grad|")


def test_the_switch_is_off_by_default_and_a_cpu_call_runs_the_composite():
    assert nfs_amd.ResidualFlow.fused_backward is False
    flow = make_flow(2, 64)
    flow.fused_backward = True
    x = make_inputs(9, 2).requires_grad_(True)
    nfs_amd.reset_stats()
    z, ld = flow.inverse(x)
    (z.sum() + ld.sum()).backward()
    assert nfs_amd.STATS == {"hip": 0, "torch": 1}
    assert x.grad is not None and all(p.grad is not None for p in flow.parameters())
    assert hasattr(flow, "_hip_backward") and hasattr(flow, "_build_backward_pack")
    assert nfs_amd.ResidualFlow.fused_backward is False  # the instance's switch is its own


def test_backward_family_is_exactly_dim_1_to_8_and_hidden_1_to_64():
    """Host-only: launches nothing."""
    from nfs_amd import _lib
    L = _lib.lib()
    for act in range(4):
        for d in range(1, 33):
            for H in range(1, 257):
                assert L.nfx_residual_backward_supported(1, d, H, act) == (1 if d <= 8 and H <= 64 else 0), (d, H, act)
    assert L.nfx_residual_backward_supported(1, 2, 64, 4) == 0 and L.nfx_residual_backward_supported(1, 2, 64, -1) == 0
    assert L.nfx_residual_backward_supported(0, 2, 64, 0) == 0 and L.nfx_residual_backward_supported(1, 0, 64, 0) == 0
    assert L.nfx_residual_backward_supported(1 << 36, 8, 64, 3) == 1


def test_backward_image_size_is_constant_per_cell_and_zero_outside():
    from nfs_amd import _lib
    L = _lib.lib()
    for d in range(1, 10):
        for lo, hi in ((1, 32), (33, 64)):
            sizes = {L.nfx_residual_backward_packed_floats(d, H) for H in range(lo, hi + 1)}
            if d > 8:
                assert sizes == {0}
                continue
            assert len(sizes) == 1
            n = sizes.pop()
            # the forward image, then the transposed H x H operand
            assert n == L.nfx_residual_packed_floats(d, hi) + hi * hi and n % 4 == 0
        assert L.nfx_residual_backward_packed_floats(d, 65) == 0 and L.nfx_residual_backward_packed_floats(d, 128) == 0
    assert L.nfx_residual_backward_packed_floats(0, 32) == 0


def test_c_abi_validates_on_the_host():
    from nfs_amd import _lib
    L = _lib.lib()
    # one wave per 32-row tile up to the slot cap; 64 threads per workgroup for few tiles, 256 beyond
    assert L.nfx_residual_backward_slots(1, 2, 64) == 1 and L.nfx_residual_backward_slots(33, 2, 64) == 2
    cap = L.nfx_residual_backward_slots(1 << 30, 2, 64)
    assert cap % 4 == 0 and L.nfx_residual_backward_slots(1 << 31, 2, 64) == cap
    assert L.nfx_residual_backward_block_threads(33, 2, 64) == 64
    assert L.nfx_residual_backward_block_threads(1 << 30, 2, 64) == 256
    assert L.nfx_residual_backward_slots(33, 2, 128) == 0 and L.nfx_residual_backward_block_threads(33, 9, 64) == 0
    w = L.nfx_residual_backward_workspace_floats(33, 2, 64)
    assert w >= 2 * (64 * 64 + 2 * 64 * 2 + 2 * 64 + 2) and L.nfx_residual_backward_workspace_floats(33, 2, 128) == 0
    assert (L.nfx_residual_backward_workspace_floats(1 << 31, 2, 64)
            == L.nfx_residual_backward_workspace_floats(1 << 30, 2, 64))

    E, U = _lib.NFX_EINVAL, _lib.NFX_EUNSUPPORTED
    raw = (None, None, None, None, 0.45) * 3
    assert L.nfx_residual_pack_backward(*raw, 2, 128, None, None) == U and b"H=128" in L.nfx_last_error()
    assert L.nfx_residual_pack_backward(*raw, 9, 64, None, None) == U
    assert L.nfx_residual_pack_backward(*raw, 0, 64, None, None) == E
    assert L.nfx_residual_pack_backward(*raw, 2, 64, None, None) == E and b"null" in L.nfx_last_error()

    def bwd(B, d, H, act=0, direction=_lib.NFX_INVERSE, nterms=3):
        return L.nfx_residual_backward(*(None,) * 12, B, d, H, act, direction, nterms, None)
    assert bwd(16, 2, 128) == U and b"H=128" in L.nfx_last_error()
    assert bwd(16, 9, 64) == U and bwd(16, 2, 64, act=7) == U
    assert bwd(-1, 2, 64) == E and bwd(16, 0, 64) == E and bwd(16, 2, 64, nterms=-1) == E
    assert bwd(16, 2, 64, direction=5) == E
    assert bwd(16, 2, 64) == E and b"null" in L.nfx_last_error()
    assert bwd(0, 2, 64) == 0
