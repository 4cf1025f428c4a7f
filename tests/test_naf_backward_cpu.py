"""NeuralAutoregressiveFlow's fused backward on the CPU: the reverse sweep the gfx950 kernel
implements, written out in float64 torch, against autograd on the composite; the host-only
behaviour of the backward's C entry points; and the switch."""
import ctypes

import pytest
import torch

import conftest  # noqa: F401  (sys.path)
import nfs_amd
from naf_backward_cases import (autograd_grads, away_from_kinks, cotangents, names, recurrence_grads, references,
                                trace)
from naf_cases import ACTIVATIONS, as_double, make_flow, make_inputs


def _compare(flow, x, seed):
    gz, gld = cotangents(x.shape[0], x.shape[1], seed=seed)
    gx, gp = recurrence_grads(flow, x, gz.double(), gld.double())
    rx, rp = autograd_grads(flow, x, gz, gld)
    for name, a, b in zip(names(flow), [gx] + gp, [rx] + rp):
        assert a.shape == b.shape, name
        scale = float(b.abs().max())
        if flow.dim == 1 and name not in ("gx", names(flow)[-1]):
            # the output rows of dimension 0 see no hidden unit: bias-only outputs, zero gradients below
            assert scale == 0.0 and float(a.abs().max()) == 0.0, name
            continue
        assert scale > 0, name
        assert float((a - b).abs().max()) <= 1e-10 * scale, name


@pytest.mark.parametrize("act", ACTIVATIONS)
@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("d,hidden", [(1, (32,)), (2, (8, 8)), (5, (33, 64, 20)), (16, (40, 40, 40))])
def test_reverse_sweep_equals_float64_autograd(act, ln, res, d, hidden):
    """Differentiating the density direction by hand gives autograd's gradients of `_torch_call` to
    rounding: 1e-10 relative per gradient."""
    flow = as_double(make_flow(d, hidden, act, ln, res))
    _compare(flow, make_inputs(37, d, seed=11).double(), d + len(hidden))


@pytest.mark.parametrize("act", ACTIVATIONS)
def test_reverse_sweep_with_both_clamps_reached(act):
    flow = as_double(make_flow(4, (40, 40), act, True, True, clamp_alpha=1.5, clamp_log_scale=1.0))
    x = make_inputs(200, 4, seed=13).double()
    t = trace(flow, x)
    assert bool((t["alpha"].abs() > 1.5).any()) and bool((t["alpha"].abs() < 1.5).any())
    assert bool((t["nls"].abs() > 1.0).any()) and bool((t["nls"].abs() < 1.0).any())
    _compare(flow, x, 3)


@pytest.mark.parametrize("act", ACTIVATIONS)
def test_away_from_kinks_drops_few_rows(act):
    """The shares the GPU parity cases lose at 4,099 rows stay under the cap (the function asserts it)."""
    for d, hidden in [(2, (8, 8)), (16, (64, 64, 64, 64))]:
        flow = make_flow(d, hidden, act)
        x = make_inputs(4099, d, seed=3)
        kept = away_from_kinks(flow, x)
        assert 0.95 * 4099 <= kept.shape[0] <= 4099
    assert references  # (shared with the GPU file)


def _widths(*w):
    arr = (ctypes.c_int * len(w))(*w)
    return arr, ctypes.addressof(arr)


def test_c_abi_validates_on_the_host():
    """Family, sizes and argument checks of the backward's entry points answer without a GPU."""
    from nfs_amd import _lib
    L = _lib.lib()
    for name in ("nfx_naf_backward_supported", "nfx_naf_backward_packed_floats", "nfx_naf_pack_backward",
                 "nfx_naf_backward_slots", "nfx_naf_backward_block_threads", "nfx_naf_backward_workspace_floats",
                 "nfx_naf_backward"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS, name
    LN = _lib.NFX_NAF_LAYER_NORM

    def supported(B, d, widths, act=0, flags=0):
        keep, p = _widths(*widths)
        return L.nfx_naf_backward_supported(B, d, len(widths), p, act, flags)

    # the required family: every dim, 1 to 4 layers, widths 1..64, every activation, LayerNorm, residuals
    for d in (1, 2, 9, 16):
        for widths in ((1,), (32,), (64,), (33, 64, 20), (64, 64, 64), (64, 64, 64, 64), (8, 8, 8, 8)):
            for act in range(4):
                assert supported(1, d, widths, act, 0) == 1 and supported(1 << 36, d, widths, act, LN) == 1
    assert supported(70, 16, (64, 64, 64), 0, LN | _lib.NFX_NAF_RESIDUAL(1) | _lib.NFX_NAF_RESIDUAL(2)) == 1
    assert supported(70, 16, (64,) * 4, 0, LN | sum(_lib.NFX_NAF_RESIDUAL(l) for l in (1, 2, 3))) == 1
    for w in (65, 96, 128):
        assert supported(1, 4, (w, w)) == 0 and supported(1, 4, (32, w)) == 0
        assert L.nfx_naf_supported(1, 4, 2, _widths(w, w)[1], 0, 0) == 1  # (the forward has them)
    assert supported(1, 17, (32,)) == 0 and supported(1, 0, (32,)) == 0
    assert supported(1, 4, (32,) * 5) == 0 and supported(1, 4, ()) == 0
    assert supported(1, 4, (32,), act=4) == 0 and supported(1, 4, (32,), act=-1) == 0
    assert supported(0, 4, (32,)) == 0
    assert supported(1, 4, (32, 40), flags=_lib.NFX_NAF_RESIDUAL(1)) == 0  # unequal widths

    # sizes: positive inside the family, 0 outside
    for d, widths in ((1, (32,)), (4, (64, 64)), (16, (64, 64, 64, 64))):
        keep, p = _widths(*widths)
        n = len(widths)
        packed = L.nfx_naf_backward_packed_floats(d, n, p)
        assert packed > L.nfx_naf_packed_floats(d, n, p) and packed % 4 == 0
        # the image and four transposition tiles fit the 160 KiB of one workgroup
        assert 4 * (packed + 4 * 32 * 33) <= 160 * 1024
        assert L.nfx_naf_backward_slots(1, d, n, p) == 1 and L.nfx_naf_backward_slots(33, d, n, p) == 2
        cap = L.nfx_naf_backward_slots(1 << 30, d, n, p)
        assert cap % 4 == 0 and L.nfx_naf_backward_slots(1 << 31, d, n, p) == cap
        assert L.nfx_naf_backward_block_threads(33, d, n, p) == 64
        assert L.nfx_naf_backward_block_threads(1 << 30, d, n, p) == 256
        ws = L.nfx_naf_backward_workspace_floats(33, d, n, p)
        n_params = sum(a * b for a, b in zip(widths + (2 * d,), (d,) + widths))
        assert ws >= 2 * n_params + 2 * n_params
        assert L.nfx_naf_backward_workspace_floats(1 << 31, d, n, p) == L.nfx_naf_backward_workspace_floats(1 << 30, d, n, p)
    keep, wide = _widths(128, 128)
    keep2, ok = _widths(64, 64)
    assert L.nfx_naf_backward_packed_floats(4, 2, wide) == 0 and L.nfx_naf_backward_packed_floats(17, 2, ok) == 0
    assert L.nfx_naf_backward_slots(33, 4, 2, wide) == 0 and L.nfx_naf_backward_block_threads(33, 17, 2, ok) == 0
    assert L.nfx_naf_backward_workspace_floats(33, 4, 2, wide) == 0
    assert L.nfx_naf_backward_workspace_floats(0, 4, 2, ok) == 0

    # argument checks
    E, U = _lib.NFX_EINVAL, _lib.NFX_EUNSUPPORTED
    assert L.nfx_naf_pack_backward(None, 4, 2, wide, None, None) == U and b"naf backward" in L.nfx_last_error()
    assert L.nfx_naf_pack_backward(None, 17, 2, ok, None, None) == U
    assert L.nfx_naf_pack_backward(None, 0, 2, ok, None, None) == E
    assert L.nfx_naf_pack_backward(None, 4, 2, None, None, None) == E
    assert L.nfx_naf_pack_backward(None, 4, 2, ok, None, None) == E and b"null" in L.nfx_last_error()

    def bwd(B, d, n, widths, act=0, flags=0, ptrs=(None,) * 8):
        return L.nfx_naf_backward(*ptrs, B, d, n, widths, act, flags, 3.0, 5.0, None)
    assert bwd(16, 4, 2, wide) == U and b"naf backward" in L.nfx_last_error()
    assert bwd(16, 17, 2, ok) == U and bwd(16, 4, 5, ok) == U
    assert bwd(16, 4, 2, ok, act=7) == U
    assert bwd(-1, 4, 2, ok) == E and bwd(16, 0, 2, ok) == E and bwd(16, 4, 2, None) == E
    assert bwd(16, 4, 2, ok, flags=64) == E
    assert bwd(16, 4, 2, ok) == E and b"null" in L.nfx_last_error()
    assert bwd(0, 4, 2, ok) == 0
    # gx aliasing x, and gx aliasing gz (host memory: the checks come before any launch)
    buf = (ctypes.c_float * 64)()
    a, b, c = ctypes.addressof(buf), ctypes.addressof(buf) + 64, ctypes.addressof(buf) + 128
    layers = (_lib.NfxNafLayer * 3)()
    grads = (_lib.NfxNafLayerGrad * 3)()
    la, ga = ctypes.addressof(layers), ctypes.addressof(grads)
    assert bwd(16, 4, 2, ok, ptrs=(a, la, b, c, a, b, ga, a)) == E and b"alias" in L.nfx_last_error()
    assert bwd(16, 4, 2, ok, ptrs=(a, la, b, c, a, c, ga, a)) == E and b"alias" in L.nfx_last_error()
    # distinct buffers pass the aliasing checks and stop at the layers' null weights
    assert bwd(16, 4, 2, ok, ptrs=(a, la, b, c, a, a + 16, ga, a)) == E and b"weight or bias" in L.nfx_last_error()


def test_flag_defaults_to_off():
    assert nfs_amd.NeuralAutoregressiveFlow.fused_backward is False
    assert make_flow(2, (8, 8)).fused_backward is False


def test_flag_on_keeps_the_composite_on_the_cpu():
    """CPU tensors take the composite whatever the flag says: the same gradients, bit for bit."""
    d, hidden = 3, (16, 16)
    x = make_inputs(21, d, seed=17)
    gz, gld = cotangents(21, d, seed=1)

    def grads(flow):
        flow.zero_grad(set_to_none=True)
        xr = x.clone().requires_grad_(True)
        nfs_amd.reset_stats()
        z, ld = flow.inverse(xr)
        torch.autograd.backward([z, ld], [gz, gld])
        assert nfs_amd.STATS == {"hip": 0, "torch": 1}
        return [xr.grad] + [p.grad for p in flow.parameters()]

    plain = grads(make_flow(d, hidden))
    on = make_flow(d, hidden)
    on.fused_backward = True
    for a, b in zip(grads(on), plain):
        assert torch.equal(a, b)
    ref, _ = autograd_grads(make_flow(d, hidden), x, gz, gld)
    assert torch.equal(plain[0], ref)
