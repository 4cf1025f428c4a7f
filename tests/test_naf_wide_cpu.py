"""CPU: the host side of NeuralAutoregressiveFlow's wide kernel family (csrc/nfx_naf_wide*.hip): the
family and argument checks of the nfx_naf_wide_* entry points, which answer without a GPU, and the
`wide_kernel` switch on CPU tensors, where it changes nothing."""
import ctypes

import torch

import nfs_amd
from nfs_amd import _lib
from naf_cases import make_flow, make_inputs


def _widths(*w):
    return (ctypes.c_int * len(w))(*w)


INSIDE = [(2, [256]), (2, [129]), (16, [512, 512, 512]), (16, [512] * 4), (3, [160, 512]), (1, [1])]


def test_family_answers_on_the_host():
    L = _lib.lib()
    relu, gelu, ln = _lib.NFX_NAF_RELU, _lib.NFX_NAF_GELU, _lib.NFX_NAF_LAYER_NORM
    res = _lib.NFX_NAF_RESIDUAL
    for d, w in INSIDE:
        for act in (relu, _lib.NFX_NAF_ELU, _lib.NFX_NAF_LEAKY_RELU, gelu):
            for flags in (0, ln):
                assert L.nfx_naf_wide_supported(1, d, len(w), _widths(*w), act, flags) == 1, (d, w, act, flags)
        n = L.nfx_naf_wide_packed_floats(d, len(w), _widths(*w))
        assert n > 0 and n % 4 == 0, (d, w, n)
    assert L.nfx_naf_wide_supported(1 << 40, 16, 3, _widths(512, 512, 512), relu, ln | res(1) | res(2)) == 1
    outside = [(17, [256]), (0, [256]), (2, [513]), (2, [0]), (2, [256, 0]), (2, [8] * 5), (2, [])]
    for d, w in outside:
        assert L.nfx_naf_wide_supported(1, d, len(w), _widths(*w), relu, ln) == 0, (d, w)
        assert L.nfx_naf_wide_packed_floats(d, len(w), _widths(*w)) == 0, (d, w)
    w2 = _widths(256, 256)
    assert L.nfx_naf_wide_supported(1, 2, 2, w2, relu, ln | res(1)) == 1
    assert L.nfx_naf_wide_supported(1, 2, 2, w2, relu, res(0)) == 0                    # a residual flag on layer 0
    assert L.nfx_naf_wide_supported(1, 2, 2, w2, relu, res(2)) == 0                    # no such layer
    assert L.nfx_naf_wide_supported(1, 2, 2, _widths(256, 255), relu, res(1)) == 0     # unequal widths
    assert L.nfx_naf_wide_supported(1, 2, 2, w2, relu, 64) == 0                        # an unknown bit
    assert L.nfx_naf_wide_supported(1, 2, 2, None, relu, ln) == 0                      # null widths
    assert L.nfx_naf_wide_packed_floats(2, 2, None) == 0
    assert L.nfx_naf_wide_supported(0, 2, 2, w2, relu, ln) == 0                        # B = 0
    assert L.nfx_naf_wide_supported(-3, 2, 2, w2, relu, ln) == 0
    assert L.nfx_naf_wide_supported(1, 2, 2, w2, 4, ln) == 0 and L.nfx_naf_wide_supported(1, 2, 2, w2, -1, ln) == 0


def test_packed_floats_follow_the_padded_widths():
    L = _lib.lib()
    f = L.nfx_naf_wide_packed_floats
    assert f(2, 1, _widths(129)) == f(2, 1, _widths(160)) > f(2, 1, _widths(128)) > 0
    assert f(5, 3, _widths(512, 136, 512)) == f(5, 3, _widths(481, 160, 500))
    assert f(5, 2, _widths(160, 160)) < f(5, 2, _widths(161, 160))
    # the dims share one 16-slot input tile and one output tile: the image does not depend on d
    assert f(1, 1, _widths(300)) == f(16, 1, _widths(300))
    # inside both families the image is the narrow family's
    assert f(3, 2, _widths(32, 32)) == L.nfx_naf_packed_floats(3, 2, _widths(32, 32))
    # [512, 512, 512]: 2 x 512 x 512 hidden weights and the rest, about 2.1 MiB
    n = f(16, 3, _widths(512, 512, 512))
    assert 2 * 512 * 512 < n < 2 * 512 * 512 + 64 * 1024


def test_flow_and_pack_validate_on_the_host():
    L = _lib.lib()
    relu, ln, res = _lib.NFX_NAF_RELU, _lib.NFX_NAF_LAYER_NORM, _lib.NFX_NAF_RESIDUAL
    w3 = _widths(512, 512, 512)

    def flow(B=16, d=2, nh=3, w=w3, act=relu, flags=ln, direction=_lib.NFX_INVERSE):
        return L.nfx_naf_wide_flow(None, None, None, None, B, d, nh, w, act, flags, 3.0, 5.0, direction, 0, None)

    assert flow() == _lib.NFX_EINVAL and b"null" in L.nfx_last_error() and b"naf_wide" in L.nfx_last_error()
    assert flow(B=0) == 0
    assert flow(d=17) == _lib.NFX_EUNSUPPORTED and b"d=17" in L.nfx_last_error() and b"512" in L.nfx_last_error()
    assert flow(nh=1, w=_widths(513)) == _lib.NFX_EUNSUPPORTED
    assert flow(nh=5, w=_widths(8, 8, 8, 8, 8)) == _lib.NFX_EUNSUPPORTED
    assert flow(act=7) == _lib.NFX_EUNSUPPORTED
    assert flow(direction=0) == _lib.NFX_EINVAL and b"direction" in L.nfx_last_error()
    assert flow(B=-1) == _lib.NFX_EINVAL and flow(d=0) == _lib.NFX_EINVAL and flow(w=None) == _lib.NFX_EINVAL
    assert flow(flags=res(0)) == _lib.NFX_EINVAL and flow(flags=64) == _lib.NFX_EINVAL
    assert flow(nh=2, w=_widths(512, 136), flags=res(1)) == _lib.NFX_EINVAL
    assert flow(flags=ln | res(1) | res(2)) == _lib.NFX_EINVAL and b"null" in L.nfx_last_error()
    assert L.nfx_naf_wide_pack(None, 17, 3, w3, None, None) == _lib.NFX_EUNSUPPORTED
    assert L.nfx_naf_wide_pack(None, 2, 3, w3, None, None) == _lib.NFX_EINVAL and b"null" in L.nfx_last_error()
    assert L.nfx_naf_wide_pack(None, 0, 3, w3, None, None) == _lib.NFX_EINVAL
    assert L.nfx_naf_wide_pack(None, 2, 3, None, None, None) == _lib.NFX_EINVAL


def test_the_narrow_family_keeps_its_answers():
    L = _lib.lib()
    relu, ln = _lib.NFX_NAF_RELU, _lib.NFX_NAF_LAYER_NORM
    for d, w in ((2, [512, 512, 512]), (16, [512, 512, 512]), (2, [256]), (2, [129]), (16, [128] * 4)):
        assert L.nfx_naf_supported(1, d, len(w), _widths(*w), relu, ln) == 0, (d, w)
        assert L.nfx_naf_packed_floats(d, len(w), _widths(*w)) == 0, (d, w)
        assert L.nfx_naf_wide_supported(1, d, len(w), _widths(*w), relu, ln) == 1, (d, w)
    assert L.nfx_naf_flow(None, None, None, None, 16, 2, 1, _widths(256), relu, ln, 3.0, 5.0, _lib.NFX_INVERSE, 0,
                          None) == _lib.NFX_EUNSUPPORTED
    assert L.nfx_naf_pack(None, 2, 1, _widths(256), None, None) == _lib.NFX_EUNSUPPORTED


def test_switch_defaults_off_and_changes_nothing_on_the_cpu():
    assert nfs_amd.NeuralAutoregressiveFlow.wide_kernel is False
    flow = make_flow(3, (160, 160), "elu")
    x = make_inputs(21, 3, seed=51)
    with torch.no_grad():
        ref = flow.inverse(x) + flow.forward(x)
        flow.wide_kernel = True
        assert type(flow).wide_kernel is False  # (the instance's switch, not the class's)
        nfs_amd.reset_stats()
        got = flow.inverse(x) + flow.forward(x)
        assert nfs_amd.STATS == {"hip": 0, "torch": 2}
        got64 = flow.double().inverse(x.double())
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert got64[0].dtype == torch.float64 and float((got64[0] - ref[0]).abs().max()) < 1e-3


def test_reason_names_both_families_with_the_switch_on():
    flow = make_flow(17, (256,), "relu")
    x = torch.zeros(4, 17)
    ok, why = flow._hip_supported(x)
    assert not ok and "kernel family" in why and "wide" not in why
    flow.wide_kernel = True
    ok, why = flow._hip_supported(x)
    assert not ok and "kernel family" in why and "wide kernel family" in why and "1..512" in why and "1..128" in why
    inside = make_flow(2, (256,), "relu")
    assert not inside._hip_supported(torch.zeros(4, 2))[0]
    inside.wide_kernel = True
    assert inside._hip_supported(torch.zeros(4, 2)) == (True, "")
    assert inside._wide() and not make_flow(3, (32, 32), "relu")._wide()
    narrow = make_flow(3, (32, 32), "relu")
    narrow.wide_kernel = True
    assert narrow._hip_supported(torch.zeros(4, 3)) == (True, "") and not narrow._wide()
