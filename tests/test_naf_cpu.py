"""NeuralAutoregressiveFlow on the CPU: the torch composite (nfs_amd/flows/naf.py, which the gfx950
kernel is tested against in test_gpu_naf.py) against the reference's own results
(tests/golden/g22_naf.npz, written by tests/golden/make_golden_naf.py), the reference's quirks pinned,
and the host-side checks of the C entry points."""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
import nfs_amd
from nfs_amd import _lib
from nfs_amd.flows import naf as naf_mod
from naf_cases import ACTIVATIONS, composite, make_flow, make_inputs

N_CONFIGS = 7


@pytest.fixture(scope="module")
def golden():
    arrs = load_golden("g22_naf.npz")
    return arrs, json.loads(bytes(arrs["meta"]).decode())


def _construct(m):
    return nfs_amd.NeuralAutoregressiveFlow(m["dim"], list(m["hidden_dims"]), activation=m["activation"],
                                            use_layer_norm=m["use_layer_norm"], use_residual=m["use_residual"],
                                            dropout=m["dropout"])


def _flow(arrs, meta, i):
    flow = _construct(meta[i])
    p = f"c{i}.sd."
    flow.load_state_dict({k[len(p):]: torch.from_numpy(v.copy()) for k, v in arrs.items() if k.startswith(p)})
    return flow.eval()


def _t(arrs, key):
    return torch.from_numpy(arrs[key].copy())


def test_fixture_covers_the_options(golden):
    _, meta = golden
    assert len(meta) == N_CONFIGS
    assert {m["activation"] for m in meta} == set(ACTIVATIONS)
    assert {m["use_layer_norm"] for m in meta} == {True, False}
    assert {m["use_residual"] for m in meta} == {True, False}
    assert {1, 2} <= {m["dim"] for m in meta} and [16, 8] in [m["hidden_dims"] for m in meta]
    assert sum(m["dropout"] > 0 for m in meta) == 1
    assert max(m["clamped_share"] for m in meta) > 0.07  # the +-2 clamp of the conditioner is reached


@pytest.mark.parametrize("i", range(N_CONFIGS))
def test_state_dict_masks_and_degrees_are_the_reference(golden, i):
    arrs, meta = golden
    flow = _construct(meta[i])
    p = f"c{i}.sd."
    ref = {k[len(p):]: v for k, v in arrs.items() if k.startswith(p)}
    sd = flow.state_dict()
    assert sorted(sd) == sorted(ref)
    for k, v in sd.items():
        assert tuple(v.shape) == ref[k].shape and v.numpy().dtype == ref[k].dtype, k
        if k.endswith(".mask"):
            assert np.array_equal(v.numpy(), ref[k]), k
    c = flow.conditioner
    assert sorted(c.m) == list(range(-1, len(meta[i]["hidden_dims"])))
    for k, v in c.m.items():
        assert np.array_equal(np.asarray(v), arrs[f"c{i}.m.{k}"]), k
    assert len(c.masks) == len(meta[i]["hidden_dims"]) + 1
    for k, v in enumerate(c.masks):
        assert v.dtype == torch.float32 and np.array_equal(v.numpy(), arrs[f"c{i}.mask.{k}"]), k


def test_state_dict_keys_of_a_three_layer_flow():
    keys = list(nfs_amd.NeuralAutoregressiveFlow(4, [64, 64, 32]).state_dict())
    want = [f"conditioner.network.0.{k}" for k in ("weight", "bias", "mask")]
    want += [f"conditioner.network.1.{k}" for k in ("weight", "bias")]
    want += [f"conditioner.network.4.linear.{k}" for k in ("weight", "bias", "mask")]
    want += [f"conditioner.network.4.layer_norm.{k}" for k in ("weight", "bias")]
    want += [f"conditioner.network.5.{k}" for k in ("weight", "bias", "mask")]
    want += [f"conditioner.network.6.{k}" for k in ("weight", "bias")]
    want += [f"conditioner.network.9.{k}" for k in ("weight", "bias", "mask")]
    assert keys == want


@pytest.mark.parametrize("i", [0, 1])
def test_seeded_construction_is_the_reference_bit_for_bit(golden, i):
    arrs, meta = golden
    torch.manual_seed(meta[i]["seed"])
    sd = _construct(meta[i]).state_dict()
    p = f"c{i}.init."
    assert sorted(sd) == sorted(k[len(p):] for k in arrs if k.startswith(p))
    for k, v in sd.items():
        assert torch.equal(v, _t(arrs, p + k)), k


@pytest.mark.parametrize("i", range(N_CONFIGS))
def test_outputs_match_the_reference(golden, i):
    """forward and inverse against the reference's fp32 results: the same operations in the same
    order, so 1e-6 (1 + |ref|) for x and z and 1e-6 absolute for the log-det."""
    arrs, meta = golden
    flow, x = _flow(arrs, meta, i), _t(arrs, f"c{i}.x")
    for direction, tag, out in ((1, "fwd", "y"), (-1, "inv", "z")):
        y, ld = composite(flow, x, direction)
        yr, ldr = _t(arrs, f"c{i}.{tag}.{out}"), _t(arrs, f"c{i}.{tag}.ld")
        ey = float(((y - yr).abs() / (1 + yr.abs())).max())
        el = float((ld - ldr).abs().max())
        print(f"[naf c{i} {tag}] x/z {ey:.3e} log-det {el:.3e} (max |log-det| {float(ldr.abs().max()):.3e})")
        assert ey <= 1e-6 and el <= 1e-6
        assert float(ldr.abs().max()) > 1e-2


@pytest.mark.parametrize("i", range(N_CONFIGS))
def test_gradients_match_the_reference(golden, i):
    """Gradients of mean(0.5 |z|^2 - ld) through the inverse, with respect to x and every parameter,
    within 2e-5 of max|ref| per tensor (fp32 rounding of the same graph)."""
    arrs, meta = golden
    flow, x = _flow(arrs, meta, i), _t(arrs, f"c{i}.x")
    xr = x.clone().requires_grad_(True)
    z, ld = flow.inverse(xr)
    (0.5 * (z * z).sum(dim=1) - ld).mean().backward()
    grads = {"x": xr.grad, **{k: p.grad for k, p in flow.named_parameters()}}
    assert len(grads) == 1 + len(list(flow.parameters()))
    for k, g in grads.items():
        ref = _t(arrs, f"c{i}.grad.{k}")
        err, scale = float((g - ref).abs().max()), float(ref.abs().max())
        print(f"[naf c{i} grad] {k}: {err:.3e} of {scale:.3e}")
        assert err <= 2e-5 * scale + 1e-12, k
    assert float(_t(arrs, f"c{i}.grad.x").abs().max()) > 0


def test_train_mode_dropout_matches_under_the_same_seed(golden):
    arrs, meta = golden
    (i,) = [j for j, m in enumerate(meta) if m["dropout"] > 0]
    flow, x = _flow(arrs, meta, i).train(), _t(arrs, f"c{i}.x")
    assert flow._torch_only() is True and flow.eval()._torch_only() is False
    flow.train()
    torch.manual_seed(meta[i]["dropout_seed"])
    with torch.no_grad():
        z, ld = flow.inverse(x)
    zr, lr = _t(arrs, f"c{i}.train_inv.z"), _t(arrs, f"c{i}.train_inv.ld")
    assert float(((z - zr).abs() / (1 + zr.abs())).max()) <= 1e-6 and float((ld - lr).abs().max()) <= 1e-6
    assert float((zr - _t(arrs, f"c{i}.inv.z")).abs().max()) > 1e-3  # the dropout did something


@pytest.mark.parametrize("d", [3, 5])
def test_round_trip_without_layer_norm(d):
    """forward(inverse(x)) = x within 1e-4 when the conditioner is autoregressive (the reference
    reaches 4e-6)."""
    flow = make_flow(d, [32, 32], "elu", ln=False)
    x = make_inputs(40, d, seed=2)
    z, li = composite(flow, x, -1)
    xb, lf = composite(flow, z, 1)
    assert float((z - x).abs().max()) > 1e-2
    assert float((xb - x).abs().max()) <= 1e-4
    assert float((lf + li).abs().max()) <= 1e-4


def test_layer_norm_breaks_the_round_trip():
    """The reference's quirk, pinned: LayerNorm mixes the hidden units, the conditioner is not
    autoregressive, and forward is not the inverse of inverse."""
    flow = make_flow(3, [32, 32], "elu", ln=True)
    x = make_inputs(40, 3, seed=2)
    z, _ = composite(flow, x, -1)
    xb, _ = composite(flow, z, 1)
    assert float((xb - x).abs().max()) > 1e-1


def test_guards():
    flow = make_flow(3, [16, 16], "relu")
    x = make_inputs(8, 3, seed=4)
    clean = composite(flow, x, -1)
    x2 = x.clone()
    x2[2] = float("nan")
    for direction in (1, -1):
        y, ld = composite(flow, x2, direction)
        assert bool((y[2] == 0).all()) and float(ld[2]) == 0.0
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(ld).all())
    z, ld = composite(flow, x2, -1)
    keep = [r for r in range(8) if r != 2]
    assert torch.equal(z[keep], clean[0][keep]) and torch.equal(ld[keep], clean[1][keep])
    # the log-det is clamped to +-100: 64 dimensions at log-scale 2 each would be 128
    wide = make_flow(64, [8], "relu")
    with torch.no_grad():
        wide.conditioner.network[-1].bias[64:] = -5.0  # alpha = -2 after the clamp: log-scale +2
    _, ld = composite(wide, make_inputs(5, 64, seed=1), -1)
    assert bool((ld == 100.0).all())
    _, ld = composite(wide, make_inputs(5, 64, seed=1), 1)
    assert bool((ld == -100.0).all())


def test_routing_and_surface():
    flow = nfs_amd.NeuralAutoregressiveFlow(3, [16, 16])
    assert isinstance(flow, nfs_amd.flows.HipFlow) and nfs_amd.flows.NeuralAutoregressiveFlow is type(flow)
    assert isinstance(flow.conditioner, nfs_amd.DeepMADE) and nfs_amd.flows.DeepMADE is nfs_amd.DeepMADE
    assert isinstance(flow.conditioner.network[4], naf_mod.ResidualBlock)
    assert naf_mod.ResidualBlock is not nfs_amd.ResidualBlock
    assert (flow.dim, flow.data_dim, flow.clamp_alpha, flow.clamp_log_scale) == (3, 3, 3.0, 5.0)
    c = flow.conditioner
    assert (c.input_dim, c.hidden_dims, c.output_dim_multiplier, c.use_layer_norm, c.use_residual, c.dropout) == \
        (3, [16, 16], 2, True, True, 0.1)
    assert c.network[2] is c.activation and c.network[4].activation is c.activation
    default = nfs_amd.NeuralAutoregressiveFlow(2)
    assert default.conditioner.hidden_dims == [512, 512, 512]
    empty = nfs_amd.NeuralAutoregressiveFlow(3, [])  # constructs, as in the reference
    assert len(empty.conditioner.network) == 1 and empty.conditioner.masks == []
    for bad in ("tanh", "swish"):
        with pytest.raises(ValueError, match=f"Unsupported activation: {bad}"):
            nfs_amd.NeuralAutoregressiveFlow(3, [8], activation=bad)
    # CPU and fp64 calls run the composite
    flow = make_flow(3, [16, 16])
    x = make_inputs(6, 3)
    nfs_amd.reset_stats()
    composite(flow, x, -1)
    composite(flow, x, 1)
    composite(flow.double(), x.double(), -1)
    assert nfs_amd.STATS == {"hip": 0, "torch": 3}
    # train mode runs the kernel route unless dropout is active
    assert make_flow(3, [8]).train()._torch_only() is False
    assert make_flow(3, [8], dropout=0.2).train()._torch_only() is True
    assert make_flow(3, [8], dropout=0.2).eval()._torch_only() is False


def _widths(*w):
    return (ctypes.c_int * len(w))(*w)


def test_c_abi_validates_on_the_host():
    """The kernel family and argument checks of the C entry points answer without a GPU."""
    L = _lib.lib()
    relu, gelu, ln = _lib.NFX_NAF_RELU, _lib.NFX_NAF_GELU, _lib.NFX_NAF_LAYER_NORM
    res = _lib.NFX_NAF_RESIDUAL
    inside = [(16, [32]), (16, [64, 64]), (16, [128, 128]), (16, [64, 64, 64, 64]), (16, [128, 64, 32]), (1, [1]),
              (2, [20, 20]), (16, [128, 128, 128])]
    for d, w in inside:
        assert L.nfx_naf_supported(1, d, len(w), _widths(*w), relu, ln) == 1, (d, w)
        n = L.nfx_naf_packed_floats(d, len(w), _widths(*w))
        assert n > 0 and n % 4 == 0 and 4 * n <= 160 * 1024, (d, w)
    assert L.nfx_naf_supported(1 << 40, 16, 2, _widths(128, 128), gelu, ln | res(1)) == 1
    assert L.nfx_naf_packed_floats(2, 2, _widths(20, 20)) == L.nfx_naf_packed_floats(2, 2, _widths(32, 32))
    outside = [(17, [64]), (0, [64]), (2, [256]), (2, [0]), (2, [129]), (2, [8] * 5), (2, []), (16, [128] * 4),
               (2, [512, 512, 512])]
    for d, w in outside:
        assert L.nfx_naf_supported(1, d, len(w), _widths(*w), relu, ln) == 0, (d, w)
        assert L.nfx_naf_packed_floats(d, len(w), _widths(*w)) == 0, (d, w)
    w2 = _widths(64, 64)
    assert L.nfx_naf_supported(0, 2, 2, w2, relu, ln) == 0
    assert L.nfx_naf_supported(1, 2, 2, w2, 4, ln) == 0 and L.nfx_naf_supported(1, 2, 2, w2, -1, ln) == 0
    assert L.nfx_naf_supported(1, 2, 2, None, relu, ln) == 0
    assert L.nfx_naf_supported(1, 2, 2, w2, relu, res(1)) == 1
    assert L.nfx_naf_supported(1, 2, 2, w2, relu, res(0)) == 0        # the first layer has nothing to skip over
    assert L.nfx_naf_supported(1, 2, 2, w2, relu, res(2)) == 0        # no such layer
    assert L.nfx_naf_supported(1, 2, 2, _widths(64, 32), relu, res(1)) == 0  # unequal widths
    assert L.nfx_naf_supported(1, 2, 2, w2, relu, 64) == 0            # unknown bit

    def flow(B=16, d=2, nh=2, w=w2, act=relu, flags=ln, direction=_lib.NFX_INVERSE):
        return L.nfx_naf_flow(None, None, None, None, B, d, nh, w, act, flags, 3.0, 5.0, direction, 0, None)

    assert flow(d=17) == _lib.NFX_EUNSUPPORTED and b"d=17" in L.nfx_last_error()
    assert flow(nh=1, w=_widths(256)) == _lib.NFX_EUNSUPPORTED
    assert flow(nh=5, w=_widths(8, 8, 8, 8, 8)) == _lib.NFX_EUNSUPPORTED
    assert flow(act=7) == _lib.NFX_EUNSUPPORTED
    assert flow(direction=0) == _lib.NFX_EINVAL and b"direction" in L.nfx_last_error()
    assert flow(B=-1) == _lib.NFX_EINVAL and flow(d=0) == _lib.NFX_EINVAL and flow(w=None) == _lib.NFX_EINVAL
    assert flow(flags=res(0)) == _lib.NFX_EINVAL
    assert flow() == _lib.NFX_EINVAL and b"null" in L.nfx_last_error()
    assert flow(B=0) == 0
    assert L.nfx_naf_pack(None, 17, 2, w2, None, None) == _lib.NFX_EUNSUPPORTED
    assert L.nfx_naf_pack(None, 2, 2, w2, None, None) == _lib.NFX_EINVAL
    assert L.nfx_naf_pack(None, 0, 2, w2, None, None) == _lib.NFX_EINVAL


def _widths_handed_to_c(flow, monkeypatch):
    """The widths that the host check of `_hip_supported` reads through its `const int*` argument,
    copied out while the call is in progress."""
    seen = []
    real = _lib.checked().nfx_naf_supported

    def spy(B, d, nh, widths, act, flags):
        seen.append(list((ctypes.c_int * nh).from_address(widths)))
        return real(B, d, nh, widths, act, flags)

    monkeypatch.setattr(_lib.checked(), "nfx_naf_supported", spy)
    ok, why = flow._hip_supported(torch.zeros(4, flow.dim))
    assert ok, why
    return seen[-1]


def test_a_copied_or_pickled_flow_hands_c_its_own_widths(monkeypatch):
    """The cached plan travels with copy.deepcopy and pickle. It holds plain values only (a flow that
    has planned a call still pickles), and the host array handed to C is built for each call from the
    flow's own plan, so no copy reads memory that another object owns or that has been freed."""
    import copy
    import gc
    import pickle
    flow = make_flow(3, [16, 16, 8])
    plan = flow._plan()
    assert plan is not None and plan[2] == (16, 16, 8)
    assert _widths_handed_to_c(flow, monkeypatch) == [16, 16, 8]

    def plain(v):
        return not isinstance(v, (ctypes.Array, ctypes._SimpleCData, ctypes._Pointer))

    assert all(plain(v) for v in plan) and not any(type(v) is int and v > 1 << 20 for v in plan)
    clones = [copy.deepcopy(flow), pickle.loads(pickle.dumps(flow))]
    for clone in clones:
        cplan = clone.__dict__["_nfx_naf_plan"][1]  # the cache came along
        assert cplan[2] == (16, 16, 8)
        assert clone._plan()[0][0][0] is clone.conditioner.network[0]  # the copy's modules, not the original's
        arr, ptr = clone._widths_arg(clone._plan())
        assert ptr == ctypes.addressof(arr) and list(arr) == [16, 16, 8]
    del flow, plan
    gc.collect()
    for clone in clones:
        assert _widths_handed_to_c(clone, monkeypatch) == [16, 16, 8]
        y, ld = composite(clone, make_inputs(5, 3), -1)
        assert bool(torch.isfinite(y).all())


def test_the_plan_rejects_trees_the_constructor_does_not_build():
    def flow(**kw):
        return make_flow(3, [16, 16], **kw)

    assert flow()._plan() is not None and flow(ln=False, res=False, dropout=0.2)._plan() is not None
    f = flow()  # [MaskedLinear, LayerNorm, act, ResidualBlock, MaskedLinear]
    net = f.conditioner.network
    assert f.conditioner.plan() is not None
    # an extra module after the activation
    g = flow()
    g.conditioner.network = torch.nn.Sequential(*net[:3], torch.nn.Tanh(), *net[3:])
    assert g.conditioner.plan() is None and g._plan() is None
    # a missing activation
    g = flow()
    g.conditioner.network = torch.nn.Sequential(net[0], net[1], net[3], net[4])
    assert g._plan() is None
    g = flow(res=False)  # [ML, LN, act, ML, LN, act, ML]
    n2 = g.conditioner.network
    g.conditioner.network = torch.nn.Sequential(*n2[:5], n2[6])
    assert g._plan() is None
    # a ResidualBlock as the first layer
    g = flow()
    g.conditioner.network = torch.nn.Sequential(net[3], net[4])
    assert g._plan() is None
    # LayerNorm on one layer and not on the other
    g = flow()
    g.conditioner.network = torch.nn.Sequential(net[0], net[2], net[3], net[4])
    assert g.conditioner.plan() is not None and g._plan() is None
    # a plain Linear where a MaskedLinear belongs, a LayerNorm of another width, two activations
    g = flow()
    g.conditioner.network[4] = torch.nn.Linear(16, 6)
    assert g._plan() is None
    g = flow()
    g.conditioner.network[1] = torch.nn.LayerNorm(16, elementwise_affine=False)
    assert g._plan() is None
    g = flow()
    g.conditioner.network[2] = torch.nn.ELU()
    assert g.conditioner.plan() is not None and g._plan() is None
    # no hidden layer at all, and a conditioner that is not a DeepMADE
    assert nfs_amd.NeuralAutoregressiveFlow(3, [])._plan() is None
    g = flow()
    g.conditioner = torch.nn.Linear(3, 6)
    assert g._plan() is None
    # a rejected tree is reported as outside the family, and replacing a module re-plans
    g = flow()
    assert g._hip_supported(torch.zeros(2, 3))[0] is True
    g.conditioner.network[2] = torch.nn.Tanh()
    ok, why = g._hip_supported(torch.zeros(2, 3))
    assert ok is False and "kernel family" in why
