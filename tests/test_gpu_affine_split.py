"""GPU: the bf16x3-split layer 2 of the streaming affine kernels against float64, at its edges.

affine_coupling_kernel (per layer) and affine_schain_kernel (one-launch chain) run layer 2 of both
conditioner nets as six bf16 piece products per fp32 multiply-add (csrc/nfx_affine_kernel.h:
split3, split_block, affine_net_split, affine_nets_split), guarded by two safety words of the
packed image: ok[0] (whole layer: W2 finite, |w| <= 1e6, and the bits cut below the smallest bf16
subnormal cannot move s by 2^-24) and ok[1] = xsafe (per 32-row tile). Every test forces
NFX_AFFINE_STREAMING. The reference is the CPU oracle in float64, the yardstick the same oracle in
fp32; neither is a kernel. Criterion on log_det (a plain sum of +-s, no exp in the way), with
e = |gpu - f64| and e_ref = |cpu32 - f64|: mean(e) <= 2 mean(e_ref) and max(e) <= 4 max(e_ref), no
absolute floor. tests/test_split_model_cpu.py shows on a CPU model that the six products measure
0.3 - 1.5 x and the nearest wrong scheme (three products) >= 10 x on the same cases.
"""
import numpy as np
import pytest
import torch

import nfs_amd
import oracle
import split_cases as sc
from conftest import assert_fp32_parity, fp32_jitter
from nfs_amd.flows import coupling as _cp

pytestmark = pytest.mark.gpu

B_SMALL, B_LARGE = 2085, 200_003


def _streaming(fn, chain=True):
    """fn under nfx_affine_kernel_policy(NFX_AFFINE_STREAMING), one-launch chains on or off."""
    L = nfs_amd._lib
    f = L.lib().nfx_affine_kernel_policy
    old_max = _cp.CHAIN_MAX_B
    if not chain:
        _cp.CHAIN_MAX_B = 0
    prev = f(L.NFX_AFFINE_STREAMING)
    try:
        with torch.no_grad():
            return fn()
    finally:
        _cp.CHAIN_MAX_B = old_max
        f(prev)


def _layer(sd, dev):
    d, H = sd["mask"].numel(), sd["s_net.0.weight"].shape[0]
    layer = nfs_amd.CouplingLayer(d, H, sd["mask"].clone())
    layer.load_state_dict(sd)
    return layer.to(dev).eval()


def _ok_words(layer, dev):
    """The safety words: the last four floats of the packed image."""
    return layer._packed(dev, layer._build_pack)[-4:].cpu().tolist()


def _f64(sd):
    return {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}


def _run(layer, x, direction):
    y, ld = _streaming(lambda: (layer.forward if direction > 0 else layer.inverse)(x))
    return y.cpu(), ld.cpu()


def _check_layer(layer, sd, x, what, dev, members=8):
    """The criterion on log_det and fp32 parity on y, both directions."""
    out = {}
    for direction in (1, -1):
        yg, lg = _run(layer, x.to(dev), direction)
        with torch.no_grad():
            y32, l32 = oracle.coupling(sd, "", x, direction)
            y64, l64 = oracle.coupling(_f64(sd), "", x.double(), direction)
        tag = f"{what} {'fwd' if direction > 0 else 'inv'}"
        out[direction] = sc.assert_split_criterion(lg.numpy(), l32.numpy(), l64.numpy(), tag + " log_det")
        sens = fp32_jitter(lambda s, v: oracle.coupling(s, "", v, direction), x, sd=sd, k=members, n_perm=members,
                           n_wjit=members)
        assert_fp32_parity(yg.numpy(), y32.numpy(), y64.numpy(), what=tag + " y", kind="y", sens=sens[0])
    return out


def _bits_equal(a, b, rows):
    return all(torch.equal(u[rows], v[rows]) for u, v in zip(a, b))


# ---- accuracy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H,B", [(d, H, B_SMALL) for d, H in sc.SHAPES] + [(2, 64, B_LARGE)])
@pytest.mark.parametrize("case", sc.CASES)
def test_split_layer_vs_float64(cuda_device, case, d, H, B):
    """Single layers, forward and inverse. (d, H) cover both hidden-tile counts, hidden units
    padded inside a tile and odd d; B = 2,085 runs 32-row half chunks and a ragged last tile,
    B = 200,003 is meant to run whole 64-row chunks (that depends on the device's resident wave
    count and is not asserted). At d = 1 (mask [1]) nothing is transformed: log_det is 0 on both
    sides and the case pins the pass-through and the tile guard with a padded layer-1 operand.
    ok[0] is 0 for binade_bal (|W2| > 1e6) and tiny (lower edge): those run the fp32 nets."""
    sd = sc.case_state(d, H, case, 1)
    layer = _layer(sd, cuda_device)
    ok = _ok_words(layer, cuda_device)
    x = sc.case_input(sd, case, B, 1, xsafe=ok[1])
    _check_layer(layer, sd, x, f"{case} d={d} H={H} B={B}", cuda_device, members=8 if B == B_SMALL else 2)
    assert ok[0] == (0.0 if case in sc.FP32_CASES else 1.0), ok


def _chain(d, H, nl, cases, dev, **kw):
    sds = [sc.case_state(d, H, c, 1 + i, mask=sc.alt_mask(d, i % 2), **(kw if c in ("wmax", "lower") else {}))
           for i, c in enumerate(cases)]
    m = nfs_amd.NormalizingFlowModel([nfs_amd.CouplingLayer(d, H, s["mask"].clone()) for s in sds])
    sd = {f"flows.{i}.{k}": v for i, s in enumerate(sds) for k, v in s.items()}
    m.load_state_dict(sd)
    return m.to(dev).eval(), sd, sds


def _check_chain(m, sd, nl, x_by_dir, what, dev):
    """One launch per call, bit equality with the per-layer streaming launches, and the criterion on
    the final log_det (both directions) and log_prob."""
    spec = oracle.realnvp_spec(nl, prefix="flows.")
    sd64 = _f64(sd)
    for direction, x in x_by_dir.items():
        xg = x.to(dev)
        assert _streaming(lambda: _cp.chain_ok(list(m.flows), xg))
        run = (lambda: m.forward(xg)) if direction > 0 else (lambda: m.inverse(xg))
        nfs_amd.reset_stats()
        yc, lc = _streaming(run)
        assert nfs_amd.STATS["hip"] == 1 and nfs_amd.STATS["torch"] == 0, nfs_amd.STATS
        yp, lp = _streaming(run, chain=False)
        assert torch.equal(yc, yp) and torch.equal(lc, lp), f"{what}: chain != per-layer launches"
        with torch.no_grad():
            y32, l32 = oracle.flow_model(sd, spec, x, direction)
            y64, l64 = oracle.flow_model(sd64, spec, x.double(), direction)
        tag = f"{what} {'fwd' if direction > 0 else 'inv'}"
        sc.assert_split_criterion(lc.cpu().numpy(), l32.numpy(), l64.numpy(), tag + " chain log_det")
        if direction < 0:
            nfs_amd.reset_stats()
            pc = _streaming(lambda: m.log_prob(xg))
            assert nfs_amd.STATS["hip"] == 1 and nfs_amd.STATS["torch"] == 0, nfs_amd.STATS
            pp = _streaming(lambda: m.log_prob(xg), chain=False)
            assert torch.equal(pc, pp), f"{what}: chain log_prob != per-layer launches"
            p32, p64 = oracle.gauss_log_prob(y32, l32), oracle.gauss_log_prob(y64, l64)
            sc.assert_split_criterion(pc.cpu().numpy(), p32.numpy(), p64.numpy(), tag + " chain log_prob")


@pytest.mark.parametrize("d,H,nl,B", [(2, 64, 4, B_SMALL), (4, 32, 3, B_SMALL), (8, 64, 2, B_SMALL), (2, 64, 4, B_LARGE)])
@pytest.mark.parametrize("case", sc.CASES)
def test_split_chain_vs_float64(cuda_device, case, d, H, nl, B):
    """The same cases through affine_schain_kernel: nl layers of the case with alternating masks.
    The inputs are crafted for the layer that runs first (layer 0 forward, layer nl - 1 inverse);
    later layers see what the chain hands them. log_prob of the edge cases is -inf on both sides
    (|z| ~ 1e30): only the pattern is compared there."""
    m, sd, sds = _chain(d, H, nl, [case] * nl, cuda_device)
    xs = {}
    for direction, first in ((1, 0), (-1, nl - 1)):
        ok = _ok_words(m.flows[first], cuda_device)
        xs[direction] = sc.case_input(sds[first], case, B, 2, xsafe=ok[1])
    _check_chain(m, sd, nl, xs, f"{case} d={d} H={H} nl={nl} B={B}", cuda_device)


# ---- whole-layer fallback: ok[0] ----------------------------------------------------------------------
BAD_ROW, TILE = 40, slice(32, 64)


def _tile_relations(layer, x, dev, expect_split, what):
    """An inf in one masked-in element of tile 1. The layer already on the fp32 nets: every clean
    row of the tile keeps its bits. The layer on the split: the tile falls back, so at least one
    bit of its clean rows changes. Rows outside the tile never change."""
    col = int(torch.nonzero(layer.mask.cpu() > 0)[0])
    xi = x.clone()
    xi[BAD_ROW, col] = float("inf")
    clean = [r for r in range(TILE.start, TILE.stop) if r != BAD_ROW]
    outside = [r for r in range(x.shape[0]) if not TILE.start <= r < TILE.stop]
    for direction in (1, -1):
        a, b = _run(layer, x.to(dev), direction), _run(layer, xi.to(dev), direction)
        assert _bits_equal(a, b, outside), f"{what}: rows outside the tile changed"
        assert _bits_equal(a, b, clean) == (not expect_split), \
            f"{what}: tile rows {'kept' if expect_split else 'changed'} their bits (dir {direction})"


@pytest.mark.parametrize("d,H", [(2, 64), (3, 48)])
def test_layer_fallback_at_w2_limit(cuda_device, d, H):
    """Largest folded |W2| entry 0.99e6: ok[0] = 1, the split runs. 1.01e6: ok[0] = 0, the fp32 nets
    run every tile. Both meet the float64 criterion."""
    for w2max, word in ((0.99e6, 1.0), (1.01e6, 0.0)):
        sd = sc.case_state(d, H, "wmax", 3, w2max=w2max)
        layer = _layer(sd, cuda_device)
        assert _ok_words(layer, cuda_device)[0] == word
        x = sc.case_input(sd, "wmax", B_SMALL, 3)
        _tile_relations(layer, x, cuda_device, expect_split=word == 1.0, what=f"|W2| {w2max:g}")
        _check_layer(layer, sd, x, f"wmax {w2max:g} d={d} H={H}", cuda_device)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_layer_fallback_nonfinite_w2(cuda_device, bad):
    """One W2 entry inf, then NaN: ok[0] = 0, and the finite / NaN pattern and the values follow the
    fp32 oracle (0 * inf = NaN where the hidden unit is off, clamp(+-inf) where it is on)."""
    sd = sc.case_state(2, 64, "plain", 4)
    sd["s_net.3.weight"][5, 7] = bad
    layer = _layer(sd, cuda_device)
    assert _ok_words(layer, cuda_device)[0] == 0.0
    x = sc.case_input(sd, "plain", 500, 4)
    for direction in (1, -1):
        yg, lg = _run(layer, x.to(cuda_device), direction)
        with torch.no_grad():
            yr, lr = oracle.coupling(sd, "", x, direction)
        assert np.array_equal(np.isfinite(yg.numpy()), np.isfinite(yr.numpy()))
        assert np.array_equal(lg.numpy() == 0, lr.numpy() == 0)  # the guard's zeros: where s was NaN
        assert float(((yg - yr).abs() / (1 + yr.abs())).max()) <= 1e-5
        assert float((lg - lr).abs().max()) <= 1e-4


def test_chain_with_one_unsafe_layer(cuda_device):
    """Four layers, only layer 1 beyond the W2 limit: the chain reads that layer's fp32 image
    (packs.p[DIR > 0 ? li : nl - 1 - li], reversed order on the inverse) and must equal the
    per-layer launches bit for bit in both directions."""
    d, H, nl = 2, 64, 4
    m, sd, sds = _chain(d, H, nl, ["plain", "wmax", "plain", "plain"], cuda_device, w2max=1.01e6)
    assert [_ok_words(f, cuda_device)[0] for f in m.flows] == [1.0, 0.0, 1.0, 1.0]
    x = sc.case_input(sds[0], "plain", B_SMALL, 5)
    _check_chain(m, sd, nl, {1: x, -1: x}, "layer 1 unsafe", cuda_device)


# ---- per-tile fallback: ok[1] = xsafe -------------------------------------------------------------------
@pytest.mark.parametrize("d,H", [(2, 64), (4, 32)])
def test_tile_fallback_at_xsafe(cuda_device, d, H):
    """ok[1] = (1e30 - max|b1'|) / max row-sum|w1'| of the folded layer 1, both nets. One masked-in
    element of row 40 at xsafe (1 - 1e-6): the tile stays on the split (bit-identical clean rows);
    at xsafe (1 + 1e-6): the tile runs the fp32 nets, exactly as with inf in that element."""
    sd = sc.case_state(d, H, "plain", 6)
    layer = _layer(sd, cuda_device)
    ok = _ok_words(layer, cuda_device)
    assert ok[0] == 1.0 and abs(ok[1] / sc.xsafe_f64(sd) - 1) <= 1e-5, (ok, sc.xsafe_f64(sd))
    x = sc.case_input(sd, "plain", B_SMALL, 6)
    col = int(torch.nonzero(sd["mask"] > 0)[0])
    clean = [r for r in range(TILE.start, TILE.stop) if r != BAD_ROW]
    outside = [r for r in range(B_SMALL) if not TILE.start <= r < TILE.stop]

    def at(v):
        xv = x.clone()
        xv[BAD_ROW, col] = v
        return xv

    below, above = float(np.float32(ok[1] * (1 - 1e-6))), float(np.float32(ok[1] * (1 + 1e-6)))
    assert below < ok[1] < above
    for direction in (1, -1):
        base = _run(layer, x.to(cuda_device), direction)
        lo = _run(layer, at(below).to(cuda_device), direction)
        hi = _run(layer, at(above).to(cuda_device), direction)
        inf = _run(layer, at(float("inf")).to(cuda_device), direction)
        assert _bits_equal(base, lo, clean), "below xsafe: the tile left the split"
        assert not _bits_equal(base, hi, clean), "above xsafe: the tile stayed on the split"
        assert _bits_equal(hi, inf, clean), "above xsafe: not the fp32 nets' bits"
        for out in (lo, hi):
            assert _bits_equal(base, out, outside), "rows outside the tile changed"
        for xv, (yg, lg) in ((at(below), lo), (at(above), hi)):
            with torch.no_grad():
                yr, lr = oracle.coupling(sd, "", xv, direction)
            assert bool(torch.isfinite(yg).all()) and bool(torch.isfinite(lg).all())
            assert float(((yg - yr).abs() / (1 + yr.abs())).max()) <= 1e-5
            assert float((lg - lr).abs().max()) <= 1e-4


# ---- the lower edge: pieces below the smallest bf16 subnormal ---------------------------------------------
def test_layer_fallback_at_lower_edge(cuda_device):
    """Activations under 2^-110 leave split3 a third piece below 2^-133, which pack_bf16 cuts. ok[0]
    requires 2^-133 * max row-sum|W2'| * max row-sum|W3| < 2^-24 (the most the cut can move s).
    One layer on each side: at 1.01 x the limit ok[0] = 0 and the float64 criterion holds even at
    activations ~ 2^-118; at 0.99 x the split runs, the cut bits move log_det by less than the
    bound (an absolute statement: fp32's own error shrinks with the activations, the cut does
    not), and with activations ~ 2^-104 (no piece cut) the criterion holds on both sides."""
    d, H = 2, 64
    for side, word in ((0.99, 1.0), (1.01, 0.0)):
        sd = sc.case_state(d, H, "lower", 7, loss=side * sc.LOSS_LIMIT)
        layer = _layer(sd, cuda_device)
        assert _ok_words(layer, cuda_device)[0] == word
        x = sc.case_input(sd, "lower", B_SMALL, 7)
        _tile_relations(layer, x, cuda_device, expect_split=word == 1.0, what=f"lower edge {side}")
        if word == 0.0:
            _check_layer(layer, sd, x, f"lower edge {side} activations 2^-118", cuda_device)
        else:
            for direction in (1, -1):
                _, lg = _run(layer, x.to(cuda_device), direction)
                with torch.no_grad():
                    l32 = oracle.coupling(sd, "", x, direction)[1].double()
                    l64 = oracle.coupling(_f64(sd), "", x.double(), direction)[1]
                e, er = float((lg.double() - l64).abs().max()), float((l32 - l64).abs().max())
                print(f"[split] lower edge {side} activations 2^-118: max err {e:.3g}, fp32 {er:.3g}, "
                      f"bound {sc.lower_edge_loss(sd):.3g}")
                assert e <= 4 * er + sc.lower_edge_loss(sd)
        x[:, 0] *= 2.0 ** 14
        _check_layer(layer, sd, x, f"lower edge {side} activations 2^-104", cuda_device)
