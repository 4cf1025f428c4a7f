"""Bit identity of the streaming affine kernels when the output-layer fold skips dead outputs
(csrc/nfx_affine_kernel.h affine_nets_split_pipe<..., LIVE>, the pack's live-row words in
csrc/nfx_affine.hip) against digests recorded BEFORE that change.

An output j of a coupling layer's conditioner with mask[j] == 1 enters the layer's result only as
(1 - m) * ..., i.e. times +0, so its fold can be skipped, except where that +0 product decides a
bit: x = -0.0 on a masked-in coordinate (the sign of 0 * t), an |x| so large that t overflows
(0 * inf = NaN, then y = 0), a dead output that is NaN (a non-finite dead row of W3), or a
log-det that is zero in every term, whose sign the dead terms then decide. The cases
below put each of those next to clean 32-row tiles; tests/golden/g20_affine_live_fold_bits.json
holds, per case and output, the sha256 of the raw bytes (and the first rows as hex, for
diagnosis) as tools/record_live_fold_bits.py wrote them from the library before the change.

Models are seeded on the CPU and perturbed as bench.py's `perturb` (as
test_gpu_affine_split_bits.py), three RealNVP-masked layers each; "layer0" runs layer 0 of the
(2, 64) model alone through nfx_affine_coupling (affine_coupling_kernel). Layer 0 masks
coordinates [0, d/2) in, so coordinate 0 is masked-in and d - 1 masked-out there (and the other way
round in layer 1).
"""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

import nfs_amd
from conftest import golden_json

pytestmark = pytest.mark.gpu

GOLDEN = "g20_affine_live_fold_bits.json"
SIZES = (37, 101, 4133)
SHAPES = {"nvp_2_64": (2, 64, 201), "nvp_4_64": (4, 64, 202), "nvp_8_32": (8, 32, 203), "nvp_8_64": (8, 64, 204),
          "layer0": (2, 64, 201)}
VARIANTS = ("perturbed", "s_zero", "w3_inf", "w3_nan", "mask_half", "mask_ones", "mask_zeros", "ld_zero")
HEAD_ROWS = 4
NLAYERS = 3


def directions(name):
    return ("inverse", "forward") if name == "layer0" else ("log_prob", "inverse", "forward")


def cases():
    """(case id, model name, weight / mask variant, B); every case runs all directions."""
    return [(f"{name}-{var}-B{B}", name, var, B) for name in SHAPES for var in VARIANTS for B in SIZES]


def build_model(name, variant):
    """The CPU model of a case (not cached: the full-fold comparison builds it twice)."""
    from bench import perturb
    d, H, seed = SHAPES[name]
    torch.manual_seed(seed)
    layers = []
    for i in range(NLAYERS):
        mask = torch.zeros(d)
        if i % 2 == 0:
            mask[:d // 2] = 1
        else:
            mask[d // 2:] = 1
        layers.append(nfs_amd.CouplingLayer(d, H, mask))
    m = nfs_amd.NormalizingFlowModel(layers)
    perturb(m, 0.1, seed + 1000)
    with torch.no_grad():
        if variant == "s_zero":      # s is exactly +0 in every layer
            for f in layers:
                f.s_net[6].weight.zero_()
                f.s_net[6].bias.zero_()
        elif variant == "w3_inf":    # a dead row of layer 0 (mask[0] == 1): the layer must not elide
            layers[0].s_net[6].weight[0, 3] = float("inf")
        elif variant == "w3_nan":    # a dead row of layer 1 (mask[d - 1] == 1), or of layer 0 alone
            if name == "layer0":
                layers[0].b_net[6].weight[0, 5] = float("nan")
            else:
                layers[1].b_net[6].weight[d - 1, 5] = float("nan")
        elif variant == "mask_half":
            layers[0].mask[0] = 0.5
        elif variant == "mask_ones":
            layers[0 if name == "layer0" else 1].mask.fill_(1.0)
        elif variant == "mask_zeros":
            layers[0 if name == "layer0" else 1].mask.fill_(0.0)
        elif variant == "ld_zero":
            # layer 0's log-det is +-0 in every row though no output is zero by construction: the live
            # s are 1e-40 and (1 - m) = 2^-24 there, a product that underflows; the sign of that zero
            # hangs on the dead outputs, which are as perturbed
            f = layers[0]
            f.s_net[6].weight[d // 2:] = 0.0
            f.s_net[6].bias[d // 2:] = 1e-40
            f.mask[d // 2:] = 1.0 - 2.0 ** -24
    return m


@functools.lru_cache(maxsize=None)
def model(name, variant, dev):
    return build_model(name, variant).to(dev).eval()


# (tile offset within a group of 12 tiles, column: 0 = masked-in at layer 0, -1 = masked-out, value);
# the odd tiles between them stay clean
POISON = ((0, 0, -0.0), (2, -1, -0.0), (4, 0, 5e33), (6, 0, 3e38), (8, -1, 3e38), (10, None, float("nan")))


def make_inputs(name, B):
    """(clean batch, poisoned batch, mask of the rows in clean tiles of the poisoned batch). The
    poisons go to row 3 of every second 32-row tile, in turn, starting with a different one per
    batch size so that the small batches see them too."""
    d = SHAPES[name][0]
    clean = torch.randn(B, d, generator=torch.Generator().manual_seed(200000 + B + d))
    x = clean.clone()
    ntiles = (B + 31) // 32
    start = {37: 0, 101: 2, 4133: 0}[B]
    clean_rows = torch.ones(B, dtype=torch.bool)
    for t in range(0, ntiles, 2):
        row = 32 * t + 3
        if row >= B:
            break
        _, col, val = POISON[((t // 2) + start) % len(POISON)]
        if col is None:
            x[row] = val
        else:
            x[row, col] = val
        clean_rows[32 * t:32 * (t + 1)] = False
    return clean, x, clean_rows


def run_model(m, name, x, dev):
    """Every direction's outputs as CPU tensors under the streaming policy."""
    L = nfs_amd._lib
    f = L.lib().nfx_affine_kernel_policy
    prev = f(L.NFX_AFFINE_STREAMING)
    out = {}
    x = x.to(dev)
    try:
        with torch.no_grad():
            for dr in directions(name):
                if name == "layer0":
                    layer = m.flows[0]
                    y, ld = (layer.inverse if dr == "inverse" else layer.forward)(x)
                    assert "affine_coupling_kernel" in L.last_kernel(), L.last_kernel()
                    out[f"{dr}.y"], out[f"{dr}.ld"] = y, ld
                elif dr == "log_prob":
                    out["log_prob.logp"] = m.log_prob(x)
                else:
                    y, ld = (m.inverse if dr == "inverse" else m.forward)(x)
                    out[f"{dr}.y"], out[f"{dr}.ld"] = y, ld
    finally:
        f(prev)
    return {k: v.cpu().contiguous() for k, v in out.items()}


def run_case(case, dev, m=None):
    """{"clean.<output>", "poison.<output>"} of a case, plus the clean-tile row mask."""
    _, name, variant, B = case
    m = model(name, variant, dev) if m is None else m
    clean, x, clean_rows = make_inputs(name, B)
    out = {f"clean.{k}": v for k, v in run_model(m, name, clean, dev).items()}
    out.update({f"poison.{k}": v for k, v in run_model(m, name, x, dev).items()})
    return out, clean_rows


def digest(t):
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def head_hex(t):
    return t[:HEAD_ROWS].contiguous().numpy().tobytes().hex()


@functools.lru_cache(maxsize=None)
def recorded():
    return golden_json(GOLDEN)["cases"]


@pytest.mark.parametrize("case", cases(), ids=[c[0] for c in cases()])
def test_bits_equal_recorded(cuda_device, case):
    rec = recorded()[case[0]]
    out, clean_rows = run_case(case, cuda_device)
    assert sorted(out) == sorted(rec)
    for k, t in out.items():
        if digest(t) != rec[k]["sha256"]:
            want = np.frombuffer(bytes.fromhex(rec[k]["head"]), np.uint32)
            got = np.frombuffer(t[:HEAD_ROWS].contiguous().numpy().tobytes(), np.uint32)
            diff = np.flatnonzero(want != got)
            where = (f"first differing word of the first {HEAD_ROWS} rows: {int(diff[0])} "
                     f"(0x{int(got[diff[0]]):08x} vs recorded 0x{int(want[diff[0]]):08x})"
                     if diff.size else f"the first {HEAD_ROWS} rows agree; the difference is further in")
            raise AssertionError(f"{case[0]} / {k}: sha256 differs from the recorded bits; {where}")
    # a row's bits depend on its own 32-row tile only: the clean tiles of the poisoned batch
    for k, t in out.items():
        if k.startswith("poison."):
            c = out["clean." + k[len("poison."):]]
            assert torch.equal(t[clean_rows].view(torch.int32), c[clean_rows].view(torch.int32)), \
                f"{case[0]} / {k}: a clean tile differs from the same rows of the all-clean batch"


@pytest.mark.parametrize("case", [c for c in cases() if c[3] == 4133], ids=[c[0] for c in cases() if c[3] == 4133])
def test_elided_equals_full_fold(cuda_device, case):
    """NFX_AFFINE_LIVE_FOLD=0 (read when a layer's weights are packed) makes every layer refuse the
    elision: the same build's full fold, bit for bit."""
    _, name, variant, _ = case
    out, _ = run_case(case, cuda_device)
    keep = os.environ.get("NFX_AFFINE_LIVE_FOLD")
    os.environ["NFX_AFFINE_LIVE_FOLD"] = "0"
    try:
        m = build_model(name, variant).to(cuda_device).eval()
        full, _ = run_case(case, cuda_device, m)  # (packs on first use)
    finally:
        if keep is None:
            del os.environ["NFX_AFFINE_LIVE_FOLD"]
        else:
            os.environ["NFX_AFFINE_LIVE_FOLD"] = keep
    for k, t in out.items():
        assert torch.equal(t.view(torch.int32), full[k].view(torch.int32)), f"{case[0]} / {k}"
