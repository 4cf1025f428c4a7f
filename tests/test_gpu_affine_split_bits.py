"""Bit identity of the streaming affine kernels (csrc/nfx_affine_kernel.h affine_nets_split_pipe /
affine_nets_split, csrc/nfx_affine_schain.hip) against recorded digests.

tests/golden/g19_affine_split_bits.json holds, per case and output, the sha256 of the output's raw
bytes (and its first 64 rows as hex, for diagnosis) as tools/record_split_bits.py wrote them from
the library BEFORE the split nets were software-pipelined. The pipeline changes instruction order
only: every accumulator receives the same products in the same order, so every output bit of
forward / inverse / log_prob must stay what it was. A row's bits depend only on its own 32-row
tile, so the digests do not depend on the CU count (the recorder checked: the one-launch chain
and the per-layer launches, which cut the batch differently, gave equal digests).

Inputs are torch.randn from a seeded CPU generator; weights are the G2 fixture or a CPU-seeded
model perturbed as bench.py's `perturb`, so the cases are the same on every machine. Batch sizes
name chunks per workgroup on a 256-CU part: 37 = one partial half chunk; 4,133 = one
chunk per workgroup or less, ragged tail; 114,725 = 7-8 chunks per workgroup ("first R waves
take a whole chunk"); 229,413 = 14 chunks (one full round plus halves); 1,250,021 = ~76 chunks
against a 73-chunk slice (second slice, layer 0's image re-staged).
"""
import functools
import hashlib

import numpy as np
import pytest
import torch

import nfs_amd
from conftest import golden_json, load_golden, state_dict_from

pytestmark = pytest.mark.gpu

GOLDEN = "g19_affine_split_bits.json"
G2_SIZES = (37, 4133, 114725, 229413, 1250021)
DIRECTIONS = ("log_prob", "inverse", "forward")
SEEDED = {"nvp_2_3_32": (2, 3, 32, 101), "nvp_4_3_64": (4, 3, 64, 102), "nvp_8_3_32": (8, 3, 32, 103)}
HEAD_ROWS = 64


def cases():
    """(case id, model name, B, poisoned, direction)."""
    out = []
    for B in G2_SIZES:
        for dr in DIRECTIONS:
            out.append((f"g2-B{B}-{dr}", "g2", B, False, dr))
    for dr in DIRECTIONS:
        out.append((f"g2-B4133-poison-{dr}", "g2", 4133, True, dr))
    for name in SEEDED:
        for dr in ("log_prob", "forward"):
            out.append((f"{name}-B4133-{dr}", name, 4133, False, dr))
    for dr in ("inverse", "forward"):
        out.append((f"g2-layer0-B4133-{dr}", "g2-layer0", 4133, False, dr))
    return out


@functools.lru_cache(maxsize=None)
def model(name, dev):
    if name in ("g2", "g2-layer0"):
        g = load_golden("g2_realnvp.npz")
        m = nfs_amd.RealNVP(2, 8, 64)
        m.load_state_dict(state_dict_from(g, "", m))
    else:
        from bench import perturb
        d, nl, H, seed = SEEDED[name]
        torch.manual_seed(seed)
        # RealNVP's stack and masks (models/real_nvp.py; its constructor takes even depths only)
        layers = []
        for i in range(nl):
            mask = torch.zeros(d)
            if i % 2 == 0:
                mask[:d // 2] = 1
            else:
                mask[d // 2:] = 1
            layers.append(nfs_amd.CouplingLayer(d, H, mask))
        m = nfs_amd.NormalizingFlowModel(layers)
        perturb(m, 0.1, seed + 1000)
    return m.to(dev).eval()


def make_input(name, B, poisoned):
    d = 2 if name.startswith("g2") else SEEDED[name][0]
    x = torch.randn(B, d, generator=torch.Generator().manual_seed(190000 + B + d))
    if poisoned:
        x[5] = float("nan")
        x[100, 0] = 3e38   # the masked-in column of layer 0
        x[2000, 1] = 3e38
    return x


def run_case(case, dev):
    """The case's outputs as CPU tensors, by name, under the streaming policy."""
    _, name, B, poisoned, dr = case
    L = nfs_amd._lib
    m = model(name, dev)
    x = make_input(name, B, poisoned).to(dev)
    f = L.lib().nfx_affine_kernel_policy
    prev = f(L.NFX_AFFINE_STREAMING)
    try:
        with torch.no_grad():
            if name == "g2-layer0":
                # layer 0 alone through nfx_affine_coupling (affine_coupling_kernel) and as a
                # one-layer chain (affine_schain_kernel): the shared split nets, bit for bit
                layer = m.flow.flows[0]
                y, ld = (layer.inverse if dr == "inverse" else layer.forward)(x)
                assert "affine_coupling_kernel" in L.last_kernel(), L.last_kernel()
                one = nfs_amd.NormalizingFlowModel([layer])
                yc, ldc = (one.inverse if dr == "inverse" else one.forward)(x)
                assert "affine_schain_kernel" in L.last_kernel(), L.last_kernel()
                out = {"y": y, "ld": ld, "chain_y": yc, "chain_ld": ldc}
            elif dr == "log_prob":
                out = {"logp": m.log_prob(x)}
            else:
                y, ld = (m.inverse if dr == "inverse" else m.forward)(x)
                out = {"y": y, "ld": ld}
    finally:
        f(prev)
    return {k: v.cpu().contiguous() for k, v in out.items()}


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
    out = run_case(case, cuda_device)
    assert sorted(out) == sorted(rec)
    for k, t in out.items():
        if digest(t) == rec[k]["sha256"]:
            continue
        want = np.frombuffer(bytes.fromhex(rec[k]["head"]), np.uint32)
        got = np.frombuffer(t[:HEAD_ROWS].contiguous().numpy().tobytes(), np.uint32)
        diff = np.flatnonzero(want != got)
        where = (f"first differing word of the first {HEAD_ROWS} rows: {int(diff[0])} "
                 f"(0x{int(got[diff[0]]):08x} vs recorded 0x{int(want[diff[0]]):08x}), {diff.size} words differ"
                 if diff.size else f"the first {HEAD_ROWS} rows agree; the difference is further in")
        raise AssertionError(f"{case[0]} / {k}: sha256 differs from the recorded bits; {where}")


@pytest.mark.parametrize("dr", ["inverse", "forward"])
def test_per_layer_kernel_equals_chain(cuda_device, dr):
    """affine_coupling_kernel (layer 0 alone, nfx_affine_coupling) and the first layer of the
    streaming chain run the same split nets: bit-equal outputs."""
    case = next(c for c in cases() if c[0] == f"g2-layer0-B4133-{dr}")
    out = run_case(case, cuda_device)
    assert torch.equal(out["y"].view(torch.int32), out["chain_y"].view(torch.int32))
    assert torch.equal(out["ld"].view(torch.int32), out["chain_ld"].view(torch.int32))
