"""GPU: the N(0, I) base draw on the device for every model (csrc/nfx_rng.h, nfx_rng.hip), the
draw fused into the IAF forward tile kernel (nfx_made_affine_sample), `sample_on_device`,
`seed_sampler` and the generator state protocol.

One draw function serves every path: z[row, dim] = Box-Muller of Philox4x32-10 block dim / 4, word
pair (dim % 4) / 2, counter (row, block, offset), key = seed. The numpy reference below restates it
(Philox on uint64 arithmetic, checked against the published known answers; Box-Muller in float64 on
the same 24-bit uniforms); nfx_base_normal is compared with it element-wise, every fused kernel
with nfx_base_normal bit for bit, and x, log_det with forward(z) bit for bit.
"""
import math

import numpy as np
import pytest
import torch

import nfs_amd
from nfs_amd import _lib
from nfs_amd.flows import autoregressive as _ar

pytestmark = pytest.mark.gpu

# E0: max |z - reference| of the coupling chain's fused draw as it stood before this file existed
# (RealNVP(8, 6, 96).sample_fused(65536): 524,288 values) against draw_reference below, measured
# on an MI355X: 5.092e-07 (max |z| = 4.94; a float32 ulp there is 4.8e-07). The device functions are
# unchanged, so the bound for nfx_base_normal is 2 E0; the factor covers only the larger number of
# values drawn at d = 784 and d = 4096.
E0 = 5.092e-07
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c, k):
    """c: four uint64 arrays holding 32-bit words, k: two. Returns the four output words."""
    c0, c1, c2, c3 = [np.asarray(v, dtype=np.uint64) for v in c]
    k0, k1 = [np.asarray(v, dtype=np.uint64) for v in k]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def draw_reference(seed, offset, n, d):
    """float64 [n, d]: the draw function of csrc/nfx_rng.h."""
    nb = (d + 3) // 4
    row = np.arange(n, dtype=np.uint64)[:, None]
    blk = np.arange(nb, dtype=np.uint64)[None, :]
    c1 = (row >> np.uint64(32)) ^ ((blk >> np.uint64(8)) << np.uint64(8)) ^ ((blk << np.uint64(24)) & M32)
    zero = np.zeros((n, nb), dtype=np.uint64)
    seed, offset = np.uint64(seed), np.uint64(offset)
    w = philox4x32_10((row & M32 | zero, c1, zero | (offset & M32), zero | (offset >> np.uint64(32))),
                      (seed & M32, seed >> np.uint64(32)))
    out = np.empty((n, nb, 4))
    for pair in range(2):
        a, b = w[2 * pair], w[2 * pair + 1]
        u1 = ((a >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (b >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        out[:, :, 2 * pair] = r * np.cos(2.0 * np.pi * u2)
        out[:, :, 2 * pair + 1] = r * np.sin(2.0 * np.pi * u2)
    return out.reshape(n, 4 * nb)[:, :d]


def base_normal(seed, offset, n, d, device):
    """nfx_base_normal at (seed, offset) on a state of its own: (z, state)."""
    state = torch.tensor([offset, 0], dtype=torch.int64, device=device)
    z = torch.empty(n, d, device=device)
    _lib.check(_lib.lib().nfx_base_normal(seed, _lib.ptr(state), _lib.ptr(z), n, d, _lib.stream_of(z)),
               "nfx_base_normal")
    return z, state


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
    return m


def _stack(cls, d, H, L, seed):
    torch.manual_seed(seed)
    return _perturb(nfs_amd.NormalizingFlowModel([cls(d, H) for _ in range(L)]), seed + 1)


def _iaf(d, H, L, seed=0):
    return _stack(nfs_amd.InverseAutoregressiveFlow, d, H, L, seed)


def _maf(d, H, L, seed=0):
    return _stack(nfs_amd.MaskedAutoregressiveFlow, d, H, L, seed)


def _realnvp(d, L, H, seed, bn=False):
    torch.manual_seed(seed)
    return _perturb(nfs_amd.RealNVP(d, L, H, batch_norm_between_layers=bn), seed + 1)


def _spline(L, H, seed):
    torch.manual_seed(seed)
    return _perturb(nfs_amd.RealNVPSpline(2, L, H), seed + 1)


def _flow(m):
    return m.flow if hasattr(m, "flow") else m


def _state(m, device):
    return _flow(m)._nfx_rng[torch.device(device)]


# ---- 1. the draw definition -------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for c, k, want in kat:
        got = tuple(int(v) for v in philox4x32_10(c, k))
        assert got == want, (c, k, [hex(v) for v in got])


@pytest.mark.parametrize("n,d", [(1, 1), (33, 3), (4000, 2), (257, 784), (64, 4096)])
def test_base_normal_matches_the_reference(cuda_device, n, d):
    seed, offset = 0x1234_5678_9ABC_DEF0 + d, 3 + n
    z, state = base_normal(seed, offset, n, d, cuda_device)
    ref = draw_reference(seed, offset, n, d)
    err = float(np.abs(z.double().cpu().numpy() - ref).max())
    print(f"base_normal ({n}, {d}): max abs error {err:.3e} (bound {2 * E0:.3e})")
    assert state.tolist() == [offset + 1, state[1].item()] and state[1].item() & 0xFFFF == 0
    assert err <= 2 * E0


# ---- 2. no counter aliasing past dimension 1024 ---------------------------------------------------
def test_no_counter_aliasing_between_1024_blocks(cuda_device):
    z, _ = base_normal(99, 0, 64, 4096, cuda_device)
    blocks = [z[:, 1024 * i:1024 * (i + 1)] for i in range(4)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert (blocks[i] == blocks[j]).float().mean().item() < 1e-3, (i, j)


# ---- 3. the coupling and spline chains draw what they always drew ------------------------------
@pytest.mark.parametrize("d,L,H", [(2, 8, 64), (4, 4, 32), (8, 6, 96)])
def test_coupling_chain_draw_is_the_stand_alone_draw(cuda_device, d, L, H):
    m = _realnvp(d, L, H, d).to(cuda_device).eval()
    m.seed_sampler(77 + d)
    with torch.no_grad():
        m.sample_fused(33, cuda_device)
        _, _, z = m.sample_fused(4000, cuda_device)  # offset 1
    assert torch.equal(z, base_normal(77 + d, 1, 4000, d, cuda_device)[0])


def test_spline_chain_draw_is_the_stand_alone_draw(cuda_device):
    m = _spline(4, 32, 5).to(cuda_device).eval()
    m.seed_sampler(5)
    with torch.no_grad():
        _, _, z = m.sample_fused(4000, cuda_device)
    assert torch.equal(z, base_normal(5, 0, 4000, 2, cuda_device)[0])


# ---- 4. the draw fused into the IAF tile kernel ---------------------------------------------------
@pytest.mark.parametrize("d,H", [(2, 64), (3, 32), (5, 64), (63, 64), (64, 128)])
@pytest.mark.parametrize("n", [1, 31, 33, 4000, 300_001])
def test_fused_iaf_sample(cuda_device, d, H, n):
    L = 3
    m = _iaf(d, H, L, d + H).to(cuda_device).eval()
    assert m.sample_fused_ok(n, cuda_device)
    m.seed_sampler(1000 + d)
    with torch.no_grad():
        m.forward(torch.zeros(1, d, device=cuda_device))  # packs the weights
        # caller buffers with 40 guard rows behind them: the range-checked row stores of the last,
        # partial tile must leave them alone
        guard = 40
        zb, xb = [torch.full((n + guard, d), -7.0, device=cuda_device) for _ in range(2)]
        ldb = torch.full((n + guard,), -7.0, device=cuda_device)
        nfs_amd.reset_stats()
        x, ld, z = m.sample_fused(n, cuda_device, out=(zb[:n], xb[:n], ldb[:n]))
        assert nfs_amd.STATS["hip"] == L and nfs_amd.STATS["torch"] == 0, nfs_amd.STATS
        xr, ldr = m.forward(z)
    for buf in (zb, xb, ldb):
        assert (buf[n:] == -7.0).all()
    assert torch.equal(z, base_normal(1000 + d, 0, n, d, cuda_device)[0])
    assert torch.equal(x, xr) and torch.equal(ld, ldr)
    assert _state(m, cuda_device)[1][0].item() == 1


# ---- 5. every other model through sample_on_device ------------------------------------------------
def _check_on_device(m, n, d, device, seed):
    m.seed_sampler(seed)
    with torch.no_grad():
        m.forward(torch.zeros(2, d, device=device))
        nfs_amd.reset_stats()
        x, ld, z = m.sample_on_device(n, device)
        assert nfs_amd.STATS["torch"] == 0 and nfs_amd.STATS["hip"] > 0, nfs_amd.STATS
        xr, ldr = m.forward(z)
    assert z.shape == (n, d)
    assert torch.equal(z, base_normal(seed, 0, n, d, device)[0])
    assert torch.equal(x, xr) and torch.equal(ld, ldr)
    assert _state(m, device)[1][0].item() == 1
    return z


@pytest.mark.parametrize("policy", ["NFX_MADE_SEQ_AUTO", "NFX_MADE_SEQ_SEGMENT", "NFX_MADE_SEQ_WAVE",
                                    "NFX_MADE_SEQ_PUSH"])
def test_on_device_maf_every_sequential_policy(cuda_device, policy):
    m = _maf(2, 64, 6, 11).to(cuda_device).eval()
    assert not m.sample_fused_ok(4000, cuda_device)
    prev = _lib.lib().nfx_made_seq_policy(getattr(_lib, policy))
    try:
        _check_on_device(m, 4000, 2, cuda_device, 21)
    finally:
        _lib.lib().nfx_made_seq_policy(prev)


@pytest.mark.parametrize("d,H,n", [(150, 64, 1000),   # made_wide_kernel
                                   (4, 200, 1000)])   # H > 128
def test_on_device_iaf_outside_the_tile_kernel(cuda_device, d, H, n):
    m = _iaf(d, H, 2, d).to(cuda_device).eval()
    assert not m.sample_fused_ok(n, cuda_device)
    _check_on_device(m, n, d, cuda_device, 31 + d)


def test_on_device_iaf_any_shape_path_draws_what_the_fused_path_draws(cuda_device, monkeypatch):
    m = _iaf(2, 64, 3, 4).to(cuda_device).eval()
    m.seed_sampler(41)
    with torch.no_grad():
        assert m.sample_fused_ok(4000, cuda_device)
        zf = m.sample_on_device(4000, cuda_device)[2].clone()
    monkeypatch.setattr(_ar, "FORCE_GENERIC", True)
    assert not m.sample_fused_ok(4000, cuda_device)
    zg = _check_on_device(m, 4000, 2, cuda_device, 41)
    assert torch.equal(zf, zg)


def test_on_device_realnvp_above_the_small_batch_chain(cuda_device):
    m = _realnvp(2, 4, 32, 5).to(cuda_device).eval()
    assert not m.sample_fused_ok(1 << 17, cuda_device)
    _check_on_device(m, 1 << 17, 2, cuda_device, 51)


def test_on_device_realnvp_with_eval_batchnorm_between_layers(cuda_device):
    m = _realnvp(2, 4, 32, 6, bn=True).to(cuda_device).eval()
    assert not m.sample_fused_ok(4000, cuda_device)
    _check_on_device(m, 4000, 2, cuda_device, 61)


def test_on_device_raises_only_where_forward_leaves_hip(cuda_device):
    m = _realnvp(2, 4, 32, 7, bn=True).to(cuda_device).train()
    with pytest.raises(NotImplementedError):
        m.sample_on_device(100, cuda_device)
    with pytest.raises(NotImplementedError):
        _iaf(2, 64, 2).eval().sample_on_device(100, "cpu")


# ---- 6. the generator state ---------------------------------------------------------------------
_STATE_MODELS = {
    "coupling_chain": lambda: _realnvp(2, 8, 64, 1),
    "spline_chain": lambda: _spline(4, 32, 2),
    "iaf_tile": lambda: _iaf(2, 64, 3, 3),
    "stand_alone": lambda: _maf(2, 64, 2, 4),
}


@pytest.mark.parametrize("kind", list(_STATE_MODELS))
def test_state_advances_by_one_and_reseeds(cuda_device, kind):
    m = _STATE_MODELS[kind]().to(cuda_device).eval()
    assert m.sample_fused_ok(4000, cuda_device) == (kind != "stand_alone")
    m.seed_sampler(123)
    with torch.no_grad():
        z1 = m.sample_on_device(4000, cuda_device)[2].clone()
        state = _state(m, cuda_device)[1]
        assert state[0].item() == 1
        z2 = m.sample_on_device(4000, cuda_device)[2].clone()
        assert state[0].item() == 2
        assert (z1 == z2).float().mean().item() < 1e-3
        m.seed_sampler(123)
        assert _state(m, cuda_device)[1][0].item() == 0
        z3 = m.sample_on_device(4000, cuda_device)[2]
    assert torch.equal(z3, z1)


@pytest.mark.parametrize("arrival", [7, -1, 0])  # -1: 2^64 - 1 as the int64 the state tensor holds
def test_any_arrival_word_is_valid_coupling_chain(cuda_device, arrival):
    """Existing API only. With the plain arrival count this replaces, a leftover in state[1] kept
    the "last workgroup" test from firing at the right time: after 2^64 - 1 the offset advanced once
    and then every later call returned the same draws (measured: z1 == z2 everywhere)."""
    m = _realnvp(2, 8, 64, 1).to(cuda_device).eval()
    with torch.no_grad():
        z0 = m.sample_fused(4000, cuda_device)[2].clone()
        seed, state = m.flow._nfx_rng[torch.device(cuda_device)]
        off = state[0].item()
        state[1] = arrival
        z1 = m.sample_fused(4000, cuda_device)[2].clone()
        z2 = m.sample_fused(4000, cuda_device)[2].clone()
    assert state[0].item() == off + 2
    for a, b in ((z0, z1), (z1, z2), (z0, z2)):
        assert (a == b).float().mean().item() < 1e-3


@pytest.mark.parametrize("kind", ["spline_chain", "iaf_tile", "stand_alone"])
@pytest.mark.parametrize("arrival", [7, -1, 0])
def test_any_arrival_word_is_valid(cuda_device, kind, arrival):
    m = _STATE_MODELS[kind]().to(cuda_device).eval()
    with torch.no_grad():
        z0 = m.sample_on_device(4000, cuda_device)[2].clone()
        state = _state(m, cuda_device)[1]
        off = state[0].item()
        state[1] = arrival
        z1 = m.sample_on_device(4000, cuda_device)[2].clone()
        z2 = m.sample_on_device(4000, cuda_device)[2].clone()
    assert state[0].item() == off + 2
    for a, b in ((z0, z1), (z1, z2), (z0, z2)):
        assert (a == b).float().mean().item() < 1e-3


# ---- 7. captured graphs ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,fused,launches", [("iaf", True, 6), ("maf", False, 7)])
def test_graphed_sampling_of_made_stacks(cuda_device, kind, fused, launches):
    m = (_iaf if kind == "iaf" else _maf)(2, 64, 6, 8).to(cuda_device).eval()
    g = nfs_amd.GraphedFlow(m, torch.empty(4000, 2, device=cuda_device), mode="sample")
    assert g.fused_draw == fused and g.launches == launches
    x1, ld1 = [t.clone() for t in g()]
    z1 = g.static_in.clone()
    x2, ld2 = [t.clone() for t in g()]
    z2 = g.static_in.clone()
    assert (z1 == z2).float().mean().item() < 1e-3
    with torch.no_grad():
        for z, x, ld in ((z1, x1, ld1), (z2, x2, ld2)):
            xr, ldr = m.forward(z)
            assert torch.equal(xr, x) and torch.equal(ldr, ld)


# ---- 8. the draws are standard normal -----------------------------------------------------------
def _assert_standard_normal(z):
    """z: float64 [n, d] on the CPU. The levels of test_gpu_sample.py::test_fused_draw_is_standard_normal."""
    v = z.reshape(-1)
    assert abs(v.mean().item()) < 4 / math.sqrt(v.numel())
    assert abs(v.std().item() - 1) < 0.005
    assert abs(((v ** 4).mean() - 3).item()) < 0.03  # kurtosis of N(0, 1)
    s = v.sort().values
    cdf = 0.5 * (1 + torch.erf(s / math.sqrt(2)))
    emp = torch.arange(1, s.numel() + 1, dtype=torch.float64) / s.numel()
    ks = (cdf - emp).abs().max().item()
    assert ks < 1.63 / math.sqrt(s.numel()) * 1.5, ks  # ~1% KS level, with margin
    # adjacent dimensions (every pair (j, j + 1), pooled) and consecutive rows
    a, b = z[:, :-1].reshape(-1), z[:, 1:].reshape(-1)
    assert abs(torch.corrcoef(torch.stack([a, b]))[0, 1].item()) < 0.01
    a, b = z[:-1].reshape(-1), z[1:].reshape(-1)
    assert abs(torch.corrcoef(torch.stack([a, b]))[0, 1].item()) < 0.01


def test_stand_alone_draw_is_standard_normal(cuda_device):
    z, _ = base_normal(2024, 0, 1024, 784, cuda_device)
    _assert_standard_normal(z.double().cpu())


def test_fused_iaf_draw_is_standard_normal(cuda_device):
    m = _iaf(2, 64, 1, 9).to(cuda_device).eval()
    zs = []
    with torch.no_grad():
        for _ in range(8):
            zs.append(m.sample_fused(65536, cuda_device)[2].double().cpu())
    _assert_standard_normal(torch.cat(zs))  # 524,288 x 2
