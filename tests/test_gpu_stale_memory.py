"""GPU: no result depends on what a fresh allocation held.

Outputs, packed images, partial-sum workspaces, float64 sum blocks, kept activations, MADE factor
rows, the CNF trajectory and BatchNorm statistics all come from `torch.empty` / `torch.empty_like`,
i.e. from blocks the caching allocator recycles. A kernel that added into an unwritten slot,
reduced one partial more than was written or skipped a pad word of a packed image would see
whatever the process did before: a small finite number in a fresh test process (so every float64
comparison stays green), Inf or NaN bits in a long training run.

Each case runs its operation with every such allocation filled with zeros, all-ones NaN, +Inf and
1e38 (stale_memory.poisoned_empty, the patterns of test_gpu_lds_poison.py) on a fresh copy of the
model, so every cached image is rebuilt under the pattern, and requires results bit-identical to
the zero-filled run, which in turn is bit-identical to a run without the fixture. Every path here
is deterministic (fixed-order float64 reductions, no float atomics), so the comparison is exact.
"""
import copy
import functools

import pytest
import torch

import naf_cases
import nfs_amd
import residual_cases
from nfs_amd import _lib
from nfs_amd.flows import arqs as _aq
from nfs_amd.flows import autoregressive as _ar
from nfs_amd.flows import coupling as _cp
from nfs_amd.flows import spline as _sp
from nfs_amd.models import normalizing_flow_model as _nfm
from stale_memory import PATTERNS, poisoned_empty, same_bits
from test_gpu_lds_poison import KINDS, _alt_mask, _model, _perturb

pytestmark = pytest.mark.gpu

BATCHES = [77, 4099]  # one workgroup with a ragged tile; many workgroups' partial slots, no multiple of 4 or 32


@pytest.fixture
def poison():
    """poison(bits) -> context manager: torch.empty / torch.empty_like fill what they return with
    `bits` while it is open (counted), and are the originals again afterwards."""
    real = (torch.empty, torch.empty_like)
    yield poisoned_empty
    assert (torch.empty, torch.empty_like) == real


# ---- models -------------------------------------------------------------------------------------
def _one_hot_mask(d, i):
    m = torch.zeros(d)
    m[i % d] = 1
    return m


def _extra_model(kind):
    torch.manual_seed(5)
    N = nfs_amd.NormalizingFlowModel
    if kind == "cnf_d2_h64":
        return _perturb(N([nfs_amd.ContinuousFlow(2, 64)]), 0.1, 21), 2
    if kind == "cnf_d5_h32":
        return _perturb(N([nfs_amd.ContinuousFlow(5, 32)]), 0.1, 22), 5
    if kind == "cnf_d8_h64":
        return _perturb(N([nfs_amd.ContinuousFlow(8, 64)]), 0.1, 23), 8
    if kind == "spline_d2":  # the one-launch spline chain
        return _perturb(N([nfs_amd.SplineCouplingLayer(2, 64, _alt_mask(2, i), num_bins=8) for i in range(2)]),
                        0.1, 24), 2
    if kind == "spline_d3_h32_k4_nt2":  # two transformed dimensions per layer
        return _perturb(N([nfs_amd.SplineCouplingLayer(3, 32, _one_hot_mask(3, i), num_bins=4) for i in range(2)]),
                        0.1, 25), 3
    if kind == "realnvp_h96":
        return _perturb(nfs_amd.RealNVP(2, 4, 96), 0.1, 26), 2
    if kind == "iaf20_h32":
        return _perturb(N([nfs_amd.InverseAutoregressiveFlow(20, 32) for _ in range(2)]), 0.05, 27), 20
    if kind == "maf100_h64":  # d > 64 at H = 64: the wide backward kernel with x streamed in chunks
        return _perturb(N([nfs_amd.MaskedAutoregressiveFlow(100, 64) for _ in range(2)]), 0.02, 34), 100
    if kind == "maf20_h128":
        return _perturb(N([nfs_amd.MaskedAutoregressiveFlow(20, 128) for _ in range(2)]), 0.05, 28), 20
    if kind == "maf12_h32_bn":
        return _perturb(N([nfs_amd.MaskedAutoregressiveFlow(12, 32, use_batch_norm=True),
                           nfs_amd.InverseAutoregressiveFlow(12, 32, use_batch_norm=True)]), 0.05, 29), 12
    if kind == "arqs_d4_k5":
        return _perturb(N([nfs_amd.ARQS(4, 64, num_bins=5)]), 0.05, 30), 4
    if kind == "coupling_h256":
        return _perturb(N([nfs_amd.CouplingLayer(4, 256, _alt_mask(4, i)) for i in range(2)]), 0.05, 31), 4
    if kind == "spline_h256":
        return _perturb(N([nfs_amd.SplineCouplingLayer(3, 256, _alt_mask(3, i), num_bins=8) for i in range(2)]),
                        0.05, 32), 3
    if kind == "made_d12_h256":
        return _perturb(N([nfs_amd.MaskedAutoregressiveFlow(12, 256), nfs_amd.InverseAutoregressiveFlow(12, 256)]),
                        0.02, 33), 12
    # the two tile-owner families whose outputs and packed images come from torch.empty too; their
    # own redraws (residual_cases, naf_cases) put the spectral normalisation and the clamps to work
    if kind == "residual_d2_h64":
        return N([residual_cases.make_flow(2, 64, "tanh", 1.8)]), 2
    if kind == "residual_d5_h40":  # a kernel with scratch and a ragged tangent group
        return N([residual_cases.make_flow(5, 40, "elu", 0.9)]), 5
    if kind == "naf_d4_h64":
        return N([naf_cases.make_flow(4, (64, 64), "gelu")]), 4
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _master(kind):
    """The CPU master of a kind (test_gpu_lds_poison's twelve, or one of the above), built once."""
    m, d = _model(kind) if kind in KINDS else _extra_model(kind)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():  # BatchNorm statistics away from their (0, 1) initial values
        for name, b in m.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return m, d


def _fresh(kind, dev, train=False):
    m, d = _master(kind)
    m = copy.deepcopy(m).to(dev)
    return (m.train() if train else m.eval()), d


def _inputs(B, d, dev, scale=1.5):
    return (scale * torch.randn(B, d, generator=torch.Generator().manual_seed(1000 + B))).to(dev)


# ---- the comparison -----------------------------------------------------------------------------
def _run(op, bits, poison):
    """op() under the pattern (None: no fixture) -> ([(name, tensor clone)], tensors filled)."""
    _nfm._GAUSS_WS.clear()  # the cached log_prob workspace is allocated anew under this pattern
    nfs_amd.reset_stats()
    if bits is None:
        out, filled = op(), None
        torch.cuda.synchronize()
        out = [(n, t.detach().clone()) for n, t in out]
    else:
        with poison(bits) as count:
            out = op()
            torch.cuda.synchronize()
            out = [(n, t.detach().clone()) for n, t in out]
        filled = count.cuda
    assert nfs_amd.STATS["hip"] > 0 and nfs_amd.STATS["torch"] == 0, (bits, dict(nfs_amd.STATS))
    return out, filled


def _differences(got, ref):
    """Per tensor that differs: (name, shape, number of differing rows, the first of them)."""
    assert [n for n, _ in got] == [n for n, _ in ref]
    bad = []
    for (name, a), (_, b) in zip(got, ref):
        rows = same_bits(a, b)
        if rows:
            bad.append((name, tuple(a.shape), len(rows), rows[:16]))
    return bad


def _check(make_op, poison):
    """make_op() -> op on a fresh model. Pattern 0 == no fixture; every other pattern == pattern 0
    (every pattern is run, and every one that differs is reported)."""
    plain, _ = _run(make_op(), None, poison)
    zero, filled = _run(make_op(), 0, poison)
    assert filled > 0
    bad = {"zero-filled vs no fixture": _differences(zero, plain)}
    for bits in PATTERNS:
        got, filled = _run(make_op(), bits, poison)
        assert filled > 0
        bad[hex(bits) + " vs zero-filled"] = _differences(got, zero)
    lines = [f"{k}: {len(v)} tensors differ, e.g. (name, shape, rows that differ, the first) {v[:3]}"
             for k, v in bad.items() if v]
    assert not lines, "\n".join(lines)


def _eval_op(kind, B, dev):
    def make():
        m, d = _fresh(kind, dev)
        x = _inputs(B, d, dev)

        def op():
            with torch.no_grad():
                lp, sums = m.log_prob(x, return_sums=True)
                z, ldi = m.inverse(x)
                y, ldf = m.forward(x)
                m.seed_sampler(11)
                xs, lds, zs = m.sample_on_device(B, dev)
            return [("log_prob", lp), ("log_prob sums", sums), ("inverse z", z), ("inverse ld", ldi),
                    ("forward x", y), ("forward ld", ldf), ("sample x", xs), ("sample ld", lds), ("sample z", zs)]
        return op
    return make


def _grad_op(kind, B, dev, train=False, sampling=False, setup=None):
    """loss = -log_prob(x).mean() (+ forward(x)[0].square().mean() with sampling=True): x.grad, every
    parameter gradient, and in train mode the BatchNorm statistics after the step."""
    def make():
        m, d = _fresh(kind, dev, train)
        if setup is not None:
            setup(m)
        x = _inputs(B, d, dev, 1.2)

        def op():
            m.zero_grad(set_to_none=True)
            xr = x.clone().requires_grad_(True)
            loss = -m.log_prob(xr).mean()
            if sampling:
                loss = loss + m.forward(xr)[0].square().mean()
            loss.backward()
            out = [("loss", loss.detach()), ("x.grad", xr.grad)]
            out += [(n + ".grad", p.grad) for n, p in m.named_parameters() if p.grad is not None]
            assert len(out) > 2
            if train:
                out += [(n, b) for n, b in m.named_buffers() if "running_" in n or "num_batches" in n]
            return out
        return op
    return make


# ---- eval ---------------------------------------------------------------------------------------
EVAL_KINDS = KINDS + ["cnf_d2_h64", "cnf_d5_h32", "spline_d2", "residual_d2_h64", "residual_d5_h40", "naf_d4_h64"]


@pytest.mark.parametrize("kind", EVAL_KINDS)
@pytest.mark.parametrize("B", BATCHES)
def test_eval_independent_of_stale_memory(cuda_device, poison, kind, B):
    _check(_eval_op(kind, B, cuda_device), poison)


@pytest.mark.parametrize("chain", ["chain", "per_layer"])
@pytest.mark.parametrize("policy", ["NFX_AFFINE_STREAMING", "NFX_AFFINE_SMALL"])
@pytest.mark.parametrize("B", BATCHES)
def test_affine_policies_independent_of_stale_memory(cuda_device, poison, policy, chain, B):
    old = _lib.lib().nfx_affine_kernel_policy(getattr(_lib, policy))
    old_chain = _cp.CHAIN_MAX_B
    if chain == "per_layer":
        _cp.CHAIN_MAX_B = 0
    try:
        _check(_eval_op("realnvp", B, cuda_device), poison)
    finally:
        _cp.CHAIN_MAX_B = old_chain
        _lib.lib().nfx_affine_kernel_policy(old)


@pytest.mark.parametrize("policy,B", [("NFX_MADE_SEQ_SEGMENT", 77), ("NFX_MADE_SEQ_SEGMENT", 4099),
                                      ("NFX_MADE_SEQ_WAVE", 77), ("NFX_MADE_SEQ_WAVE", 4099),
                                      ("NFX_MADE_SEQ_PUSH", 1024)])
def test_made_seq_policies_independent_of_stale_memory(cuda_device, poison, policy, B):
    old = _lib.lib().nfx_made_seq_policy(getattr(_lib, policy))
    try:
        _check(_eval_op("iaf784", B, cuda_device), poison)
    finally:
        _lib.lib().nfx_made_seq_policy(old)


@pytest.mark.parametrize("mod,kind", [(_cp, "realnvp"), (_sp, "spline"), (_ar, "maf63"), (_aq, "arqs")],
                         ids=["coupling", "spline", "made", "arqs"])
@pytest.mark.parametrize("B", BATCHES)
def test_forced_any_shape_path_independent_of_stale_memory(cuda_device, poison, mod, kind, B):
    old = mod.FORCE_GENERIC
    mod.FORCE_GENERIC = True
    try:
        _check(_eval_op(kind, B, cuda_device), poison)
    finally:
        mod.FORCE_GENERIC = old


# ---- gradients ----------------------------------------------------------------------------------
GRAD_BATCHES = [1] + BATCHES
# Train-mode BatchNorm is not defined for one sample. The train-mode kernels take B >= 2 only
# (CouplingLayer._train_ok, autoregressive.bn_train_supported: `x.shape[0] >= 2`), so a single
# sample goes to the composite, whose nn.BatchNorm1d raises as the reference's does:
# test_train_mode_refuses_one_sample pins that.
TRAIN_BATCHES = BATCHES
TRAIN_KINDS = ["realnvp", "realnvp_h96", "realnvp_bn_between", "maf12_h32_bn", "coupling_h256"]

# (kind, sampling direction too)
EVAL_GRAD = [("spline_d2", False), ("spline_d3_h32_k4_nt2", False), ("maf63", True), ("iaf20_h32", True),
             ("maf100_h64", True), ("maf100_h128", True), ("maf20_h128", True), ("maf12_h32_bn", True), ("arqs_d4_k5", False),
             ("coupling_h256", False), ("spline_h256", False), ("made_d12_h256", True)]


@pytest.mark.parametrize("kind,sampling", EVAL_GRAD, ids=[k for k, _ in EVAL_GRAD])
@pytest.mark.parametrize("B", GRAD_BATCHES)
def test_gradients_independent_of_stale_memory(cuda_device, poison, kind, sampling, B):
    _check(_grad_op(kind, B, cuda_device, sampling=sampling), poison)


@pytest.mark.parametrize("kind", TRAIN_KINDS)
@pytest.mark.parametrize("B", TRAIN_BATCHES)
def test_train_mode_gradients_independent_of_stale_memory(cuda_device, poison, kind, B):
    # realnvp: nfx_affine_train_* with the kept layer-2 pre-activations; realnvp_h96: the wide kernel,
    # nothing kept; realnvp_bn_between: flowbn; the last two: the any-shape path's nfx_bn_*
    _check(_grad_op(kind, B, cuda_device, train=True, sampling=kind == "maf12_h32_bn"), poison)


@pytest.mark.parametrize("kind", TRAIN_KINDS)
def test_train_mode_refuses_one_sample(cuda_device, kind):
    """B = 1 in train mode raises (torch's "Expected more than 1 value per channel when training")
    before any train-mode kernel runs, and leaves the running means and variances as they were
    (nn.BatchNorm1d counts the batch in num_batches_tracked before it raises, as in the reference)."""
    m, d = _fresh(kind, cuda_device, train=True)
    before = {n: b.clone() for n, b in m.named_buffers() if "running_" in n}
    nfs_amd.reset_stats()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m.log_prob(_inputs(1, d, cuda_device).requires_grad_(True))
    assert nfs_amd.STATS["hip"] == 0, dict(nfs_amd.STATS)
    for n, b in m.named_buffers():
        if n in before:
            assert torch.equal(b, before[n]), n


@pytest.mark.parametrize("policy", ["NFX_MADE_SEQ_SEGMENT", "NFX_MADE_SEQ_WAVE"])
@pytest.mark.parametrize("kind", ["maf63", "iaf20_h32"])
@pytest.mark.parametrize("B", GRAD_BATCHES)
def test_sequential_gradients_independent_of_stale_memory(cuda_device, poison, kind, policy, B):
    """MAF.forward / IAF.inverse (the sequential directions) and their backward under each policy."""
    old = _lib.lib().nfx_made_seq_policy(getattr(_lib, policy))
    try:
        _check(_grad_op(kind, B, cuda_device, sampling=True), poison)
    finally:
        _lib.lib().nfx_made_seq_policy(old)


def _fused_cnf_backward(m):
    for f in m.flows:
        f.fused_backward = True  # on the instance: the class default stays off


@pytest.mark.parametrize("kind", ["cnf_d2_h64", "cnf_d8_h64"])
@pytest.mark.parametrize("B", GRAD_BATCHES)
def test_cnf_fused_backward_independent_of_stale_memory(cuda_device, poison, kind, B):
    _check(_grad_op(kind, B, cuda_device, setup=_fused_cnf_backward), poison)
