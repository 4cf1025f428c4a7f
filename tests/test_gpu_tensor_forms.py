"""GPU: results do not depend on the form a tensor arrives in.

The ctypes binding passes `data_ptr()` and nothing else, so the kernels see a dense row-major
array at whatever address they are given: correctness rests on every call site having made the
tensor contiguous and, where the kernel moves rows as 8- or 16-byte words, based at a 16-byte
boundary (`_lib.dense`). The reference modules accept any tensor torch accepts, so here one small
model per family runs every direction and the gradient pass with plain tensors (fresh, contiguous,
allocator-aligned) and with the same values held in another form: column-major, row-strided, a
column slice of a wider tensor, a contiguous view that starts one float into a larger buffer;
upstream gradients with stride 0, transposed, or one float into a buffer; parameters whose storage
is transposed, masks, BatchNorm buffers and spectral-norm vectors one float into a buffer. Results
must be bit-identical to the plain run, and the odd tensor's address must never reach the library
(a copy was made).

The entry points that promise to take a 4-byte-aligned base themselves (nfx_linear_*: the scalar
-load GEMM variants and the scalar column-sum kernel; nfx_flowbn_*: the scalar body) are called
directly with each operand in turn one float into a buffer and compared with float64 under the
bounds of test_gpu_generic.py::test_linear_kernels_vs_float64 and of test_gpu_flowbn_seq.py.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import nfs_amd
from nfs_amd import _lib
from test_gpu_flowbn_seq import abs_close, rel_close
from test_gpu_generic import _close
from test_gpu_stale_memory import _fresh, _fused_cnf_backward, _inputs
from stale_memory import same_bits

pytestmark = pytest.mark.gpu

BATCHES = [77, 1057]

# family -> (model kind of test_gpu_stale_memory._master, train mode in the gradient pass,
#            gradient pass also through forward())
FAMILIES = {
    "affine_fused": ("realnvp", False, False),
    "affine_fused_train": ("realnvp", True, False),
    "affine_any_shape": ("coupling_h256", False, False),
    "spline_d2": ("spline_d2", False, False),
    "spline_d3": ("spline", False, False),
    "maf": ("maf63", False, True),
    "iaf": ("iaf20_h32", False, True),
    "arqs": ("arqs_d4_k5", False, False),
    "cnf": ("cnf_d2_h64", False, False),
    "flowbn": ("realnvp_bn_between", True, False),
    "residual": ("residual_d5_h40", False, False),
    "naf": ("naf_d4_h64", False, False),
}
# The residual flow and the NAF have no backward kernel: their gradients recompute through the torch
# composite (STATS["torch"] == 1), which `_grad` refuses, so they run the eval tests only.
EVAL_ONLY_FAMILIES = ["residual", "naf"]
GRAD_FAMILIES = [f for f in FAMILIES if f not in EVAL_ONLY_FAMILIES]
EVAL_FAMILIES = [f for f in FAMILIES if f != "affine_fused_train"]


# ---- forms --------------------------------------------------------------------------------------
def off4(t):
    """The values of t, contiguous, one float into a larger buffer: data_ptr() % 16 == 4."""
    flat = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size() % 16
    return v


def col_major(t):
    v = t.t().contiguous().t()
    assert v.shape == t.shape and (t.shape[0] == 1 or t.shape[1] == 1 or not v.is_contiguous())
    return v


def row_strided(t):
    big = torch.full((2 * t.shape[0], t.shape[1]), 7.0, device=t.device, dtype=t.dtype)
    big[::2] = t
    return big[::2]


def col_slice(t):
    wide = torch.full((t.shape[0], t.shape[1] + 3), 7.0, device=t.device, dtype=t.dtype)
    wide[:, 1:1 + t.shape[1]] = t
    return wide[:, 1:1 + t.shape[1]]


X_FORMS = {"col_major": col_major, "row_strided": row_strided, "col_slice": col_slice, "off4": off4}


def weights_transposed(m):
    """Every 2-D `weight` becomes a Parameter whose storage is the transpose's."""
    for mod in m.modules():
        w = mod._parameters.get("weight")
        if w is not None and w.dim() == 2:
            mod.weight = nn.Parameter(w.detach().t().contiguous().t())
            assert mod.weight.shape == w.shape and (min(w.shape) == 1 or not mod.weight.is_contiguous())


def buffers_off4(m):
    """Every mask, every BatchNorm running statistic and every spectral-norm vector one float into a
    larger buffer."""
    n = 0
    for mod in m.modules():
        for name in ("mask", "running_mean", "running_var", "u", "v"):
            b = mod._buffers.get(name)
            if b is not None:
                mod._buffers[name] = off4(b)
                n += 1
    assert n > 0


PARAM_FORMS = {"weights_transposed": weights_transposed, "buffers_off4": buffers_off4}


# ---- what reaches the library -------------------------------------------------------------------
@pytest.fixture
def seen(monkeypatch):
    """The addresses of every tensor handed to the checked handle while the test runs."""
    ns, ptrs = _lib.checked(), set()

    def spy(fn):
        def call(*args):
            for a in args:
                if hasattr(a, "data_ptr"):
                    ptrs.add(a.data_ptr())
            return fn(*args)
        return call

    for name in _lib.EXPORTED_SYMBOLS:
        fn = getattr(ns, name, None)
        if fn is not None:
            monkeypatch.setattr(ns, name, spy(fn))
    return ptrs


# ---- the operations -----------------------------------------------------------------------------
def _model(family, dev, grad):
    kind, train, _ = FAMILIES[family]
    m, d = _fresh(kind, dev, train and grad)
    if family == "cnf":
        _fused_cnf_backward(m)
    return m, d


def _eval(m, x):
    nfs_amd.reset_stats()
    with torch.no_grad():
        lp = m.log_prob(x)
        z, ldi = m.inverse(x)
        y, ldf = m.forward(x)
    torch.cuda.synchronize()
    assert nfs_amd.STATS["hip"] > 0 and nfs_amd.STATS["torch"] == 0, dict(nfs_amd.STATS)
    return [("log_prob", lp), ("inverse z", z), ("inverse ld", ldi), ("forward x", y), ("forward ld", ldf)]


def _cotangents(B, d, dev, const):
    """Upstream gradients of (z, ld) per direction: random, or the ones `.sum().backward()` gives."""
    if const:
        return [torch.ones(B, d, device=dev), torch.ones(B, device=dev)] * 2
    g = torch.Generator().manual_seed(77 + B)
    return [torch.randn(s, generator=g).to(dev) for s in ((B, d), (B,), (B, d), (B,))]


def _grad(family, m, x, cot):
    """Gradients of <cot, (inverse(x), forward(x))> w.r.t. x and every parameter (train mode: and
    the BatchNorm statistics after the step)."""
    _, train, sampling = FAMILIES[family]
    nfs_amd.reset_stats()
    m.zero_grad(set_to_none=True)
    xr = x.detach().requires_grad_(True)
    outs = list(m.inverse(xr))
    if sampling:
        outs += list(m.forward(xr))
    torch.autograd.backward(outs, cot[:len(outs)])
    torch.cuda.synchronize()
    assert nfs_amd.STATS["hip"] > 0 and nfs_amd.STATS["torch"] == 0, dict(nfs_amd.STATS)
    res = [("x.grad", xr.grad)] + [(n + ".grad", p.grad) for n, p in m.named_parameters() if p.grad is not None]
    assert len(res) > 1
    if train:
        res += [(n, b) for n, b in m.named_buffers() if "running_" in n]
    return res


def _keep(res):
    return [(n, t.detach().clone()) for n, t in res]


@functools.lru_cache(maxsize=None)
def _plain_eval(family, B, dev):
    m, d = _model(family, dev, False)
    return _keep(_eval(m, _inputs(B, d, dev)))


@functools.lru_cache(maxsize=None)
def _plain_grad(family, B, const, dev):
    m, d = _model(family, dev, True)
    return _keep(_grad(family, m, _inputs(B, d, dev, 1.2), _cotangents(B, d, dev, const)))


def _assert_same(got, ref, what):
    assert [n for n, _ in got] == [n for n, _ in ref], what
    bad = []
    for (name, a), (_, b) in zip(got, ref):
        rows = same_bits(a.contiguous(), b.contiguous())
        if rows:
            bad.append((name, tuple(a.shape), len(rows), rows[:16]))
    assert not bad, (what, bad)


# ---- x in another form --------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(X_FORMS))
@pytest.mark.parametrize("family", EVAL_FAMILIES)
@pytest.mark.parametrize("B", BATCHES)
def test_eval_x_form(cuda_device, seen, family, form, B):
    m, d = _model(family, cuda_device, False)
    x = X_FORMS[form](_inputs(B, d, cuda_device))
    _assert_same(_eval(m, x), _plain_eval(family, B, cuda_device), (family, form))
    assert x.data_ptr() not in seen, "the odd tensor's own address reached the library: no copy was made"


@pytest.mark.parametrize("form", list(X_FORMS))
@pytest.mark.parametrize("family", GRAD_FAMILIES)
@pytest.mark.parametrize("B", BATCHES)
def test_gradient_x_form(cuda_device, seen, family, form, B):
    m, d = _model(family, cuda_device, True)
    x = X_FORMS[form](_inputs(B, d, cuda_device, 1.2))
    got = _grad(family, m, x, _cotangents(B, d, cuda_device, False))
    _assert_same(got, _plain_grad(family, B, False, cuda_device), (family, form))
    assert x.data_ptr() not in seen, "the odd tensor's own address reached the library: no copy was made"


# ---- upstream gradients in another form ---------------------------------------------------------
def _stride0(t):
    v = torch.ones((), device=t.device).expand(t.shape)
    assert all(s == 0 for s in v.stride())
    return v


def _transposed(t):
    return col_major(t) if t.dim() == 2 else row_strided(t.unsqueeze(1)).squeeze(1)


G_FORMS = {"stride0": (_stride0, True), "non_contiguous": (_transposed, False), "off4": (off4, False)}


@pytest.mark.parametrize("form", list(G_FORMS))
@pytest.mark.parametrize("family", GRAD_FAMILIES)
@pytest.mark.parametrize("B", BATCHES)
def test_gradient_cotangent_form(cuda_device, seen, family, form, B):
    fn, const = G_FORMS[form]
    m, d = _model(family, cuda_device, True)
    cot = [fn(t) for t in _cotangents(B, d, cuda_device, const)]
    got = _grad(family, m, _inputs(B, d, cuda_device, 1.2), cot)
    _assert_same(got, _plain_grad(family, B, const, cuda_device), (family, form))
    for t in cot:
        assert t.data_ptr() not in seen, "the odd tensor's own address reached the library: no copy was made"


# ---- parameters and buffers in another form -----------------------------------------------------
def _parameter_form_eval(family, form, B, dev):
    m, d = _model(family, dev, False)
    PARAM_FORMS[form](m)
    got = _eval(m, _inputs(B, d, dev))
    _assert_same(got, _plain_eval(family, B, dev), (family, form, "eval"))


# (the CNF has neither a mask nor a BatchNorm: nothing for buffers_off4 to move)
@pytest.mark.parametrize("family,form", [(fam, form) for fam in GRAD_FAMILIES for form in PARAM_FORMS
                                         if (fam, form) != ("cnf", "buffers_off4")])
@pytest.mark.parametrize("B", BATCHES)
def test_parameter_form(cuda_device, family, form, B):
    if family != "affine_fused_train":
        _parameter_form_eval(family, form, B, cuda_device)
    m, d = _model(family, cuda_device, True)
    PARAM_FORMS[form](m)
    got = _grad(family, m, _inputs(B, d, cuda_device, 1.2), _cotangents(B, d, cuda_device, False))
    _assert_same(got, _plain_grad(family, B, False, cuda_device), (family, form, "gradients"))


@pytest.mark.parametrize("form", list(PARAM_FORMS))
@pytest.mark.parametrize("family", EVAL_ONLY_FAMILIES)
@pytest.mark.parametrize("B", BATCHES)
def test_parameter_form_eval_only(cuda_device, family, form, B):
    """The eval half of test_parameter_form for the families without a backward kernel."""
    _parameter_form_eval(family, form, B, cuda_device)


def test_dense_copies_only_what_it_must(cuda_device):
    t = torch.randn(33, 6, device=cuda_device)
    assert _lib.dense(t) is t
    for form in X_FORMS.values():
        v = form(t)
        c = _lib.dense(v)
        assert c.is_contiguous() and c.data_ptr() % 16 == 0 and c.data_ptr() != v.data_ptr() and torch.equal(c, t)


# ---- buffers the caller owns and the library writes: refused, since they cannot be copied ---------
def test_caller_buffers_off_a_16_byte_boundary_are_refused(cuda_device):
    """A log_prob workspace (float64 partials) and the out = (z, x, ld) buffers of the sampling calls
    are written in place, so a copy cannot stand in for them: one that is not based at a 16-byte
    boundary raises, and the same buffers on an aligned base are taken."""
    m, d = _fresh("realnvp", cuda_device)
    B = 77
    x = _inputs(B, d, cuda_device)
    n = _lib.lib().nfx_gauss_workspace_bytes(B)
    raw = torch.empty(n + 16, device=cuda_device, dtype=torch.uint8)
    with torch.no_grad():
        ref = m.log_prob(x, workspace=raw[:n])
        with pytest.raises(ValueError, match="16-byte"):
            m.log_prob(x, workspace=raw[4:4 + n])
        assert torch.equal(m.log_prob(x, workspace=raw[16:16 + n]), ref)
        good = (torch.empty(B, d, device=cuda_device), torch.empty(B, d, device=cuda_device),
                torch.empty(B, device=cuda_device))
        assert m.sample_fused_ok(B, cuda_device)
        m.sample_fused(B, cuda_device, out=good)
        for i in range(3):
            bad = tuple(off4(t) if j == i else t for j, t in enumerate(good))
            with pytest.raises(ValueError, match="16-byte"):
                m.sample_fused(B, cuda_device, out=bad)
        # a stack without a fused draw: sample_on_device draws into z with the stand-alone kernel
        mb, db = _fresh("realnvp_bn_between", cuda_device)
        assert not mb.sample_fused_ok(B, cuda_device)
        z = torch.empty(B, db, device=cuda_device)
        mb.sample_on_device(B, cuda_device, out=(z, None, None))
        with pytest.raises(ValueError, match="16-byte"):
            mb.sample_on_device(B, cuda_device, out=(off4(z), None, None))


# ---- the entry points that take a 4-byte-aligned base themselves --------------------------------
@functools.lru_cache(maxsize=None)
def _linear_case(M, K, N):
    """Operands (CPU fp32) and float64 references with their conditioning, computed once."""
    g = torch.Generator().manual_seed(M + K + N)
    t = {"x": torch.randn(M, K, generator=g), "w": 0.2 * torch.randn(N, K, generator=g),
         "wmask": (torch.rand(N, K, generator=g) > 0.3).float(), "b": torch.randn(N, generator=g),
         "gy": torch.randn(M, N, generator=g)}
    x, w, b, gy = (t[k].double() for k in ("x", "w", "b", "gy"))
    wm = w * t["wmask"].double()
    ref = {"y": (x @ wm.T + b, x.abs() @ wm.abs().T + b.abs()),
           "gx": (gy @ wm, gy.abs() @ wm.abs()),
           "gw": ((gy.T @ x) * t["wmask"].double(), gy.abs().T @ x.abs()),
           "gb": (gy.sum(0), gy.abs().sum(0))}
    return t, ref


def _linear_run(t, M, K, N, dev):
    """The three nfx_linear_* entry points on device tensors t: (y, gx, gw, gb) and the kernel names."""
    L = _lib.checked()
    st = _lib.stream_of(t["x"])
    y = torch.empty(M, N, device=dev)
    gx = torch.empty(M, K, device=dev)
    gw = torch.empty(N, K, device=dev)
    gb = torch.empty(N, device=dev)
    ws = torch.empty(max(1, L.nfx_linear_workspace_bytes(M, N, K)), device=dev, dtype=torch.uint8)
    names = []
    L.nfx_linear_forward(t["x"], t["w"], t["wmask"], t["b"], None, None, None, y, M, K, N, 0, st)
    names.append(_lib.last_kernel())
    L.nfx_linear_backward_data(t["gy"], t["w"], t["wmask"], None, None, gx, M, N, K, 0, st)
    names.append(_lib.last_kernel())
    L.nfx_linear_backward_weight(t["gy"], t["x"], None, t["wmask"], gw, gb, M, N, K, ws, st)
    names.append(_lib.last_kernel())
    torch.cuda.synchronize()
    return {"y": y, "gx": gx, "gw": gw, "gb": gb}, names


@pytest.mark.parametrize("odd", ["none", "x", "w", "wmask", "gy"])
@pytest.mark.parametrize("M,K,N", [(65, 64, 64), (300, 128, 232)])
def test_linear_abi_operand_on_4_byte_base(cuda_device, M, K, N, odd):
    """K % 4 == 0 and N % 4 == 0, one operand one float into a buffer: gemm_go's va / vb turn false
    for it (the scalar-load variant of gemm_kernel at (65, 64, 64), of gemm2_kernel at
    (300, 128, 232)), and with gy odd at (65, 64, 64) the bias gradient runs colsum_kernel<false>
    (at (300, 128, 232) the large-tile GEMM sums the bias itself). Against float64 under
    test_linear_kernels_vs_float64's bound; whether the variant's bits equal the vector one's is
    printed, not required (the loads differ, the MFMA order does not)."""
    cpu, ref = _linear_case(M, K, N)
    plain = {k: v.to(cuda_device) for k, v in cpu.items()}
    t = dict(plain)
    if odd != "none":
        t[odd] = off4(plain[odd])
        assert t[odd].data_ptr() % 16 == 4
    got, names = _linear_run(t, M, K, N, cuda_device)
    for k, (r64, cond) in ref.items():
        _close(got[k], r64, cond, f"{k} with {odd} on a 4-byte base")
    if odd != "none":
        base, _ = _linear_run(plain, M, K, N, cuda_device)
        print(f"[tensor forms] linear ({M}, {K}, {N}) {odd} on a 4-byte base: last kernels {names}; bit-identical "
              f"to the aligned run: { {k: bool(torch.equal(got[k], base[k])) for k in got} }")


@functools.lru_cache(maxsize=None)
def _flowbn_case(B, d):
    g = torch.Generator().manual_seed(B + d)
    t = {"x": 1.5 * torch.randn(B, d, generator=g) + 0.3, "ld": torch.randn(B, generator=g),
         "gamma": 0.5 + torch.rand(d, generator=g), "beta": 0.1 * torch.randn(d, generator=g),
         "rm": 0.2 * torch.randn(d, generator=g), "rv": 0.5 + torch.rand(d, generator=g)}
    x, ld, ga, be, rm, rv = (t[k].double() for k in ("x", "ld", "gamma", "beta", "rm", "rv"))
    s = torch.sqrt(rv + 1e-5)
    c = (torch.log(ga.abs()) - 0.5 * torch.log(rv + 1e-5)).sum()
    mean = x.mean(0)
    ref = {1: ((x - rm) / s * ga + be, ld + c), -1: ((x - be) / ga * s + rm, ld - c),
           "mean": mean, "var": ((x - mean) ** 2).mean(0)}
    return t, ref


@pytest.mark.parametrize("odd", ["in", "out", "in_out"])
@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("B,d", [(77, 6), (1057, 16)])
def test_flowbn_apply_abi_on_4_byte_base(cuda_device, B, d, direction, odd):
    """flowbn_apply_kernel's scalar body (in or out off a 16-byte boundary): the same expression per
    element as the float4 body, contraction off, so the bits equal the aligned run's; and against
    float64 under the between-layer BatchNorm tests' tolerances (1e-5 (1 + |ref|), log-det 1e-4)."""
    cpu, ref = _flowbn_case(B, d)
    t = {k: v.to(cuda_device) for k, v in cpu.items()}
    L = _lib.checked()

    def run(x, out):
        ld = t["ld"].clone()
        L.nfx_flowbn_apply(x, out, ld, t["gamma"], t["beta"], t["rm"], t["rv"], 1e-5, B, d, direction,
                           _lib.stream_of(x))
        name = _lib.last_kernel()
        torch.cuda.synchronize()
        return out.clone(), ld, name

    y0, ld0, _ = run(t["x"], torch.empty(B, d, device=cuda_device))
    x = off4(t["x"]) if "in" in odd else t["x"]
    out = off4(torch.zeros(B, d, device=cuda_device)) if "out" in odd else torch.empty(B, d, device=cuda_device)
    assert (x.data_ptr() | out.data_ptr()) % 16 == 4
    y, ld, name = run(x, out)
    print(f"[tensor forms] flowbn_apply ({B}, {d}) dir {direction} {odd} on a 4-byte base: last kernel {name}")
    rel_close(y.cpu(), ref[direction][0], 1e-5)
    abs_close(ld.cpu(), ref[direction][1], 1e-4)
    assert torch.equal(y, y0) and torch.equal(ld, ld0)


@pytest.mark.parametrize("B,d", [(77, 6), (1057, 16)])
def test_flowbn_moments_abi_on_4_byte_base(cuda_device, B, d):
    """nfx_flowbn_moments reads x one float at a time in a fixed order: x off a 16-byte boundary gives
    the aligned run's bits; mean and biased variance against float64 (1e-6 (1 + |ref|), the bound of
    test_between_layer_bn_train_forward_updates_running_stats)."""
    cpu, ref = _flowbn_case(B, d)
    x = cpu["x"].to(cuda_device)
    L = _lib.checked()

    def run(x):
        stats = torch.empty(d, 3, device=cuda_device, dtype=torch.float64)
        ws = torch.empty(max(1, L.nfx_flowbn_workspace_bytes(B, d)), device=cuda_device, dtype=torch.uint8)
        L.nfx_flowbn_moments(x, B, d, stats, ws, _lib.stream_of(x))
        name = _lib.last_kernel()
        torch.cuda.synchronize()
        return stats, name

    s0, _ = run(x)
    xo = off4(x)
    assert xo.data_ptr() % 16 == 4
    s, name = run(xo)
    print(f"[tensor forms] flowbn_moments ({B}, {d}) x on a 4-byte base: last kernel {name}")
    assert torch.equal(s, s0)
    assert np.array_equal(s[:, 0].cpu().numpy(), np.full(d, float(B)))
    rel_close(s[:, 1].cpu(), ref["mean"], 1e-6)
    rel_close((s[:, 2] / B).cpu(), ref["var"], 1e-6)
