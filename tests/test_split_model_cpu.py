"""CPU: the crafted cases of tests/split_cases.py and a model of the bf16x3-split layer 2.

The GPU tests (tests/test_gpu_affine_split.py) hold the streaming kernels to "at most 2x the fp32
mean error and 4x the fp32 max error against float64" on these cases. This file shows, without a
GPU, that the criterion separates the arithmetic the kernel documents (six piece products, three
truncated activation pieces, three round-to-nearest weight pieces, hi/lo accumulation) from the
nearest wrong one (the three products with i + j <= 1), and that every case leaves its outputs
visible (at most 5 % of the float64 s values reach the +-10 clamp).
"""
import pytest
import torch

import oracle
import split_cases as sc
from oracle.flows_ref import _coupling_net

MODEL_SHAPES = ((2, 64), (8, 64))
ROWS = 256


def _case(d, H, case, seed=1, B=ROWS):
    sd = sc.case_state(d, H, case, seed)
    return sd, sc.case_input(sd, case, B, seed)


@pytest.mark.parametrize("d,H", sc.SHAPES)
@pytest.mark.parametrize("case", sc.CASES)
def test_cases_keep_s_visible(case, d, H):
    """Builder contract: the oracle's float64 s has |s| >= 10 (clamped: any error hidden) on at most
    5 % of the elements, the fp32 oracle's error against float64 is non-zero, and the masked-in
    inputs are what the case says (edge: |x * m| <= xsafe, reached to 1e-6)."""
    sd, x = _case(d, H, case, B=2085)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    xa = x * sd["mask"]
    s64 = _coupling_net(sd64, "s_net.", xa.double())
    s32 = _coupling_net(sd, "s_net.", xa)
    share = float((s64.abs() >= 10).double().mean())
    print(f"[split] {case} d={d} H={H}: clamp share {share:.4f}, |s| median {float(s64.abs().median()):.3g}")
    assert share <= 0.05
    assert float((s32.double() - s64).abs().max()) > 0
    if d > 1:  # (d = 1, mask [1]: nothing is transformed, log_det is 0 exactly)
        ld32, ld64 = oracle.coupling(sd, "", x, 1)[1], oracle.coupling(sd64, "", x.double(), 1)[1]
        assert float((ld32.double() - ld64).abs().max()) > 0
    if case in ("edge", "edge_pos"):
        top = float(xa.abs().max()) / sc.xsafe_f64(sd)
        assert 1 - 2e-6 <= top <= 1 - 5e-7, top
    if case in ("binade", "binade_bal"):
        h = torch.relu(xa.double() @ sc.fold(sd, "s_net.")[0].double().T)
        assert float(h.max() / h[h > 0].min()) >= 2.0 ** 58
    assert sc.w2_safe_f64(sd) == (case not in sc.FP32_CASES)


@pytest.mark.parametrize("d,H", MODEL_SHAPES)
@pytest.mark.parametrize("case", [c for c in sc.CASES if c != "tiny"])
def test_model_six_products_pass_three_fail(case, d, H):
    """The 6-product model meets the 2x / 4x criterion against float64 (yardstick: the k-ordered
    fp32 fma chain), the 3-product model does not: the GPU criterion can fail."""
    sd, x = _case(d, H, case)
    ref = sc.model_s(sd, x, "f64")
    yard = sc.model_s(sd, x, "f32")
    six = sc.model_s(sd, x, "split", products=sc.PRODUCTS_6)
    three = sc.model_s(sd, x, "split", products=sc.PRODUCTS_3)
    assert float((ref.abs() >= 10).double().mean()) <= 0.05
    r6, r3 = sc.error_ratios(six, yard, ref), sc.error_ratios(three, yard, ref)
    print(f"[split model] {case} d={d} H={H}: 6 products {r6[0]:.2f} / {r6[1]:.2f} x fp32 (mean / max), "
          f"3 products {r3[0]:.1f} / {r3[1]:.1f}")
    assert sc.meets_criterion(six, yard, ref), r6
    assert not sc.meets_criterion(three, yard, ref), r3
    assert r3[0] > 2 and r3[1] > 4, r3  # (outside on both counts)
    # binade_bal: |W2| > 1e6, the kernel runs the fp32 nets; no guard fires on the other cases
    assert torch.equal(sc.model_s(sd, x, "kernel"), yard if case in sc.FP32_CASES else six)


@pytest.mark.parametrize("d,H", MODEL_SHAPES)
def test_model_tiny_activations(d, H):
    """Activations ~ 2^-118: the third piece of split3 lies below the smallest bf16 subnormal
    (2^-133) and pack_bf16 cuts it, so the six products are an order of magnitude worse than fp32
    (two more if the matrix unit read subnormal inputs as zero). Nothing in the split itself can
    mend that; the pack's ok[0] now bounds what the cut bits can do to s (lower_edge_loss <
    LOSS_LIMIT), the case's layer exceeds the bound, and the kernel as modelled runs the fp32 nets."""
    sd, x = _case(d, H, "tiny")
    ref, yard = sc.model_s(sd, x, "f64"), sc.model_s(sd, x, "f32")
    six = sc.model_s(sd, x, "split")
    flushed = sc.model_s(sd, x, "split", flush=True)
    r6, rf = sc.error_ratios(six, yard, ref), sc.error_ratios(flushed, yard, ref)
    print(f"[split model] tiny d={d} H={H}: 6 products {r6[0]:.1f} / {r6[1]:.1f} x fp32, subnormal pieces flushed "
          f"{rf[0]:.0f} / {rf[1]:.0f}; lower-edge bound {sc.lower_edge_loss(sd):.3g} vs limit {sc.LOSS_LIMIT:.3g}")
    assert r6[0] > 8 and r6[1] > 8, r6
    assert rf[0] > 20 * r6[0], (rf, r6)
    assert sc.lower_edge_loss(sd) >= sc.LOSS_LIMIT and not sc.w2_safe_f64(sd)
    kern = sc.model_s(sd, x, "kernel")
    assert torch.equal(kern, yard) and sc.meets_criterion(kern, yard, ref)


def test_model_lower_threshold_sides():
    """One layer on each side of the lower-edge limit. Below it the split runs and the bits it cuts
    move s by less than the bound (hence by less than LOSS_LIMIT); the relative criterion cannot
    hold there for activations under 2^-110 (fp32's own error shrinks with the activations, the
    cut does not), which is why the bound is absolute. With activations at 2^-104 no piece is cut
    and both sides meet the relative criterion."""
    d, H = 2, 64
    for side, safe in ((0.99, True), (1.01, False)):
        sd = sc.case_state(d, H, "lower", 1, loss=side * sc.LOSS_LIMIT)
        assert sc.w2_safe_f64(sd) == safe
        x = sc.case_input(sd, "lower", ROWS, 1)
        ref, yard, kern = (sc.model_s(sd, x, m) for m in ("f64", "f32", "kernel"))
        e = float((kern - ref).abs().max())
        assert e <= 4 * float((yard - ref).abs().max()) + sc.lower_edge_loss(sd), e
        assert safe or torch.equal(kern, yard)
        x[:, 0] *= 2.0 ** 14  # activations ~ 2^-104: every piece representable
        ref, yard, kern = (sc.model_s(sd, x, m) for m in ("f64", "f32", "kernel"))
        assert float((ref.abs() >= 10).double().mean()) <= 0.05
        r = sc.error_ratios(kern, yard, ref)
        print(f"[split model] lower-edge {side}: {r[0]:.2f} / {r[1]:.2f} x fp32 at activations 2^-104")
        assert sc.meets_criterion(kern, yard, ref), r


def test_safety_words_f64():
    """xsafe and the W2 bound recomputed from the fold, on layers built to sit at the edges."""
    sd = sc.case_state(2, 64, "edge", 1)
    assert abs(sc.xsafe_f64(sd) / 1e30 - 1) < 1e-5
    for w, ok in ((0.99e6, True), (1.01e6, False)):
        s = sc.case_state(2, 64, "wmax", 1, w2max=w)
        top = max(float(sc.fold(s, n)[2].abs().max()) for n in sc.NETS)
        assert abs(top / w - 1) < 1e-6 and sc.w2_safe_f64(s) == ok
