"""Crafted CouplingLayer cases for the bf16x3-split layer 2 (csrc/nfx_affine_kernel.h: split3,
split_block, affine_net_split), shared by the CPU model test (tests/test_split_model_cpu.py) and
the GPU tests (tests/test_gpu_affine_split.py). Not a conftest: plain functions, imported by name.

A case is a state dict keyed as oracle.coupling reads it (both conditioner nets, BatchNorm buffers
included, `mask`) and an input batch. The seven cases:

  plain       N(0,1)-scaled weights, random BatchNorm statistics (exercises the fold)
  binade      layer-1 activations spread over 2^-30 .. 2^30 inside every layer-2 dot product
              (W1 rows 2^e, zero b1, positive masked-in inputs in (0.5, 2)); W2 O(1), W3 * 2^-28
  binade_bal  the same activations with W2's columns scaled 2^-e: every term of the dot is O(1).
              |W2| reaches 2^30 / 8 > 1e6, so ok[0] = 0 and the kernels run this layer on the fp32
              nets: the case pins the whole-layer fallback, not the split
  binade_bal18  the same with e spread over [-18, 18] (|W2| < 1e6): stays on the split
  cancel      W2 rows of +-100 pairs that cancel to 1e-4: the result is 1e-4 of the terms
  edge        masked-in inputs at xsafe (1 - 1e-6), |W2| up to 0.99e6 with random signs
  edge_pos    the same with every W2 entry positive: partial sums reach ~6e37, finite
  tiny        activations ~ 2^-118 (the third bf16 piece is subnormal), |W2| <= 9e5, W3 * 2^96

plus `wmax` (a plain-like layer whose largest folded |W2| entry is set exactly) and `lower`
(tiny-like, the subnormal-piece bound of the pack set exactly) for the two ok[0] thresholds.

Also here: the BatchNorm fold in float64 as the pack kernel does it (csrc/nfx_pack.h), the two
safety words recomputed from it, a CPU model of the split arithmetic with a parameter for which
piece products are summed, and the float64 / fp32 error criterion every test applies.
"""
import numpy as np
import torch

CASES = ("plain", "binade", "binade_bal", "binade_bal18", "cancel", "edge", "edge_pos", "tiny")
FP32_CASES = ("binade_bal", "tiny")  # ok[0] = 0: the whole layer runs the fp32 nets
SHAPES = ((1, 16), (2, 64), (3, 48), (4, 32), (8, 64))
NETS = ("s_net.", "b_net.")
W2_LIMIT = 1e6            # ok[0]: every folded |w2| <= 1e6
ACT_LIMIT = 1e30          # ok[1] = xsafe keeps every layer-1 activation <= 1e30
BF16_MIN_SUBNORMAL = 2.0 ** -133
# ok[0] (lower edge): 2^-133 * max row-sum|W2'| * max row-sum|W3| < 2^-24 — the most the bits an
# activation piece loses below the smallest bf16 subnormal can move s, kept under the relative
# rounding of exp(s) in fp32 (csrc/nfx_affine.hip affine_split_pack_kernel)
LOSS_LIMIT = 2.0 ** -24


def alt_mask(d, phase=0):
    m = torch.zeros(d)
    m[phase::2] = 1
    return m


# ---- state dicts ---------------------------------------------------------------------------------
def _identity_bn(sd, n, H):
    for i in (1, 4):
        sd[n + f"{i}.weight"] = torch.ones(H)
        sd[n + f"{i}.bias"] = torch.zeros(H)
        sd[n + f"{i}.running_mean"] = torch.zeros(H)
        sd[n + f"{i}.running_var"] = torch.ones(H) - 1e-5
        sd[n + f"{i}.num_batches_tracked"] = torch.tensor(0)


def case_state(d, H, case, seed, mask=None, w2max=None, loss=None):
    """State dict of one CouplingLayer(d, H) for `case`. `mask` defaults to alt_mask(d).
    w2max (case "wmax"): the largest folded |W2| entry, over both nets. loss (case "lower"): the
    value of lower_edge_loss(sd), set by scaling W3."""
    gen = torch.Generator().manual_seed(seed * 7919 + d * 131 + H)
    mask = alt_mask(d) if mask is None else mask.clone().float()
    inn = mask > 0
    n_in = max(int(inn.sum()), 1)
    rn = lambda *s: torch.randn(*s, generator=gen)
    ru = lambda *s: torch.rand(*s, generator=gen)
    sd = {}
    for n in NETS:
        w1 = rn(H, d)          # masked-out columns: random (they multiply x * m = 0)
        b1 = torch.zeros(H)
        b2 = torch.zeros(H)
        top = 18 if case == "binade_bal18" else 30
        e = torch.linspace(-top, top, H)[torch.randperm(H, generator=gen)]
        if case in ("plain", "wmax"):
            b1 = 0.1 * rn(H)
            w2 = rn(H, H) / H ** 0.5
            b2 = 0.1 * rn(H)
            w3 = rn(d, H) / H
        elif case in ("binade", "binade_bal", "binade_bal18"):
            w1[:, inn] = (2.0 ** e)[:, None] * (1 + ru(H, n_in)) / n_in
            w2 = rn(H, H) / H ** 0.5
            b2 = 0.1 * rn(H)
            w3 = rn(d, H) / H
            if case == "binade":
                w3 = w3 * 2.0 ** -28
            else:
                w2 = w2 * (2.0 ** -e)[None, :]
        elif case == "cancel":
            w1[:, inn] = (1 + 0.01 * rn(H, n_in)) / n_in
            b1 = 0.5 + 0.01 * rn(H)
            half = 100 * rn(H, H // 2)
            w2 = torch.cat([half, -half * (1 + 1e-4 * rn(H, H // 2))], 1)
            b2 = 0.1 * rn(H)
            w3 = rn(d, H) / H / 10
        elif case in ("edge", "edge_pos"):
            w1 = torch.zeros(H, d)
            w1[:, inn] = (0.5 + 0.5 * ru(H, n_in)) / n_in
            w1[0, inn] = 1.0 / n_in   # the row that reaches 1e30 at |x * m| = xsafe
            w2 = 0.99e6 * (0.5 + 0.5 * ru(H, H))
            if case == "edge":
                w2 = w2 * (torch.randint(0, 2, (H, H), generator=gen) * 2 - 1)
            w3 = rn(d, H) * ((1e-36 if case == "edge" else 1e-38) / 8)
        elif case in ("tiny", "lower"):
            w1[:, inn] = 2.0 ** -118 * (1 + ru(H, n_in)) / n_in
            w2 = rn(H, H)
            w2 = w2 * (9e5 / w2.abs().max())
            w3 = rn(d, H) / H * 2.0 ** 96
        else:
            raise ValueError(case)
        sd.update({n + "0.weight": w1.float(), n + "0.bias": b1.float(), n + "3.weight": w2.float(),
                   n + "3.bias": b2.float(), n + "6.weight": w3.float(), n + "6.bias": torch.zeros(d)})
        _identity_bn(sd, n, H)
        if case == "plain":
            for i in (1, 4):
                sd[n + f"{i}.weight"] = 1 + 0.1 * rn(H)
                sd[n + f"{i}.bias"] = 0.1 * rn(H)
                sd[n + f"{i}.running_mean"] = 0.1 * rn(H)
                sd[n + f"{i}.running_var"] = 0.5 + ru(H)
    sd["mask"] = mask
    if case == "wmax":
        top = max(float(fold(sd, n)[2].abs().max()) for n in NETS)
        for n in NETS:  # (fp32 rounding moves the entry by 1e-7 relative; the tests use +-1 %)
            sd[n + "3.weight"] = (sd[n + "3.weight"].double() * (w2max / top)).float()
            sd[n + "6.weight"] = (sd[n + "6.weight"].double() * (top / w2max)).float()  # s stays O(1)
    if case == "lower":
        cur = lower_edge_loss(sd)
        for n in NETS:
            sd[n + "6.weight"] = (sd[n + "6.weight"].double() * (loss / cur)).float()
    return sd


def case_input(sd, case, B, seed, xsafe=None):
    """[B, d] inputs for `case` on the layer `sd`: masked-out columns N(0,1); masked-in columns
    as the case needs. xsafe: the layer's ok[1] (the GPU tests read it from the packed image);
    default: recomputed in float64 from the folded state dict."""
    gen = torch.Generator().manual_seed(seed * 104729 + B)
    mask = sd["mask"]
    d = mask.numel()
    inn = mask > 0
    n_in = int(inn.sum())
    x = torch.randn(B, d, generator=gen)
    if case in ("plain", "wmax"):
        x = x * 1.5
    elif case in ("edge", "edge_pos"):
        xs = (xsafe_f64(sd) if xsafe is None else float(xsafe)) * (1 - 1e-6)
        v = xs * (0.25 + 0.75 * torch.rand(B, 1, generator=gen, dtype=torch.float64))
        v[0] = xs
        x[:, inn] = v.float().expand(B, n_in)
        assert float(x[:, inn].abs().max()) < xs / (1 - 1e-6)
    else:  # binade, binade_bal, cancel, tiny, lower: positive, one binade around 1
        x[:, inn] = 0.5 + 1.5 * torch.rand(B, n_in, generator=gen)
    return x.float()


# ---- the pack's arithmetic in float64 -------------------------------------------------------------
def fold(sd, n, p=""):
    """(W1', b1', W2', b2', W3, b3) of net `n`: BatchNorm folded in float64 and rounded to fp32,
    as mlp_weight / mlp_bias (csrc/nfx_pack.h) do."""
    eps = float(np.float32(1e-5))
    g = lambda k: sd[p + n + k].double()
    out = []
    for lin, bn in (("0", "1"), ("3", "4")):
        a = g(bn + ".weight") / torch.sqrt(g(bn + ".running_var") + eps)
        out.append((a[:, None] * g(lin + ".weight")).float())
        out.append((a * (g(lin + ".bias") - g(bn + ".running_mean")) + g(bn + ".bias")).float())
    out += [sd[p + n + "6.weight"].float(), sd[p + n + "6.bias"].float()]
    return out


def xsafe_f64(sd, p=""):
    """ok[1]: (1e30 - max|b1'|) / max row-sum|w1'| over both nets, in float64."""
    rows = max(float(fold(sd, n, p)[0].double().abs().sum(1).max()) for n in NETS)
    bmax = max(float(fold(sd, n, p)[1].double().abs().max()) for n in NETS)
    return (ACT_LIMIT - bmax) / rows if rows > 0 else float("inf")


def lower_edge_loss(sd, p=""):
    """2^-133 * max row-sum|W2'| * max row-sum|W3|, the larger of the two nets, in float64."""
    out = 0.0
    for n in NETS:
        f = fold(sd, n, p)
        out = max(out, BF16_MIN_SUBNORMAL * float(f[2].double().abs().sum(1).max())
                  * float(f[4].double().abs().sum(1).max()))
    return out


def w2_safe_f64(sd, p=""):
    """ok[0] as the pack computes it: W2' finite with every |w| <= 1e6, and the lower-edge loss
    below LOSS_LIMIT."""
    big = all(bool((fold(sd, n, p)[2].abs() <= W2_LIMIT).all()) for n in NETS)
    return big and lower_edge_loss(sd, p) < LOSS_LIMIT


# ---- CPU model of affine_net_split ------------------------------------------------------------------
def _trunc16(x):
    """The fp32 pattern's top 16 bits (split3 / pack_bf16)."""
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def split_act(a):
    """split3 followed by pack_bf16: three truncations, each of the exact fp32 remainder."""
    a0 = _trunc16(a)
    r1 = a - a0
    a1 = _trunc16(r1)
    return a0, a1, _trunc16(r1 - a1)


def split_weight(w):
    """affine_split_pack_kernel: three round-to-nearest bf16 pieces."""
    rne = lambda t: t.to(torch.bfloat16).to(torch.float32)
    w0 = rne(w)
    r1 = w - w0
    w1 = rne(r1)
    return w0, w1, rne(r1 - w1)


def fma_chain(a, w, c):
    """c + sum_k a[:, k] * w[:, k]: a k-ordered fp32 fma chain (exact product, one rounding per
    step). a [B, K], w [O, K], c [B, O]."""
    acc = c.clone().float()
    for k in range(a.shape[1]):
        acc = (acc.double() + a[:, k:k + 1].double() * w[None, :, k].double()).float()
    return acc


PRODUCTS_6 = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0))  # (activation piece, weight piece), into lo
PRODUCTS_3 = ((0, 1), (1, 0))                          # the i + j <= 1 variant


def layer2_split(a, w, b, products=PRODUCTS_6, flush=False):
    """hi = b2 + sum a0 w0 (k-ordered fma chain), lo = the small products, result hi + lo."""
    A, W = split_act(a), split_weight(w)
    if flush:  # a matrix unit that reads subnormal bf16 inputs as zero
        z = lambda t: torch.where(t.abs() < 2.0 ** -126, torch.zeros_like(t), t)
        A, W = tuple(z(t) for t in A), tuple(z(t) for t in W)
    hi = fma_chain(A[0], W[0], b[None, :].expand(a.shape[0], -1))
    lo = torch.zeros_like(hi)
    for i, j in products:
        lo = fma_chain(A[i], W[j], lo)
    return hi + lo


def model_s(sd, x, mode, n="s_net.", **kw):
    """The conditioner's output before the clamp, [B, d], on the folded weights.
    mode "f64": float64 throughout; "f32": k-ordered fp32 fma chains; "split": fp32 chains with
    layer 2 by layer2_split(**kw); "kernel": what the kernel runs — "split" when ok[0] holds
    (w2_safe_f64) and every |x * m| <= xsafe, else "f32" (whole batch: the model has no tiles)."""
    w1, b1, w2, b2, w3, b3 = fold(sd, n)
    xa = (x * sd["mask"]).float()
    if mode == "kernel":
        ok = w2_safe_f64(sd) and bool((xa.abs().double() <= xsafe_f64(sd)).all())
        mode = "split" if ok else "f32"
    if mode == "f64":
        h = torch.relu(xa.double() @ w1.double().T + b1.double())
        h = torch.relu(h @ w2.double().T + b2.double())
        return h @ w3.double().T + b3.double()
    rows = lambda b: b[None, :].expand(x.shape[0], -1)
    h = torch.relu(fma_chain(xa, w1, rows(b1)))
    h = layer2_split(h, w2, b2, **kw) if mode == "split" else fma_chain(h, w2, rows(b2))
    return fma_chain(torch.relu(h), w3, rows(b3)).double()


# ---- the criterion ------------------------------------------------------------------------------------
def error_ratios(got, yard, ref):
    """(mean ratio, max ratio, n): e = |got - ref|, e_ref = |yard - ref| over the elements where
    all three are finite; ratios mean(e) / mean(e_ref) and max(e) / max(e_ref)."""
    got, yard, ref = (np.asarray(t, np.float64).ravel() for t in (got, yard, ref))
    ok = np.isfinite(got) & np.isfinite(yard) & np.isfinite(ref)
    if not ok.any():
        return float("nan"), float("nan"), 0
    e, er = np.abs(got - ref)[ok], np.abs(yard - ref)[ok]
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(e.mean() / er.mean()), float(e.max() / er.max()), int(ok.sum())


def assert_split_criterion(got, yard, ref, what):
    """mean|got - f64| <= 2 mean|fp32 - f64| and max|got - f64| <= 4 max|fp32 - f64|, no absolute
    floor; the finite pattern of `got` must be the yardstick's. Prints the two ratios."""
    g, y, r = (np.asarray(t, np.float64).ravel() for t in (got, yard, ref))
    assert np.array_equal(np.isfinite(g), np.isfinite(y)), f"{what}: finite pattern differs from the fp32 oracle"
    ok = np.isfinite(g) & np.isfinite(r)
    if not ok.any():
        print(f"[split] {what}: no finite element")
        return None
    e, er = np.abs(g - r)[ok], np.abs(y - r)[ok]
    rm = e.mean() / er.mean() if er.mean() > 0 else (0.0 if e.mean() == 0 else float("inf"))
    rx = e.max() / er.max() if er.max() > 0 else (0.0 if e.max() == 0 else float("inf"))
    print(f"[split] {what}: mean err {e.mean():.3g} = {rm:.2f} x fp32 ({er.mean():.3g}), "
          f"max err {e.max():.3g} = {rx:.2f} x fp32 ({er.max():.3g}), n = {int(ok.sum())}")
    assert e.mean() <= 2 * er.mean(), f"{what}: mean err {e.mean():.3g} > 2 x fp32's {er.mean():.3g} ({rm:.2f} x)"
    assert e.max() <= 4 * er.max(), f"{what}: max err {e.max():.3g} > 4 x fp32's {er.max():.3g} ({rx:.2f} x)"
    return rm, rx


def meets_criterion(got, yard, ref):
    rm, rx, n = error_ratios(got, yard, ref)
    return n > 0 and rm <= 2 and rx <= 4
