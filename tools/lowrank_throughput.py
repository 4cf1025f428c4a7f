#!/usr/bin/env python
"""Time per call of a 16-layer PlanarFlow(16) stack and a 16-layer SylvesterFlow(8) stack on one
GPU, both directions, three routes on the same device:

    python tools/lowrank_throughput.py [--batch 1048576] [--layers 16] [--replays 20] [--out FILE.json]

  stack      the whole stack in ONE launch of lowrank_stack_kernel (what SequentialFlow and
             NormalizingFlowModel run)
  per_layer  the same layers launched one by one (the same kernel with n_layers = 1, the log-det
             accumulated in place): what the stack would cost without the fusion
  eager      the layers' torch composites on the same GPU (what a call outside the kernel family
             runs under ALLOW_TORCH_FALLBACK): a fixed-point loop with one host sync per iteration

hipEvent time of each of `--replays` calls after warm-up (median and min), and the stack's achieved
bytes/s counted as B (2 dim + 1) 4 bytes: x in, z out, the log-det out. The parameters are redrawn
at a contraction bound of 0.6 (tests/lowrank_cases.redraw): at the constructors' initialisation the
layers are nearly the identity and the inverse stops at once. Prints one JSON line.

    python tools/lowrank_throughput.py --train [--batch 1048576] [--layers 16] [--train-replays 3] [--out FILE.json]

times one NLL step instead, `(-NormalizingFlowModel(layers).log_prob(x).mean()).backward()` with no
optimizer, of the same two stacks on two routes of the same build, taken in turn:

  fused      every layer with fused_backward = True: one forward launch that saves only its output, one
             backward launch for the whole stack (csrc/nfx_lowrank_bwd*.hip), one parameter launch per layer
  composite  the default: the forward kernels, then each layer's gradients recomputed through its torch
             composite (autograd unrolled through the fixed-point loop)

and reports every run, so "the fused step is faster in every run" can be read off.
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "normalizing-flows-study_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nfs_amd  # noqa: E402
from lowrank_cases import redraw  # noqa: E402


def time_calls(fn, warmup, replays):
    with torch.no_grad():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(replays):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    return ms


def per_layer(flows, x, direction, bufs, ld):
    ld.zero_()
    cur, k = x, 0
    for f in (flows if direction > 0 else reversed(flows)):
        f._hip_launch_counted(cur, bufs[k], ld, direction, accumulate=True)
        cur, k = bufs[k], k ^ 1
    return cur, ld


def step_ms(model, x):
    """hipEvent milliseconds of one NLL step."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    model.zero_grad(set_to_none=True)
    e0.record()
    (-model.log_prob(x).mean()).backward()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def train(a, dev):
    rows = []
    B = a.batch
    for name, dim, make in STACKS:
        layers = [redraw(make(), 100 + i, 0.6).eval() for i in range(a.layers)]
        plain = nfs_amd.NormalizingFlowModel([copy.deepcopy(f) for f in layers]).to(dev).eval()
        fused = nfs_amd.NormalizingFlowModel([copy.deepcopy(f) for f in layers]).to(dev).eval()
        for f in fused.flows:
            f.fused_backward = True
        x = (1.5 * torch.randn(B, dim, generator=torch.Generator().manual_seed(dim))).to(dev)
        nfs_amd.reset_stats()
        step_ms(fused, x)
        assert nfs_amd.STATS["torch"] == 0, nfs_amd.STATS
        nfs_amd.reset_stats()
        step_ms(plain, x)
        assert nfs_amd.STATS["torch"] == a.layers, nfs_amd.STATS
        agree = max(float((p.grad - q.grad).abs().max() / q.grad.abs().max().clamp_min(1e-30))
                    for p, q in zip(fused.parameters(), plain.parameters()))
        ms, cms = [], []
        for _ in range(a.train_replays):
            ms.append(step_ms(fused, x))
            cms.append(step_ms(plain, x))
        plain.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
        rows.append({"stack": f"{a.layers} x {name}", "B": B, "fused_ms": ms, "composite_ms": cms,
                     "fused_speedup_over_composite": statistics.median(cms) / statistics.median(ms),
                     "fused_slowest_below_composite_fastest": max(ms) < min(cms),
                     "max_relative_gradient_difference": agree})
        print(f"[lowrank train] {a.layers} x {name} B={B}: fused " + " / ".join(f"{m:.3f}" for m in ms) + " ms, composite "
              + " / ".join(f"{m:.1f}" for m in cms) + f" ms; fused is {statistics.median(cms) / statistics.median(ms):.0f}x; "
              f"parameter gradients differ by {agree:.1e} relative (implicit against unrolled)", file=sys.stderr, flush=True)
    return {"workload": "one NLL step: (-NormalizingFlowModel(layers).log_prob(x).mean()).backward(), no optimizer",
            "device": torch.cuda.get_device_name(0), "runs": a.train_replays,
            "all_below": all(r["fused_slowest_below_composite_fastest"] for r in rows), "results": rows}


STACKS = (("PlanarFlow(16)", 16, lambda: nfs_amd.PlanarFlow(16)), ("SylvesterFlow(8)", 8, lambda: nfs_amd.SylvesterFlow(8)))


def finish(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eager-replays", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--train-replays", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.train:
        res = train(a, dev)
        finish(res, a.out)
        return 0 if res["all_below"] else 1
    B = a.batch
    rows = []
    for name, dim, make in STACKS:
        flows = [redraw(make(), 100 + i, 0.6).to(dev).eval() for i in range(a.layers)]
        stack = nfs_amd.SequentialFlow(flows).eval()
        x = (1.5 * torch.randn(B, dim, generator=torch.Generator().manual_seed(dim))).to(dev)
        bufs = [torch.empty_like(x), torch.empty_like(x)]
        ld = torch.empty(B, device=dev)
        traffic = B * (2 * dim + 1) * 4
        for dname, direction in (("forward", 1), ("inverse", -1)):
            call = stack.forward if direction > 0 else stack.inverse
            nfs_amd.reset_stats()
            ms = time_calls(lambda: call(x), a.warmup, a.replays)
            assert nfs_amd.STATS == {"hip": a.warmup + a.replays, "torch": 0}, nfs_amd.STATS
            lms = time_calls(lambda: per_layer(flows, x, direction, bufs, ld), a.warmup, a.replays)
            with torch.no_grad():
                ys, ls = call(x)
                yl, ll = per_layer(flows, x, direction, bufs, ld)
                same = bool(torch.equal(ys, yl) and torch.equal(ls, ll))
                nfs_amd.flows.flow.ALLOW_TORCH_FALLBACK = True
                for f in flows:
                    f._torch_only = lambda: True
                nfs_amd.reset_stats()
                ems = time_calls(lambda: call(x), 1, a.eager_replays)
                assert nfs_amd.STATS["hip"] == 0, nfs_amd.STATS
                agree = float((call(x)[0] - ys).abs().max())
                for f in flows:
                    del f._torch_only
                nfs_amd.flows.flow.ALLOW_TORCH_FALLBACK = False
            med, lmed, emed = statistics.median(ms), statistics.median(lms), statistics.median(ems)
            rows.append({"stack": f"{a.layers} x {name}", "B": B, "direction": dname, "stack_ms_median": med,
                         "stack_ms_min": min(ms), "per_layer_ms_median": lmed, "per_layer_ms_min": min(lms),
                         "eager_ms_median": emed, "eager_ms_min": min(ems), "stack_speedup_over_per_layer": lmed / med,
                         "stack_speedup_over_eager": emed / med, "stack_bytes_per_s": traffic / (med * 1e-3),
                         "stack_equals_per_layer": same, "max_abs_difference_from_eager": agree})
            print(f"[lowrank] {a.layers} x {name} B={B} {dname}: stack {med:.3f} ms (min {min(ms):.3f}), per layer "
                  f"{lmed:.3f} ms (min {min(lms):.3f}), eager {emed:.1f} ms; stack is {lmed / med:.2f}x per-layer, "
                  f"{emed / med:.0f}x eager, {traffic / (med * 1e-3) / 1e9:.1f} GB/s; bit-equal to per-layer: {same}; "
                  f"differs from eager by {agree:.1e}", file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(0), "replays": a.replays, "eager_replays": a.eager_replays,
           "results": rows}
    finish(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
