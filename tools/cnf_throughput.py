#!/usr/bin/env python
"""Throughput of ContinuousFlow(2, 64) on one GPU: the fused RK4 kernel against the eager torch
composite on the same device.

    python tools/cnf_throughput.py [--batches 4096,1048576] [--replays 20] [--out FILE.json]
    python tools/cnf_throughput.py --train [--batches 4096,65536]     # -> profiles/cnf_train.json

`--train` times one NLL step (forward + backward) with the fused backward kernels
(`ContinuousFlow.fused_backward = True`) against the default route, whose backward recomputes
through the composite, in the same run; it also reports the backward's cost in forwards.

Per batch size and direction (inverse = density, forward = sampling): hipEvent time of each of
`--replays` calls after warm-up (median and min), samples/s, and the achieved fp32 MFMA rate from
the flops the kernel executes in its two H x H products, 2 * 2 H^2 per field evaluation (layer 2 and
the trace product g2 . (C g1)), 4 evaluations per step, against the 157.3 TFLOP/s fp32 MFMA ceiling
DESIGN.md uses. (The per-dimension tangent form of the same trace counts (1 + d) * 2 H^2; that
figure is reported beside it.) The comparator is the same call forced through the
layer's torch composite (the ALLOW_TORCH_FALLBACK route) on the same GPU. The reference's own
figure — 4 k samples/s, BASELINE.md:18, CPU — is quoted as published, not re-measured (its solver
dependency is not part of this project's environment). Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "normalizing-flows-study_amd"))

import nfs_amd  # noqa: E402

PEAK_TF = 157.3
PUBLISHED_REFERENCE_SAMPLES_PER_S = 4000.0  # BASELINE.md:18 (CPU), published, not re-measured


def make_flow(d, H, device):
    flow = nfs_amd.ContinuousFlow(d, H)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for lin in flow.ode_func.linears():
            fan_out, fan_in = lin.weight.shape
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * (2.0 / (fan_in + fan_out)) ** 0.5)
            lin.bias.copy_(0.1 * torch.randn(lin.bias.shape, generator=g))
    return flow.to(device).eval()


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


def time_steps(fn, warmup, replays):
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


def train(a):
    """One NLL step (forward + backward, no optimizer) of ContinuousFlow(d, H): the fused backward
    (fused_backward = True) against the composite recompute (the default route), in the same run."""
    dev = torch.device("cuda:0")
    d, H = a.dim, a.hidden
    rows = []
    for B in [int(b) for b in (a.batches or "4096,65536").split(",")]:
        x = 1.5 * torch.randn(B, d, generator=torch.Generator().manual_seed(B)).to(dev)
        row = {"B": B}
        for name, fused, replays in (("fused", True, a.replays), ("composite", False, a.eager_replays)):
            flow = make_flow(d, H, dev)
            flow.fused_backward = fused
            model = nfs_amd.NormalizingFlowModel([flow]).to(dev)

            def step():
                model.zero_grad(set_to_none=True)
                (-model.log_prob(x).mean()).backward()

            nfs_amd.reset_stats()
            ms = time_steps(step, 1 if not fused else a.warmup, replays)
            assert nfs_amd.STATS["torch"] == (0 if fused else 1 + replays), nfs_amd.STATS
            row[f"{name}_step_ms_median"], row[f"{name}_step_ms_min"] = statistics.median(ms), min(ms)
            if fused:  # the forward alone, for the backward's cost in forwards
                fms = time_calls(lambda: flow.inverse(x), a.warmup, a.replays)
                row["fused_forward_ms_median"] = statistics.median(fms)
                row["fused_backward_in_forwards"] = (row["fused_step_ms_median"] - row["fused_forward_ms_median"]) \
                    / row["fused_forward_ms_median"]
        row["fused_speedup_over_composite"] = row["composite_step_ms_median"] / row["fused_step_ms_median"]
        rows.append(row)
        print(f"[cnf train] B={B}: fused step {row['fused_step_ms_median']:.2f} ms (forward alone "
              f"{row['fused_forward_ms_median']:.2f} ms), composite step {row['composite_step_ms_median']:.1f} ms; "
              f"fused is {row['fused_speedup_over_composite']:.1f}x", file=sys.stderr, flush=True)
    res = {"model": f"ContinuousFlow({d}, {H})", "device": torch.cuda.get_device_name(0), "workload": "NLL step",
           "replays": a.replays, "composite_replays": a.eager_replays, "results": rows}
    line = json.dumps(res)
    print(line)
    out = a.out or os.path.join(ROOT, "profiles", "cnf_train.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true",
                    help="time one NLL step, fused backward against the composite recompute, at B = 4096 and "
                         "65536 (or --batches); writes profiles/cnf_train.json (or --out)")
    ap.add_argument("--batches", default=None)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eager-replays", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.train:
        return train(a)
    a.batches = a.batches or "4096,1048576"
    dev = torch.device("cuda:0")
    d, H = a.dim, a.hidden
    flow = make_flow(d, H, dev)
    eager = make_flow(d, H, dev)
    eager._torch_only = lambda: True  # every call takes the torch composite route
    steps = len(flow.time_grid(torch.tensor([0.0, 1.0]))) - 1
    flop_per_sample = steps * 4 * 2 * 2 * H * H            # executed: layer 2 + the trace product
    tangent_form_flop_per_sample = steps * 4 * (1 + d) * 2 * H * H
    rows = []
    for B in [int(b) for b in a.batches.split(",")]:
        x = 1.5 * torch.randn(B, d, generator=torch.Generator().manual_seed(B)).to(dev)
        for name, call, ecall in (("inverse", flow.inverse, eager.inverse), ("forward", flow.forward, eager.forward)):
            nfs_amd.reset_stats()
            ms = time_calls(lambda: call(x), a.warmup, a.replays)
            assert nfs_amd.STATS["torch"] == 0, nfs_amd.STATS
            med, lo = statistics.median(ms), min(ms)
            row = {"B": B, "direction": name, "fused_ms_median": med, "fused_ms_min": lo,
                   "fused_samples_per_s": B / (med * 1e-3),
                   "fused_mfma_tflops": B * flop_per_sample / (med * 1e-3) / 1e12,
                   "fused_frac_of_fp32_mfma_peak": B * flop_per_sample / (med * 1e-3) / 1e12 / PEAK_TF}
            if not a.no_eager:
                nfs_amd.reset_stats()
                ems = time_calls(lambda: ecall(x), 1, a.eager_replays)
                assert nfs_amd.STATS["hip"] == 0, nfs_amd.STATS
                emed = statistics.median(ems)
                row.update({"eager_ms_median": emed, "eager_samples_per_s": B / (emed * 1e-3),
                            "fused_speedup_over_eager": emed / med})
            rows.append(row)
            print(f"[cnf] B={B} {name}: fused {med:.3f} ms (min {lo:.3f}) = {row['fused_samples_per_s']:.3e} samples/s, "
                  f"{row['fused_mfma_tflops']:.1f} TF ({100 * row['fused_frac_of_fp32_mfma_peak']:.1f} % of {PEAK_TF})"
                  + ("" if a.no_eager else f"; eager composite {row['eager_ms_median']:.1f} ms = "
                     f"{row['eager_samples_per_s']:.3e} samples/s; fused is {row['fused_speedup_over_eager']:.0f}x"),
                  file=sys.stderr, flush=True)
    res = {"model": f"ContinuousFlow({d}, {H})", "device": torch.cuda.get_device_name(0), "steps": steps,
           "field_evaluations": 4 * steps, "flop_per_sample": flop_per_sample,
           "tangent_form_flop_per_sample": tangent_form_flop_per_sample, "fp32_mfma_peak_tflops": PEAK_TF,
           "reference_published_samples_per_s_cpu_not_remeasured": PUBLISHED_REFERENCE_SAMPLES_PER_S,
           "replays": a.replays, "results": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
