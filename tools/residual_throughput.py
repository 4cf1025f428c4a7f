#!/usr/bin/env python
"""Time per call of ResidualFlow(2, 64) on one GPU: the fused kernel against the eager torch
composite on the same device, both directions.

    python tools/residual_throughput.py [--batches 65536] [--replays 20] [--activation relu]
                                        [--lipschitz 0.9] [--out FILE.json]

Per batch size and direction (inverse = density, forward = sampling): hipEvent time of each of
`--replays` calls after warm-up (median and min) and samples/s. The comparator is the same call
forced through the layer's torch composite on the same GPU (what a call outside the kernel family
runs under ALLOW_TORCH_FALLBACK): a fixed-point loop with one host sync per iteration, and the
closed-form Jacobian as batched matmuls. The weights are redrawn at Xavier gain 1, so the spectral
normalisation engages on every layer. Prints one JSON line.
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

import nfs_amd  # noqa: E402


def make_flow(d, H, activation, lipschitz, device):
    flow = nfs_amd.ResidualFlow(d, H, lipschitz_constant=lipschitz, activation=activation)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for layer in flow.residual_block.layers():
            lin = layer.module
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="65536")
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eager-replays", type=int, default=5)
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--activation", default="relu")
    ap.add_argument("--lipschitz", type=float, default=0.9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    d, H = a.dim, a.hidden
    flow = make_flow(d, H, a.activation, a.lipschitz, dev)
    eager = copy.deepcopy(flow)  # the same weights and the same u, v
    eager._torch_only = lambda: True  # every call takes the torch composite route
    rows = []
    for B in [int(b) for b in a.batches.split(",")]:
        x = 1.5 * torch.randn(B, d, generator=torch.Generator().manual_seed(B)).to(dev)
        for name, call, ecall in (("inverse", flow.inverse, eager.inverse), ("forward", flow.forward, eager.forward)):
            nfs_amd.reset_stats()
            ms = time_calls(lambda: call(x), a.warmup, a.replays)
            assert nfs_amd.STATS["torch"] == 0, nfs_amd.STATS
            nfs_amd.reset_stats()
            ems = time_calls(lambda: ecall(x), 2, a.eager_replays)
            assert nfs_amd.STATS["hip"] == 0, nfs_amd.STATS
            med, emed = statistics.median(ms), statistics.median(ems)
            with torch.no_grad():
                agree = float((call(x)[0] - ecall(x)[0]).abs().max())
            rows.append({"B": B, "direction": name, "fused_ms_median": med, "fused_ms_min": min(ms),
                         "fused_samples_per_s": B / (med * 1e-3), "eager_ms_median": emed, "eager_ms_min": min(ems),
                         "eager_samples_per_s": B / (emed * 1e-3), "fused_speedup_over_eager": emed / med,
                         "max_abs_difference": agree})
            print(f"[residual] B={B} {name}: fused {med:.3f} ms (min {min(ms):.3f}), eager composite {emed:.3f} ms "
                  f"(min {min(ems):.3f}); fused is {emed / med:.1f}x; outputs differ by {agree:.1e}",
                  file=sys.stderr, flush=True)
    res = {"model": f"ResidualFlow({d}, {H}, activation={a.activation!r}, lipschitz_constant={a.lipschitz})",
           "device": torch.cuda.get_device_name(0), "replays": a.replays, "eager_replays": a.eager_replays,
           "results": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
