#!/usr/bin/env python
"""Time per call of ResidualFlow(2, 64) on one GPU: the fused kernel against the eager torch
composite on the same device, both directions.

    python tools/residual_throughput.py [--batches 65536] [--replays 20] [--activation relu]
                                        [--lipschitz 0.9] [--out FILE.json]
    python tools/residual_throughput.py --train [--batches 65536,1048576]   # -> profiles/residual_train.json

Per batch size and direction (inverse = density, forward = sampling): hipEvent time of each of
`--replays` calls after warm-up (median and min) and samples/s. The comparator is the same call
forced through the layer's torch composite on the same GPU (what a call outside the kernel family
runs under ALLOW_TORCH_FALLBACK): a fixed-point loop with one host sync per iteration, and the
closed-form Jacobian as batched matmuls. The weights are redrawn at Xavier gain 1, so the spectral
normalisation engages on every layer. Prints one JSON line.

`--train` times one NLL step (`-model.log_prob(x).mean().backward()`, eval mode, no optimizer) with
the fused backward kernels (`fused_backward = True`) against the composite-recompute route of the
same build (the default), alternating the two routes `--rounds` times in one process: per round and
route the median hipEvent time per step after warm-up.
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
    """One NLL step of ResidualFlow(d, H) in eval mode: the fused backward against the composite
    recompute (the default route), alternated in the same process."""
    dev = torch.device("cuda:0")
    d, H = a.dim, a.hidden
    rows = []
    for B in [int(b) for b in (a.batches or "65536,1048576").split(",")]:
        x = 1.5 * torch.randn(B, d, generator=torch.Generator().manual_seed(B)).to(dev)
        models = {}
        for name, fused in (("fused", True), ("composite", False)):
            flow = make_flow(d, H, a.activation, a.lipschitz, dev)
            flow.fused_backward = fused
            models[name] = nfs_amd.NormalizingFlowModel([flow]).to(dev).eval()
        row = {"B": B, "fused_step_ms": [], "composite_step_ms": []}
        for _ in range(a.rounds):
            for name, replays in (("fused", a.replays), ("composite", a.eager_replays)):
                model = models[name]

                def step():
                    model.zero_grad(set_to_none=True)
                    (-model.log_prob(x).mean()).backward()

                nfs_amd.reset_stats()
                ms = time_steps(step, a.warmup if name == "fused" else 1, replays)
                steps = replays + (a.warmup if name == "fused" else 1)
                assert nfs_amd.STATS["torch"] == (0 if name == "fused" else steps), nfs_amd.STATS
                row[f"{name}_step_ms"].append(statistics.median(ms))
        fms = time_calls(lambda: models["fused"].flows[0].inverse(x), a.warmup, a.replays)
        row["fused_forward_ms_median"] = statistics.median(fms)
        row["fused_faster_in_every_pair"] = all(f < c for f, c in zip(row["fused_step_ms"], row["composite_step_ms"]))
        row["fused_speedup_over_composite"] = statistics.median(row["composite_step_ms"]) \
            / statistics.median(row["fused_step_ms"])
        rows.append(row)
        print(f"[residual train] B={B}: fused step {row['fused_step_ms']} ms (forward alone "
              f"{row['fused_forward_ms_median']:.3f} ms), composite step {row['composite_step_ms']} ms; fused is "
              f"{row['fused_speedup_over_composite']:.1f}x", file=sys.stderr, flush=True)
    res = {"model": f"ResidualFlow({d}, {H}, activation={a.activation!r}, lipschitz_constant={a.lipschitz})",
           "device": torch.cuda.get_device_name(0), "workload": "NLL step, eval mode", "rounds": a.rounds,
           "replays": a.replays, "composite_replays": a.eager_replays, "results": rows}
    line = json.dumps(res)
    print(line)
    out = a.out or os.path.join(ROOT, "profiles", "residual_train.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true",
                    help="time one NLL step, fused backward against the composite recompute, at B = 65536 and "
                         "1048576 (or --batches); writes profiles/residual_train.json (or --out)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", default=None)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eager-replays", type=int, default=5)
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--activation", default="relu")
    ap.add_argument("--lipschitz", type=float, default=0.9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.train:
        return train(a)
    a.batches = a.batches or "65536"
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
