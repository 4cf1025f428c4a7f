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
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eager-replays", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.batch
    rows = []
    for name, dim, make in (("PlanarFlow(16)", 16, lambda: nfs_amd.PlanarFlow(16)),
                            ("SylvesterFlow(8)", 8, lambda: nfs_amd.SylvesterFlow(8))):
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
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
