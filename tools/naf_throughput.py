#!/usr/bin/env python
"""Time per call of NeuralAutoregressiveFlow(4, [64, 64]) and (16, [128, 128]) on one GPU, eval mode:
the fused kernel against the eager torch composite on the same device, both directions.

    python tools/naf_throughput.py [--batches 1024,65536] [--replays 20] [--calls 50] [--activation relu]
                                   [--out FILE.json]

Per model, batch size and direction (inverse = density, forward = sampling): `--replays` timing
windows per route after warm-up, the two routes alternating window by window; a window is one
hipEvent pair around `--calls` fused (`--eager-calls` eager) back-to-back calls, so that it lasts far
longer than an event's resolution, and its time is divided by the number of calls. Reported: median,
min and max over the windows (the spread over the repeats) and samples/s. These are times per CALL
(launch, argument handling and kernel), not kernel times.
The comparator is the same call forced through the layer's torch composite on the same GPU (what a
call outside the kernel family runs under ALLOW_TORCH_FALLBACK, and the only thing the reference's
user can run): one conditioner call for the inverse, `dim` of them for the forward. The weights are
redrawn at Xavier gain 2, so the +-2 clamp of the conditioner is reached. The fused call must be the
faster one in every cell (`all_faster`, and the exit status). Prints one JSON line.

    python tools/naf_throughput.py --train [--batches 1024,65536] [--replays 20] [--calls 20] [--out FILE.json]

`--train` times one NLL step instead, `NormalizingFlowModel([flow]).log_prob(x).mean().backward()` with
the optimizer left out, for (4, [64, 64]) and (16, [64, 64]): the fused backward
(`NeuralAutoregressiveFlow.fused_backward = True`, no composite call) against the composite-recompute
route (the flag off: the fused forward kernel, then the eager DeepMADE and autograd), the same windows
taken in turn, `--calls` steps per window on both routes. The fused step's slowest window must lie
below the composite route's fastest in every cell (`all_below`, and the exit status).

    python tools/naf_throughput.py --wide [--batches 1024,65536] [--replays 20] [--calls 50] [--out FILE.json]

`--wide` times the wide kernel family (`wide_kernel = True`, csrc/nfx_naf_wide*.hip) on the constructor's
default widths, (2, [512, 512, 512]) and (16, [512, 512, 512]), by the same method against the same
comparator. Every window is kept in the result (`fused_ms_windows`, `eager_ms_windows`). A cell holds
when the fused call's slowest window lies below the eager composite's fastest (`all_below`, and the
exit status). `mfma_tflops_from_call_time` is the fp32 MFMA work the kernel executes (padded tiles,
every pass, 4,096 flop per v_mfma_f32_32x32x2_f32) divided by the median time per CALL, so it
understates what the matrix pipe reaches inside the kernel.
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

MODELS = [(4, [64, 64]), (16, [128, 128])]
WIDE_MODELS = [(2, [512, 512, 512]), (16, [512, 512, 512])]


def wide_mfma_flop(d, hidden, B, direction):
    """fp32 MFMA flop one wide-kernel call executes: per 32-row tile and conditioner pass, 4 (d <= 8) or
    8 k-steps per out tile of the first layer and 16 per (out tile, k tile) pair above it, the output
    layer being one out tile; one pass for the inverse, d for the forward."""
    nt = [(w + 31) // 32 for w in hidden]
    mfma = nt[0] * (4 if d <= 8 else 8) + sum(16 * a * b for a, b in zip(nt[1:], nt[:-1])) + 16 * nt[-1]
    return 4096 * mfma * ((B + 31) // 32) * (d if direction == "forward" else 1)


def make_flow(d, hidden, activation, device):
    flow = nfs_amd.NeuralAutoregressiveFlow(d, hidden, activation=activation, dropout=0.0)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in flow.conditioner.network.modules():
            if isinstance(m, torch.nn.Linear):
                fan_out, fan_in = m.weight.shape
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 2.0 * (2.0 / (fan_in + fan_out)) ** 0.5)
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
    return flow.to(device).eval()


def window(fn, calls):
    """Milliseconds per call of `calls` back-to-back calls inside one event pair."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def time_alternating(fused, eager, warmup, replays, calls, eager_calls):
    """([fused ms per call], [eager ms per call]) over `replays` windows each, taken in turn."""
    with torch.no_grad():
        for _ in range(warmup):
            fused()
            eager()
        torch.cuda.synchronize()
        ms, ems = [], []
        for _ in range(replays):
            ms.append(window(fused, calls))
            ems.append(window(eager, eager_calls))
    return ms, ems


TRAIN_MODELS = [(4, [64, 64]), (16, [64, 64])]


def train(a, dev):
    """One NLL step per call: the fused backward against the composite recompute."""
    rows = []
    for d, hidden in TRAIN_MODELS:
        flow = make_flow(d, hidden, a.activation, dev)
        plain = nfs_amd.NormalizingFlowModel([copy.deepcopy(flow)]).to(dev)
        flow.fused_backward = True
        fused = nfs_amd.NormalizingFlowModel([flow]).to(dev)
        for B in [int(b) for b in a.batches.split(",")]:
            x = 1.5 * torch.randn(B, d, generator=torch.Generator().manual_seed(B)).to(dev)

            def step(model):
                model.zero_grad(set_to_none=True)
                (-model.log_prob(x).mean()).backward()

            nfs_amd.reset_stats()
            step(fused)
            assert nfs_amd.STATS["torch"] == 0 and nfs_amd.STATS["hip"] >= 2, nfs_amd.STATS
            nfs_amd.reset_stats()
            step(plain)
            assert nfs_amd.STATS["torch"] == 1, nfs_amd.STATS
            agree = max(float((p.grad - q.grad).abs().max() / q.grad.abs().max().clamp_min(1e-30))
                        for p, q in zip(fused.parameters(), plain.parameters()))
            for _ in range(a.warmup):
                step(fused)
                step(plain)
            torch.cuda.synchronize()
            ms, ems = [], []
            for _ in range(a.replays):
                ms.append(window(lambda: step(fused), a.calls))
                ems.append(window(lambda: step(plain), a.calls))
            med, emed = statistics.median(ms), statistics.median(ems)
            rows.append({"dim": d, "hidden_dims": hidden, "B": B, "fused_ms_median": med, "fused_ms_min": min(ms),
                         "fused_ms_max": max(ms), "composite_ms_median": emed, "composite_ms_min": min(ems),
                         "composite_ms_max": max(ems), "fused_speedup_over_composite": emed / med,
                         "fused_slowest_below_composite_fastest": max(ms) < min(ems),
                         "max_relative_gradient_difference": agree})
            print(f"[naf train] ({d}, {hidden}) B={B}: fused backward {med:.3f} ms (min {min(ms):.3f}, max "
                  f"{max(ms):.3f}), composite recompute {emed:.3f} ms (min {min(ems):.3f}, max {max(ems):.3f}); fused is "
                  f"{emed / med:.1f}x; gradients differ by {agree:.1e} relative", file=sys.stderr, flush=True)
    res = {"models": [f"NeuralAutoregressiveFlow({d}, {h}, activation={a.activation!r})" for d, h in TRAIN_MODELS],
           "workload": "one NLL step: (-NormalizingFlowModel([flow]).log_prob(x).mean()).backward(), no optimizer",
           "device": torch.cuda.get_device_name(0), "replays": a.replays, "steps_per_window": a.calls,
           "all_below": all(r["fused_slowest_below_composite_fastest"] for r in rows), "results": rows}
    return res, res["all_below"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,65536")
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--eager-calls", type=int, default=5)
    ap.add_argument("--activation", default="relu")
    ap.add_argument("--out", default=None)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--wide", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.train:
        res, ok = train(a, dev)
        return finish(res, ok, a.out)
    rows = []
    models = WIDE_MODELS if a.wide else MODELS
    for d, hidden in models:
        flow = make_flow(d, hidden, a.activation, dev)
        flow.wide_kernel = a.wide
        eager = copy.deepcopy(flow)
        eager._torch_only = lambda: True  # every call takes the torch composite route
        for B in [int(b) for b in a.batches.split(",")]:
            x = 1.5 * torch.randn(B, d, generator=torch.Generator().manual_seed(B)).to(dev)
            for name, call, ecall in (("inverse", flow.inverse, eager.inverse),
                                      ("forward", flow.forward, eager.forward)):
                nfs_amd.reset_stats()
                ms, ems = time_alternating(lambda: call(x), lambda: ecall(x), a.warmup, a.replays, a.calls,
                                           a.eager_calls)
                n_fused, n_eager = (a.warmup + a.replays * a.calls), (a.warmup + a.replays * a.eager_calls)
                assert nfs_amd.STATS == {"hip": n_fused, "torch": n_eager}, nfs_amd.STATS
                med, emed = statistics.median(ms), statistics.median(ems)
                with torch.no_grad():
                    agree = float((call(x)[0] - ecall(x)[0]).abs().max())
                rows.append({"dim": d, "hidden_dims": hidden, "B": B, "direction": name, "fused_ms_median": med,
                             "fused_ms_min": min(ms), "fused_ms_max": max(ms),
                             "fused_samples_per_s": B / (med * 1e-3), "eager_ms_median": emed,
                             "eager_ms_min": min(ems), "eager_ms_max": max(ems),
                             "eager_samples_per_s": B / (emed * 1e-3), "fused_speedup_over_eager": emed / med,
                             "fused_is_faster": med < emed, "max_abs_difference": agree})
                if a.wide:
                    rows[-1].update({"fused_slowest_below_eager_fastest": max(ms) < min(ems),
                                     "mfma_tflops_from_call_time": wide_mfma_flop(d, hidden, B, name) / (med * 1e9),
                                     "fused_ms_windows": ms, "eager_ms_windows": ems})
                print(f"[naf] ({d}, {hidden}) B={B} {name}: fused {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}), "
                      f"eager composite {emed:.3f} ms (min {min(ems):.3f}, max {max(ems):.3f}); fused is "
                      f"{emed / med:.1f}x; outputs differ by {agree:.1e}", file=sys.stderr, flush=True)
    res = {"models": [f"NeuralAutoregressiveFlow({d}, {h}, activation={a.activation!r})" for d, h in models],
           "device": torch.cuda.get_device_name(0), "replays": a.replays, "calls_per_window": a.calls,
           "eager_calls_per_window": a.eager_calls,
           "all_faster": all(r["fused_ms_median"] < r["eager_ms_median"] for r in rows), "results": rows}
    if a.wide:
        res["all_below"] = all(r["fused_slowest_below_eager_fastest"] for r in rows)
        return finish(res, res["all_below"], a.out)
    return finish(res, res["all_faster"], a.out)


def finish(res, ok, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
