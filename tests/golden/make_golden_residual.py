"""Generate tests/golden/g21_residual.npz from the REFERENCE ResidualFlow itself.

Runs only where the reference checkout is available (NFS_REFERENCE, default /root/reference), on
the CPU in fp32:

    python tests/golden/make_golden_residual.py

The reference package imports `torchdiffeq` at import time; a stub module is injected in-process
(no code used here calls it). Per configuration `c<i>` the file holds plain arrays:

  c<i>.sd.<key>        the state dict after the redraw (tests/residual_cases.redraw)
  c<i>.init.<key>      the state dict of a construction under torch.manual_seed(SEED + i) (c0, c1 only)
  c<i>.x               inputs [ROWS, dim]
  c<i>.fwd.y/.ld       eval-mode forward(x);   c<i>.inv.z/.ld   eval-mode inverse(x)
  c<i>.grad.x, c<i>.grad.<parameter name>
                       gradients of mean(0.5 |z|^2 - ld), (z, ld) = inverse(x), in eval mode with
                       tol = 0 and max_iter = GRAD_ITERS: every row then runs all the iterations, so
                       the per-sample stopping rule of nfs_amd and the reference's batch-global one
                       unroll the same graph
  c<i>.train_fwd.uv, c<i>.train_inv.uv
                       the `u` and `v` buffers, concatenated in state-dict order, after ONE
                       train-mode forward(x), and after ONE train-mode inverse(x), each from the
                       redrawn state
  meta                 JSON: the configurations, and sigma / c per layer

Two regimes: `engaged` (weights at Xavier gain 1: sigma > c on every layer) and not engaged (gain
0.1, the constructor's: sigma < c on every layer); in both |sigma - c| > 1e-3 c, asserted here, so
no fp32 reordering flips the branch.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("NFS_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "normalizing-flows-study_amd"))

SEED = 2100
ROWS = 24
GRAD_ITERS = 8
#          dim, H, activation, engaged
CONFIGS = [(2, 8, "relu", True), (3, 16, "elu", False), (4, 8, "leaky_relu", True),
           (2, 16, "tanh", False), (3, 8, "tanh", True), (4, 16, "relu", False)]


def import_reference():
    stub = types.ModuleType("torchdiffeq")

    def odeint(*a, **k):
        raise RuntimeError("torchdiffeq is not installed (stub for the reference import)")

    stub.odeint = odeint
    sys.modules.setdefault("torchdiffeq", stub)
    sys.dont_write_bytecode = True
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from src.flows.advanced.residual_flow import ResidualFlow
    return ResidualFlow


def reference_sigmas(flow):
    """[(sigma, c)] per layer, with the reference's own fp32 expressions."""
    out = []
    for layer in (flow.residual_block.layer1, flow.residual_block.layer2, flow.residual_block.layer3):
        w = layer.module.weight.detach()
        v = torch.nn.functional.normalize(torch.mv(w.t(), layer.u), dim=0)
        u = torch.nn.functional.normalize(torch.mv(w, v), dim=0)
        out.append((float(torch.dot(u, torch.mv(w, v))), float(layer.lipschitz_constant)))
    return out


def main():
    from residual_cases import make_inputs, redraw
    Ref = import_reference()
    arrs, meta = {}, []
    for i, (d, H, act, engaged) in enumerate(CONFIGS):
        p = f"c{i}."
        torch.manual_seed(SEED + i)
        flow = Ref(d, hidden_dim=H, activation=act)
        if i < 2:
            for k, v in flow.state_dict().items():
                arrs[p + "init." + k] = v.numpy().copy()
        redraw(flow, SEED + 50 + i, 1.0 if engaged else 0.1)
        sd = {k: v.clone() for k, v in flow.state_dict().items()}
        for k, v in sd.items():
            arrs[p + "sd." + k] = v.numpy().copy()
        sig = reference_sigmas(flow)
        for s, c in sig:
            assert (s > c) == engaged and abs(s - c) > 1e-3 * c, (i, s, c)
        x = make_inputs(ROWS, d, seed=40 + i)
        arrs[p + "x"] = x.numpy().copy()

        flow.eval()
        y, ld = flow.forward(x)
        z, li = flow.inverse(x)
        arrs[p + "fwd.y"], arrs[p + "fwd.ld"] = y.detach().numpy().copy(), ld.detach().numpy().copy()
        arrs[p + "inv.z"], arrs[p + "inv.ld"] = z.detach().numpy().copy(), li.detach().numpy().copy()
        assert all(torch.equal(sd[k], v) for k, v in flow.state_dict().items())  # eval mode leaves u, v alone

        tol, max_iter = flow.tol, flow.max_iter
        flow.tol, flow.max_iter = 0.0, GRAD_ITERS
        flow.zero_grad()
        xr = x.clone().requires_grad_(True)
        zg, lg = flow.inverse(xr)
        (0.5 * (zg * zg).sum(dim=1) - lg).mean().backward()
        arrs[p + "grad.x"] = xr.grad.numpy().copy()
        for k, prm in flow.named_parameters():
            arrs[p + "grad." + k] = prm.grad.numpy().copy()
        flow.tol, flow.max_iter = tol, max_iter
        flow.zero_grad()

        for name in ("forward", "inverse"):
            flow.load_state_dict(sd)
            flow.train()
            getattr(flow, name)(x)
            uv = [v for k, v in flow.state_dict().items() if k.endswith((".u", ".v"))]
            assert not any(torch.equal(v, sd[k]) for k, v in flow.state_dict().items() if k.endswith((".u", ".v")))
            arrs[p + ("train_fwd.uv" if name == "forward" else "train_inv.uv")] = torch.cat(uv).numpy().copy()
        meta.append({"dim": d, "hidden_dim": H, "activation": act, "engaged": engaged, "seed": SEED + i,
                     "sigma_c": sig, "grad_iters": GRAD_ITERS})
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(HERE, "g21_residual.npz")
    np.savez_compressed(out, **arrs)
    print(f"wrote {out}: {os.path.getsize(out)} bytes, {len(arrs)} arrays")


if __name__ == "__main__":
    main()
