"""Generate tests/golden/g22_naf.npz from the REFERENCE NeuralAutoregressiveFlow itself.

Runs only where the reference checkout is available (NFS_REFERENCE, default /root/reference), on
the CPU in fp32:

    python tests/golden/make_golden_naf.py

The reference package imports `torchdiffeq` at import time; a stub module is injected in-process
(no code used here calls it). Per configuration `c<i>` the file holds plain arrays:

  c<i>.sd.<key>        the state dict after the redraw (tests/naf_cases.redraw)
  c<i>.init.<key>      the state dict of a construction under torch.manual_seed(SEED + i) (c0, c1 only)
  c<i>.m.<k>, c<i>.mask.<k>
                       the degree vectors `conditioner.m[k]` and the list `conditioner.masks`
  c<i>.x               inputs [ROWS, dim]
  c<i>.fwd.y/.ld       eval-mode forward(x);   c<i>.inv.z/.ld   eval-mode inverse(x)
  c<i>.grad.x, c<i>.grad.<parameter name>
                       gradients of mean(0.5 |z|^2 - ld), (z, ld) = inverse(x), in eval mode
  c<i>.train_inv.z/.ld train-mode inverse(x) under torch.manual_seed(DROPOUT_SEED) (the dropout = 0.2
                       configuration only)
  meta                 JSON: the configurations
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

SEED = 2200
DROPOUT_SEED = 2299
ROWS = 24
#          dim, hidden_dims, activation, layer norm, residual, dropout
CONFIGS = [(4, [16, 16, 8], "relu", True, True, 0.0),
           (3, [16, 16], "gelu", True, True, 0.0),
           (2, [12, 12], "elu", True, True, 0.0),          # the d == 2 degree pattern under a residual block
           (3, [16, 8], "leaky_relu", False, True, 0.0),   # unequal widths, no LayerNorm
           (1, [8], "relu", True, True, 0.0),
           (5, [16, 16], "elu", False, False, 0.0),        # equal widths without the residual block
           (3, [16, 16], "gelu", True, True, 0.2)]         # Dropout modules in the Sequential


def import_reference():
    stub = types.ModuleType("torchdiffeq")

    def odeint(*a, **k):
        raise RuntimeError("torchdiffeq is not installed (stub for the reference import)")

    stub.odeint = odeint
    sys.modules.setdefault("torchdiffeq", stub)
    sys.dont_write_bytecode = True
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from src.flows.advanced.neural_autoregressive_flow import NeuralAutoregressiveFlow
    return NeuralAutoregressiveFlow


def main():
    from naf_cases import make_inputs, redraw
    Ref = import_reference()
    arrs, meta = {}, []
    for i, (d, hidden, act, ln, res, dropout) in enumerate(CONFIGS):
        p = f"c{i}."
        torch.manual_seed(SEED + i)
        flow = Ref(d, hidden_dims=list(hidden), activation=act, use_layer_norm=ln, use_residual=res, dropout=dropout)
        if i < 2:
            for k, v in flow.state_dict().items():
                arrs[p + "init." + k] = v.numpy().copy()
        for k, v in flow.conditioner.m.items():
            arrs[p + f"m.{k}"] = np.asarray(v).astype(np.int64)
        for k, v in enumerate(flow.conditioner.masks):
            arrs[p + f"mask.{k}"] = v.numpy().copy()
        redraw(flow, SEED + 50 + i)
        for k, v in flow.state_dict().items():
            arrs[p + "sd." + k] = v.numpy().copy()
        x = make_inputs(ROWS, d, seed=40 + i)
        arrs[p + "x"] = x.numpy().copy()

        flow.eval()
        with torch.no_grad():
            y, ld = flow.forward(x)
            z, li = flow.inverse(x)
        arrs[p + "fwd.y"], arrs[p + "fwd.ld"] = y.numpy().copy(), ld.numpy().copy()
        arrs[p + "inv.z"], arrs[p + "inv.ld"] = z.numpy().copy(), li.numpy().copy()
        params = flow.conditioner(x).detach()
        clamped = float((params.abs() == 2.0).float().mean())

        flow.zero_grad()
        xr = x.clone().requires_grad_(True)
        zg, lg = flow.inverse(xr)
        (0.5 * (zg * zg).sum(dim=1) - lg).mean().backward()
        arrs[p + "grad.x"] = xr.grad.numpy().copy()
        for k, prm in flow.named_parameters():
            arrs[p + "grad." + k] = prm.grad.numpy().copy()
        flow.zero_grad()

        if dropout > 0:
            flow.train()
            torch.manual_seed(DROPOUT_SEED)
            with torch.no_grad():
                zt, lt = flow.inverse(x)
            arrs[p + "train_inv.z"], arrs[p + "train_inv.ld"] = zt.numpy().copy(), lt.numpy().copy()
            assert not torch.equal(zt, z)
        meta.append({"dim": d, "hidden_dims": list(hidden), "activation": act, "use_layer_norm": ln,
                     "use_residual": res, "dropout": dropout, "seed": SEED + i, "dropout_seed": DROPOUT_SEED,
                     "clamped_share": clamped})
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(HERE, "g22_naf.npz")
    np.savez_compressed(out, **arrs)
    print(f"wrote {out}: {os.path.getsize(out)} bytes, {len(arrs)} arrays")
    print([round(m["clamped_share"], 3) for m in meta])


if __name__ == "__main__":
    main()
