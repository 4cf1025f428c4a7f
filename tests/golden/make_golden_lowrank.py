"""Generate tests/golden/g23_lowrank.npz from the REFERENCE PlanarFlow, RadialFlow and SylvesterFlow.

Runs only where the reference checkout is available (NFS_REFERENCE, default /root/reference), on
the CPU in fp32:

    python tests/golden/make_golden_lowrank.py

The reference package imports `torchdiffeq` at import time; a stub module is injected in-process
(no code used here calls it). Per configuration `c<i>` the file holds plain arrays:

  c<i>.sd.<key>        the state dict after the redraw (tests/lowrank_cases.redraw)
  c<i>.init.<key>      the state dict of a construction under torch.manual_seed(SEED + i)
  c<i>.x               inputs [ROWS, dim]
  c<i>.fwd.y/.ld       eval-mode forward(x)
  c<i>.inv.z/.ld       eval-mode inverse(x) computed ONE ROW AT A TIME: with one row the
                       reference's batch-global stopping test is the per-sample one of nfs_amd
  c<i>.grad.x, c<i>.grad.<parameter name>
                       gradients of mean(0.5 |y|^2 - ld), (y, ld) = forward(x)
  meta                 JSON: the configurations and each contraction bound
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

SEED = 2300
ROWS = 24
#          kind, dim, num_householder, num_transforms, bound
CONFIGS = [("planar", 1, None, None, 0.6), ("planar", 3, None, None, 0.6), ("planar", 12, None, None, 0.4),
           ("radial", 1, None, None, 0.6), ("radial", 3, None, None, 0.6), ("radial", 12, None, None, 0.4),
           ("sylvester", 2, 2, 2, 0.6), ("sylvester", 3, 8, 1, 0.6), ("sylvester", 5, 3, 3, 0.4),
           ("sylvester", 8, 8, None, 0.6), ("sylvester", 12, 4, 5, 0.6)]


def import_reference():
    stub = types.ModuleType("torchdiffeq")

    def odeint(*a, **k):
        raise RuntimeError("torchdiffeq is not installed (stub for the reference import)")

    stub.odeint = odeint
    sys.modules.setdefault("torchdiffeq", stub)
    sys.dont_write_bytecode = True
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from src.flows.advanced.planar_flow import PlanarFlow
    from src.flows.advanced.radial_flow import RadialFlow
    from src.flows.advanced.sylvester_flow import SylvesterFlow
    return types.SimpleNamespace(PlanarFlow=PlanarFlow, RadialFlow=RadialFlow, SylvesterFlow=SylvesterFlow)


def main():
    from lowrank_cases import construct, contraction_bound, make_inputs, redraw
    ref = import_reference()
    arrs, meta = {}, []
    for i, (kind, d, nh, nt, bound) in enumerate(CONFIGS):
        p = f"c{i}."
        torch.manual_seed(SEED + i)
        flow = construct(kind, d, num_householder=nh if nh is not None else 8, num_transforms=nt, module=ref)
        for k, v in flow.state_dict().items():
            arrs[p + "init." + k] = v.numpy().copy()
        redraw(flow, SEED + 50 + i, bound)
        for k, v in flow.state_dict().items():
            arrs[p + "sd." + k] = v.numpy().copy()
        x = make_inputs(ROWS, d, seed=60 + i)
        arrs[p + "x"] = x.numpy().copy()
        flow.eval()
        with torch.no_grad():
            y, ld = flow.forward(x)
            rows = [flow.inverse(x[r:r + 1]) for r in range(ROWS)]
        arrs[p + "fwd.y"], arrs[p + "fwd.ld"] = y.numpy().copy(), ld.numpy().copy()
        arrs[p + "inv.z"] = torch.cat([z for z, _ in rows]).numpy().copy()
        arrs[p + "inv.ld"] = torch.cat([l for _, l in rows]).numpy().copy()
        flow.zero_grad()
        xr = x.clone().requires_grad_(True)
        yg, lg = flow.forward(xr)
        (0.5 * (yg * yg).sum(dim=1) - lg).mean().backward()
        arrs[p + "grad.x"] = xr.grad.numpy().copy()
        for k, prm in flow.named_parameters():
            arrs[p + "grad." + k] = prm.grad.numpy().copy()
        meta.append({"kind": kind, "dim": d, "num_householder": nh, "num_transforms": nt, "seed": SEED + i,
                     "bound": contraction_bound(flow)})
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(HERE, "g23_lowrank.npz")
    np.savez_compressed(out, **arrs)
    print(f"wrote {out}: {os.path.getsize(out)} bytes, {len(arrs)} arrays")


if __name__ == "__main__":
    main()
