"""Record the output bits of the streaming affine kernels for tests/test_gpu_affine_split_bits.py.

    python tools/record_split_bits.py [--out tests/golden/g19_affine_split_bits.json]

Run it on the GPU with the library whose bits are to be pinned (NFX_LIB=... selects another
build). Every case of the test runs twice under the streaming policy: as the one-launch chain
(affine_schain_kernel) and as per-layer launches (affine_coupling_kernel, chains disabled). A
row's bits depend only on its own 32-row tile, so the two — which cut the batch into workgroups
differently, as another CU count would — must give equal digests; the file records whether they
did ("per_layer_equal"), and the per-layer digests where they did not.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "normalizing-flows-study_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import test_gpu_affine_split_bits as T  # noqa: E402
from nfs_amd.flows import coupling  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", T.GOLDEN))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec, per_layer_diff = {}, {}
    for case in T.cases():
        out = T.run_case(case, dev)
        rec[case[0]] = {k: {"sha256": T.digest(t), "shape": list(t.shape), "head": T.head_hex(t)}
                        for k, t in out.items()}
        if case[1] == "g2-layer0":
            continue  # already both kernels
        keep = coupling.CHAIN_MAX_B
        coupling.CHAIN_MAX_B = 0  # per-layer launches
        try:
            pl = T.run_case(case, dev)
        finally:
            coupling.CHAIN_MAX_B = keep
        d = {k: T.digest(t) for k, t in pl.items() if T.digest(t) != rec[case[0]][k]["sha256"]}
        if d:
            per_layer_diff[case[0]] = d
        print(f"{case[0]}: {'chain == per-layer' if not d else 'per-layer DIFFERS: ' + ', '.join(d)}", flush=True)
    doc = {"device": torch.cuda.get_device_name(0),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count,
           "per_layer_equal": not per_layer_diff, "per_layer_digests_where_different": per_layer_diff,
           "cases": rec}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out}: {len(rec)} cases, per_layer_equal={not per_layer_diff}")


if __name__ == "__main__":
    main()
