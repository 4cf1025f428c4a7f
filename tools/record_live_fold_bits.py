"""Record the output bits of the streaming affine kernels for tests/test_gpu_affine_live_fold.py.

    python tools/record_live_fold_bits.py [--out tests/golden/g20_affine_live_fold_bits.json]

Run it on the GPU with the library whose bits are to be pinned (NFX_LIB=... selects another
build): the one from before the output-layer fold skipped dead outputs. Every case of the test
runs once under the streaming policy, on an all-clean batch and on the batch with the poisoned
tiles; the file holds the sha256 of every output's raw bytes and its first rows as hex.
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

import test_gpu_affine_live_fold as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", T.GOLDEN))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {}
    for case in T.cases():
        out, clean_rows = T.run_case(case, dev)
        for k, t in out.items():
            if k.startswith("poison."):
                c = out["clean." + k[len("poison."):]]
                assert torch.equal(t[clean_rows].view(torch.int32), c[clean_rows].view(torch.int32)), (case[0], k)
        rec[case[0]] = {k: {"sha256": T.digest(t), "shape": list(t.shape), "head": T.head_hex(t)}
                        for k, t in out.items()}
        print(case[0], flush=True)
    doc = {"device": torch.cuda.get_device_name(0),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "cases": rec}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out}: {len(rec)} cases")


if __name__ == "__main__":
    main()
