"""Per-kernel register usage of one translation unit (hipcc -Rpass-analysis=kernel-resource-usage).
    python tools/kres.py normalizing-flows-study_amd/csrc/<file>.hip [extra hipcc flags]"""
import importlib.util
import os
import re
import subprocess
import sys

here = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location(
    "nfx_build", os.path.join(here, "..", "normalizing-flows-study_amd", "build.py"))
nfx_build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(nfx_build)  # the library's own compiler and flags
cmd = [nfx_build.hipcc()] + nfx_build.CFLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", sys.argv[1],
                                                 "-o", "/tmp/kres.o"] + sys.argv[2:]
r = subprocess.run(cmd, capture_output=True, text=True)
cur = None
rows = []
for line in r.stderr.splitlines():
    m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
    if not m:
        continue
    k, v = m.groups()
    if k == "Function Name":
        cur = {"name": subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()}
        rows.append(cur)
    else:
        cur[k] = v
for c in rows:
    print(f"{c.get('VGPRs','?'):>4} vgpr {c.get('AGPRs','?'):>3} agpr spill {c.get('VGPRs Spill','?'):>3} occ {c.get('Occupancy [waves/SIMD]','?')}  {c['name'][:150]}")
if r.returncode:
    print(r.stderr[-3000:])
