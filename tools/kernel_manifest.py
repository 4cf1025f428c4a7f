"""One line per gfx950 kernel of csrc/*.hip: mangled name, sha256 of its instruction encodings, and
its register / LDS / scratch sizes. Two trees whose manifests are equal run the same device code.
    python tools/kernel_manifest.py [--jobs N] [file.hip ...] > manifest.txt
Hashes and tabulates only; needs no GPU. Exit status 1 if a kernel emitted by several translation
units differs between them."""
import argparse
import concurrent.futures as cf
import glob
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "normalizing-flows-study_amd")
_spec = importlib.util.spec_from_file_location("nfx_build", os.path.join(ROOT, "build.py"))
nfx_build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(nfx_build)

LLVM = os.path.join(os.path.dirname(os.path.realpath(nfx_build.hipcc())), "..", "llvm", "bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size",
          ".private_segment_fixed_size")


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd[:1] + cmd[-3:])} failed:\n{r.stderr[-4000:]}")
    return r.stdout


def manifest_of(src, tmp):
    """{mangled name: (digest, resource numbers...)} for the kernels of one translation unit."""
    obj = os.path.join(tmp, os.path.basename(src)[:-4] + ".o")
    run([nfx_build.hipcc()] + nfx_build.CFLAGS
        + ["--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", obj])
    # Notes: the kernels are the "  - .key: v" items of amdhsa.kernels, their fields at indent 4.
    kernels, cur = {}, None
    for line in run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj]).splitlines():
        m = re.match(r"^(  - |    )(\.\w+): +(\S+)$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is not None:
            cur[m.group(2)] = m.group(3)
            if ".name" in cur:
                kernels[cur[".name"]] = cur
    # Disassembly: "<name>:" opens a function; each instruction ends in "// address: words".
    digests, h = {}, None
    for line in run([os.path.join(LLVM, "llvm-objdump"), "-d", obj]).splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            h = digests[m.group(1)] = hashlib.sha256()
            continue
        m = re.search(r"// [0-9A-Fa-f]+: ((?:[0-9A-Fa-f]{8} ?)+)$", line)
        if m and h is not None:
            h.update(m.group(1).strip().upper().encode() + b"\n")
    return {n: (digests[n].hexdigest(),) + tuple(k.get(f, "?") for f in FIELDS)
            for n, k in kernels.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 4))
    ap.add_argument("srcs", nargs="*")
    a = ap.parse_args()
    srcs = a.srcs or sorted(glob.glob(os.path.join(nfx_build.CSRC, "*.hip")))
    rows, clash = {}, False
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(min(16, a.jobs)) as ex:
        for src, m in zip(srcs, ex.map(lambda s: manifest_of(s, tmp), srcs)):
            for name, row in m.items():
                if rows.setdefault(name, row) != row:
                    clash = True
                    print(f"DIFFERS between units: {name} (again in {os.path.basename(src)})",
                          file=sys.stderr)
    for name in sorted(rows):
        d, *nums = rows[name]
        print(name, d, *(f"{f[1:]}={v}" for f, v in zip(FIELDS, nums)))
    print(f"{len(rows)} kernels from {len(srcs)} units", file=sys.stderr)
    return 1 if clash else 0


if __name__ == "__main__":
    sys.exit(main())
