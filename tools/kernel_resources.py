#!/usr/bin/env python3
"""Register, LDS, scratch and code-size table of every gfx950 kernel in the objects under pinot_amd/csrc/ (CSV on stdout,
sorted by mangled name). Reads code-object metadata and symbol sizes only; two builds with equal tables hold the same
kernels. Usage: python tools/kernel_resources.py [csrc-dir] > profiles/kernel_resources.csv"""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
FIELDS = ["vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size"]


def run(tool, *args, cwd=None):
    cmd = [os.path.join(LLVM, tool)] + list(args)
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def kernels(obj):
    """(name, fields..., code_bytes) of every kernel in the gfx950 code object bundled in `obj`."""
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, os.path.basename(obj))
        os.symlink(os.path.abspath(obj), local)
        run("llvm-objdump", "--offloading", local, cwd=tmp)  # writes <obj>.<n>.hipv4-amdgcn-amd-amdhsa--gfx950
        rows = []
        for co in glob.glob(local + ".*gfx950*"):
            syms = run("llvm-readelf", "-sW", co)
            size = {m.group(2): int(m.group(1)) for m in
                    re.finditer(r"^\s*\d+:\s+\S+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)$", syms, re.M)}
            first = len(rows)
            for k in re.split(r"\n\s+- \.agpr_count:", run("llvm-readelf", "--notes", co))[1:]:
                val = lambda f: re.search(r"^\s+\.%s:\s+(\S+)$" % f, k, re.M).group(1)
                rows.append([val("name")] + [val(f) for f in FIELDS] + [str(size[val("name")])])
            descriptors = len(set(re.findall(r"\s(\S+\.kd)$", syms, re.M)))  # one kernel descriptor symbol per kernel
            found = len(rows) - first
            assert found == descriptors, "%s: %d kernels in the notes, %d descriptors" % (obj, found, descriptors)
        return rows


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "..", "pinot_amd", "csrc")
    rows = sorted(r for o in sorted(glob.glob(os.path.join(csrc, "*.o"))) for r in kernels(o))
    print(",".join(["name"] + FIELDS + ["code_bytes"]))
    for r in rows:
        print(",".join(r))
