#!/usr/bin/env python
"""Registers, scratch, LDS and occupancy of every kernel of the named sources, from the compiler's own remarks.

    python tools/kernel_resources.py                          # the five raster_*.hip files
    python tools/kernel_resources.py raster_fwd.hip isect.hip
    python tools/kernel_resources.py --against ../other_tree  # only the rows that differ from another checkout

Compiles with the flags of street_crafter_amd/build.py plus -Rpass-analysis=kernel-resource-usage (device pass only,
nothing is written) and prints one row per kernel.  This is how the resource tables of DESIGN.md are made.
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from street_crafter_amd import build as B  # noqa: E402

FIELDS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "waves")]


def resources(tree, src):
    """{demangled kernel name: (sgpr, vgpr, scratch, lds, waves)} of one source file of a checkout."""
    path = os.path.join(tree, "street_crafter_amd", "csrc", src)
    cmd = [B._hipcc(), *B.COMMON_FLAGS, '-DSC_ABI_HASH="0"', "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", path, "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"hipcc failed on {path}:\n{r.stderr}")
    rows, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
            rows[name] = {}
        elif name:
            rows[name][m.group(1)] = m.group(2)
    names = list(rows)
    plain = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    full = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for n, p, f in zip(names, plain, full):
        targs = re.search(re.escape(p.split("::")[-1]) + r"(<.*?>)\(", f)       # template arguments, without the parameters
        out[p.replace("(anonymous namespace)::", "") + (targs.group(1) if targs else "")] = tuple(
            int(rows[n].get(k, -1)) for k, _ in FIELDS)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="*", help="sources under street_crafter_amd/csrc (default: raster_*.hip)")
    ap.add_argument("--against", metavar="OTHER_TREE", help="print only rows that differ from this checkout's")
    a = ap.parse_args()
    files = a.files or sorted(f for f in os.listdir(B.CSRC) if f.startswith("raster_") and f.endswith(".hip"))
    head = f"{'kernel':<84} {'sgpr':>5} {'vgpr':>5} {'scratch':>7} {'lds':>6} {'waves':>5}"
    print(head)
    differ = 0
    for src in files:
        src = os.path.basename(src)
        mine = resources(ROOT, src)
        theirs = resources(os.path.abspath(a.against), src) if a.against else None
        for k in sorted(set(mine) | set(theirs or {})):
            row = lambda v: " ".join(f"{x:>{w}}" for x, w in zip(v, (5, 5, 7, 6, 5))) if v else "absent"
            if theirs is None:
                print(f"{src + ': ' + k:<84} {row(mine.get(k))}")
            elif mine.get(k) != theirs.get(k):
                differ += 1
                print(f"{src + ': ' + k:<84} {row(theirs.get(k))}   (other)\n{'':<84} {row(mine.get(k))}   (this)")
    if a.against:
        print(f"{differ} kernel(s) differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
