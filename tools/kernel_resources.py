#!/usr/bin/env python3
"""Registers, scratch and instruction count of every gfx950 kernel in a built libswg.so, and the comparison of two builds.

    python tools/kernel_resources.py seq-align-gpu_amd/libswg.so > mine.tsv
    python tools/kernel_resources.py seq-align-gpu_amd/libswg.so --against parent.tsv [--family swg_diag_dyn_kernel]
                                     [--rename 'Lb0EEv16SwgDiagDynParams$=Ev16SwgDiagDynParams']

A change that adds a template flag to a fill kernel must leave every existing instantiation as it was: same VGPRs, SGPRs,
scratch bytes and instruction count per kernel symbol.  The counts come from the code object itself -- the registers and
the scratch size from its metadata note, the instructions from its disassembly -- not from the compiler's remarks.
--against prints every symbol that differs or is missing on either side and exits 1 if a symbol of the other build
differs or is gone; symbols only this build has are listed as new.  A new template parameter changes the mangled name of
every instantiation, the old ones included: --rename REGEX=TEXT rewrites this build's names before they are matched (the
example takes a trailing `false` flag off swg_diag_dyn_kernel's arguments, so the instantiations with the flag off meet
the other build's).
"""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "lib", "llvm", "bin")


def resources(lib):
    """{kernel symbol: (vgprs, sgprs, scratch bytes, instructions)} over the gfx950 code objects of lib."""
    tmp = tempfile.mkdtemp()
    out = {}
    try:
        copy = os.path.join(tmp, "lib.so")
        shutil.copy(lib, copy)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", copy], stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, check=True, cwd=tmp)
        for co in sorted(glob.glob(copy + ".*gfx950*")):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], stdout=subprocess.PIPE, text=True,
                                   check=True).stdout
            meta = {}
            cur = {}
            for line in notes.splitlines():
                m = re.match(r"\s*-?\s*\.(name|private_segment_fixed_size|sgpr_count|vgpr_count|symbol):\s*(\S+)", line)
                if not m:
                    continue
                key, val = m.group(1), m.group(2).strip("'\"")
                if key == "name" and not val.startswith("_Z") and not val.startswith("swg"):
                    continue                                  # (an argument's name, not a kernel's)
                cur[key] = val
                if key == "vgpr_count":                       # the last of a kernel's keys in the note's order
                    name = cur.get("name")
                    if name:
                        meta[name] = (int(cur["vgpr_count"]), int(cur.get("sgpr_count", 0)),
                                      int(cur.get("private_segment_fixed_size", 0)))
                    cur = {}
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], stdout=subprocess.PIPE, text=True,
                                 check=True).stdout
            name, count = None, {}
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    name = m.group(1)
                    count[name] = 0
                elif name and re.match(r"^\s+[a-z_0-9]+\b.*//", line):
                    count[name] += 1
            for k, (v, s, p) in meta.items():
                out[k] = (v, s, p, count.get(k, 0))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("--against", help="a table this tool printed for another build")
    ap.add_argument("--family", default="", help="only symbols containing this text")
    ap.add_argument("--rename", action="append", default=[], help="REGEX=TEXT applied to this build's symbol names")
    a = ap.parse_args()
    mine = {k: v for k, v in resources(a.lib).items() if a.family in k}
    for r in a.rename:
        pat, _, text = r.partition("=")
        mine = {re.sub(pat, text, k): v for k, v in mine.items()}
    if not a.against:
        for k in sorted(mine):
            print("%s\t%d\t%d\t%d\t%d" % ((k,) + mine[k]))
        return 0
    other = {}
    for line in open(a.against):
        f = line.rstrip("\n").split("\t")
        if len(f) == 5 and a.family in f[0]:
            other[f[0]] = tuple(int(x) for x in f[1:])
    bad = 0
    for k in sorted(other):
        if k not in mine:
            print("GONE     %s %s" % (k, other[k]))
            bad += 1
        elif mine[k] != other[k]:
            print("DIFFERS  %s  vgpr/sgpr/scratch/instructions %s -> %s" % (k, other[k], mine[k]))
            bad += 1
    new = sorted(k for k in mine if k not in other)
    for k in new:
        print("NEW      %s  vgpr/sgpr/scratch/instructions %s" % (k, mine[k]))
    print("%d symbols of the other build compared: %d differ or are gone; %d new" % (len(other), bad, len(new)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
