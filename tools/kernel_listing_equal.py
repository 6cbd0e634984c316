"""Kernel by kernel, is the device code of two versions of one HIP source the same?  Cross-compiles both with the Makefile's flags plus
--cuda-device-only -S -Rpass-analysis=kernel-resource-usage (no GPU needed) and prints one line per kernel of either version: the
name, then for the parent and the new version the instruction count, VGPRs, SGPRs, SGPR spills, scratch bytes per lane and the
compiler's occupancy, then "identical" (the same instruction listing, local labels renumbered), "differs", "deleted" or "added".
Resource figures and counts only: the listing is compared as text, never searched.

    python tools/kernel_listing_equal.py PARENT.hip NEW.hip [-I include_dir ...] > profiles/NAME.txt
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "feynmandiagram.jl_amd", "csrc")
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-result -Wno-unused-value".split()
FIELDS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("SGPRs Spill", "sgpr_spill"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occupancy"))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    short = [re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", d)) for d in out.splitlines()]
    return dict(zip(names, (re.sub(r"\(.*$", "", s) for s in short)))


def compile_listing(src, includes):
    """{mangled kernel name: {"text": normalised listing, "n": instructions, resource figures ...}}"""
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "out.s")
        cmd = ["/opt/rocm/bin/hipcc", *FLAGS, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-x", "hip", src, "-o", asm]
        for inc in includes:
            cmd += ["-I", inc]
        remarks = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        lines = open(asm).read().splitlines()
    kernels, name = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m and name:
                kernels[name][key] = int(m.group(1))
    body, cur = {}, None
    for line in lines:
        m = re.match(r"^(\w+):", line)
        if m and m.group(1) in kernels:
            cur = m.group(1)
            body[cur] = []
            continue
        if cur and re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
        elif cur:
            code = line.split(";")[0].rstrip()
            if code.strip():
                body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", code))
    for k, text in body.items():
        kernels[k]["text"] = "\n".join(text)
        kernels[k]["n"] = sum(1 for t in text if t.startswith("\t") and not t.lstrip().startswith("."))
    return kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("-I", dest="includes", action="append", default=[CSRC])
    a = ap.parse_args()
    old, new = compile_listing(a.parent, a.includes), compile_listing(a.new, a.includes)
    names = demangle(sorted(set(old) | set(new)))
    cols = ("n", "vgpr", "sgpr", "sgpr_spill", "scratch", "occupancy")
    print("kernel | parent: instructions vgpr sgpr sgpr_spill scratch occupancy | new: the same | listing")
    count = {"identical": 0, "differs": 0, "deleted": 0, "added": 0}
    for k in sorted(names, key=lambda k: names[k]):
        fig = lambda d: " ".join(str(d[k][c]) for c in cols) if k in d else "-"
        verdict = "deleted" if k not in new else "added" if k not in old else "identical" if old[k]["text"] == new[k]["text"] else "differs"
        count[verdict] += 1
        print(f"{names[k]} | {fig(old)} | {fig(new)} | {verdict}")
    print(f"parent: {len(old)} kernels; new: {len(new)} kernels; " + ", ".join(f"{v} {k}" for k, v in count.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
