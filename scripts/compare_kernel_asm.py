#!/usr/bin/env python3
"""Compares the device code of two builds kernel by kernel: the check that a host-side or header-only refactor left the
machine code alone (EXPERIMENTS.md, "InfoNCE / BCE: one engine header ..." ran it by hand).

    python scripts/compare_kernel_asm.py PARENT_TEMPS BRANCH_TEMPS

Both directories come from `recommendation_amd._build.build(force=True, keep_temps=DIR)`, which keeps every unit's device
assembly as <unit>-hip-amdgcn-amd-amdhsa-gfx950.s.  A kernel is keyed by its mangled name; two things are compared as text:

  * its instructions and block labels, with comments, assembler directives and the function's number inside block labels
    (.LBB<function>_<block>: the number moves when a unit gains or loses a kernel) stripped;
  * its whole .amdhsa_kernel descriptor (registers, LDS, scratch, kernarg size, ...).

Prints identical / differing / added / missing per unit and exits non-zero on any of the last three.  Nothing is searched
for: the tool knows no instruction by name."""
import glob
import os
import re
import sys

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
BLOCK_LABEL = re.compile(r"\.LBB\d+_(\d+)")


def kernels(path):
    """mangled name -> (instruction text, descriptor text) of every kernel of one assembly file"""
    with open(path) as f:
        lines = f.read().split("\n")
    descriptors, name, block = {}, None, []
    for line in lines:
        s = line.strip()
        if s.startswith(".amdhsa_kernel "):
            name, block = s.split()[1], []
        elif s == ".end_amdhsa_kernel":
            descriptors[name], name = "\n".join(block), None
        elif name is not None:
            block.append(" ".join(s.split(";")[0].split()))
    out, name, body, in_descriptor = {}, None, [], False
    for line in lines:
        if name is None:
            label = line.split(":")[0]
            if line[:1] not in ("", "\t", " ", ".", ";") and label in descriptors and line.startswith(label + ":"):
                name, body = label, []
            continue
        s = line.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            out[name], name = ("\n".join(body), descriptors[name]), None
        elif s.startswith(".amdhsa_kernel "):
            in_descriptor = True
        elif s == ".end_amdhsa_kernel":
            in_descriptor = False
        elif s and not in_descriptor and (not s.startswith(".") or s.startswith(".LBB")):
            body.append(BLOCK_LABEL.sub(r".LBB_\1", " ".join(s.split())))
    missing_body = set(descriptors) - set(out)
    if missing_body:
        raise SystemExit(f"{path}: no body found for {sorted(missing_body)}")
    return out


def units(directory):
    found = {os.path.basename(p)[:-len(SUFFIX)]: p for p in glob.glob(os.path.join(directory, "*" + SUFFIX))}
    if not found:
        raise SystemExit(f"{directory}: no *{SUFFIX} (build with keep_temps=)")
    return found


def main(argv):
    if len(argv) != 3:
        raise SystemExit(__doc__)
    parent, branch = units(argv[1]), units(argv[2])
    bad = 0
    for unit in sorted(set(parent) | set(branch)):
        if unit not in parent or unit not in branch:
            print(f"{unit}: unit {'added' if unit in branch else 'missing'}")
            bad += 1
            continue
        a, b = kernels(parent[unit]), kernels(branch[unit])
        added, missing = sorted(set(b) - set(a)), sorted(set(a) - set(b))
        text = [k for k in sorted(set(a) & set(b)) if a[k][0] != b[k][0]]
        desc = [k for k in sorted(set(a) & set(b)) if a[k][0] == b[k][0] and a[k][1] != b[k][1]]
        same = len(set(a) & set(b)) - len(text) - len(desc)
        print(f"{unit}: {same} identical, {len(text) + len(desc)} differing, {len(added)} added, {len(missing)} missing")
        for tag, names in (("instructions differ", text), ("descriptor differs", desc), ("added", added), ("missing", missing)):
            for k in names:
                print(f"    {tag}: {k}")
        bad += len(text) + len(desc) + len(added) + len(missing)
    print("all kernels identical" if not bad else f"{bad} deviation(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
