#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds, kernel by kernel, from their device assembly.

    hipcc <FLAGS of clair_torch_amd/build.py> --cuda-device-only -S -o before/ct_merge.s clair_torch_amd/csrc/ct_merge.hip
    ... (every translation unit of interest, for both trees)
    python tools/compare_kernel_asm.py before/ after/

Every *.s file of a directory is split into one record per kernel, keyed by the mangled name: the text from the
kernel's label to its .end_amdhsa_kernel (instructions and the kernel descriptor: registers, LDS, scratch, kernarg
size) plus its entry in the amdhsa.kernels metadata (argument offsets, occupancy).  The two directories must hold the
same set of kernels, and every record must be byte-identical.  Which file a kernel is in and the order of the kernels
inside a file do not matter; for that reason the per-file function ordinal inside local labels and the comments that name
them (.LBB<n>_, BB<n>_, .LJTI<n>_, .Lfunc_end<n>) is dropped before the comparison, together with the padding between
such a label and its trailing comment (it depends on the ordinal's width) -- nothing else is normalised.

Prints the first differing kernel as a unified diff and exits 1; exits 0 when all are identical.  No GPU needed.
"""
import difflib
import glob
import os
import re
import sys

LABEL = re.compile(r"^(_Z\w+):")
ORDINAL = re.compile(r"(BB|JTI|\.Lfunc_begin|\.Lfunc_end|\.Ltmp)\d+(?=_\d|\b)")
LABEL_PAD = re.compile(r"^(\.L\w+:) +;", re.M)
META_NAME = re.compile(r"^    \.name:\s+(\S+)")


def kernel_records(directory):
    """{mangled name: text} over every .s file of `directory`."""
    code, meta = {}, {}
    files = sorted(glob.glob(os.path.join(directory, "*.s")))
    if not files:
        sys.exit(f"{directory}: no .s files")
    for path in files:
        with open(path) as f:
            lines = f.read().split("\n")
        name, start = None, 0
        for i, line in enumerate(lines):
            if line == "amdhsa.kernels:":
                break
            m = LABEL.match(line)
            if m:
                name, start = m.group(1), i  # (a label not followed by a descriptor was a device function)
            elif name is not None and line.strip() == ".end_amdhsa_kernel":
                if name in code:
                    sys.exit(f"{path}: kernel {name} defined twice in {directory}")
                code[name] = LABEL_PAD.sub(r"\1 ;", ORDINAL.sub(r"\1", "\n".join(lines[start:i + 1])))
                name = None
        else:
            continue  # no kernels in this file
        # the amdhsa.kernels list: entries start with "  - " and the list ends at the first line that is not indented
        entry = []
        for line in lines[i + 1:] + [""]:
            if entry and (line.startswith("  - ") or not line.startswith("  ")):
                names = [m.group(1) for m in map(META_NAME.match, entry) if m]
                meta[names[0]] = "\n".join(entry)
                entry = []
            if not line.startswith("  "):
                break
            entry.append(line)
    missing = sorted(set(code) ^ set(meta))
    if missing:
        sys.exit(f"{directory}: kernels without metadata or metadata without kernel: {missing[:3]}")
    return {k: code[k] + "\n" + meta[k] for k in code}


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    before, after = kernel_records(argv[1]), kernel_records(argv[2])
    print(f"kernels: {len(before)} in {argv[1]}, {len(after)} in {argv[2]}")
    lost, added = sorted(set(before) - set(after)), sorted(set(after) - set(before))
    for k in lost[:10]:
        print(f"only in {argv[1]}: {k}")
    for k in added[:10]:
        print(f"only in {argv[2]}: {k}")
    differing = [k for k in sorted(set(before) & set(after)) if before[k] != after[k]]
    print(f"names compared: {len(set(before) & set(after))}, identical: {len(set(before) & set(after)) - len(differing)}, "
          f"differing: {len(differing)}, lost: {len(lost)}, added: {len(added)}")
    if differing:
        k = differing[0]
        print(f"first differing kernel: {k}")
        diff = difflib.unified_diff(before[k].split("\n"), after[k].split("\n"), argv[1], argv[2], lineterm="", n=2)
        print("\n".join(list(diff)[:200]))
    return 1 if (lost or added or differing) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
