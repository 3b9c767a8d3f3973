#!/usr/bin/env python3
"""Compare the device assembly of two builds of one .hip file, kernel by kernel.

    hipcc <the Makefile's flags> --save-temps -c csrc/attn_enc.hip        (once per build, in two directories)
    tools/kernel_asm_diff.py OLD/attn_enc-hip-amdgcn-amd-amdhsa-gfx950.s NEW/attn_enc-hip-amdgcn-amd-amdhsa-gfx950.s

The compiler emits kernels in instantiation order and numbers its local labels by position in the file, so a refactor of the host code
that names the same instantiations in another order moves every kernel without changing one.  This splits both files at the kernels'
symbols, renumbers the per-function labels and compares each kernel's text - instructions, the .amdhsa_ descriptor (registers, LDS,
scratch) and its metadata entry.  Exit status 0: same set of kernels, every one identical.
"""
import re
import sys


def kernels(path):
    text = open(path).read()
    body, _, meta = text.partition("\t.amdgpu_metadata")
    out = {}
    # one block per function: from its first .section line to the next function's
    starts = [m.start() for m in re.finditer(r"^\t\.section\t\.text\.(\S+?),.*\n\t\.protected\t", body, re.M)]
    for a, b in zip(starts, starts[1:] + [len(body)]):
        blk = body[a:b]
        sym = re.match(r"\t\.section\t\.text\.(\S+?),", blk).group(1)
        blk = re.sub(r"\s*;.*$", "", blk, flags=re.M)                                # comments (they quote label numbers and pad to a column)
        blk = re.sub(r"(\.LBB|\.Lfunc_end|\.Lfunc_begin|\.LJTI)\d+", r"\1N", blk)
        lines = [l.rstrip() for l in blk.splitlines()]
        out[sym] = "\n".join(l for l in lines if l and "__hip_cuid" not in l and not re.match(r"\t\.(file|ident)\b", l))      # (per-build id)
    for entry in re.split(r"^  - \.agpr_count:", meta, flags=re.M)[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", entry, re.M).group(1)
        out[name] = out.get(name, "") + "\n--- metadata ---\n" + entry.split("amdhsa.target")[0]
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for sym in sorted(set(old) | set(new)):
        if sym not in new or sym not in old:
            print(("only in OLD: " if sym in old else "only in NEW: ") + sym)
            bad += 1
        elif old[sym] != new[sym]:
            a, b = old[sym].splitlines(), new[sym].splitlines()
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print(f"DIFFERS: {sym} ({len(a)} / {len(b)} lines; first at line {first}: {a[first:first + 1]} / {b[first:first + 1]})")
            bad += 1
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW, {bad} differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
