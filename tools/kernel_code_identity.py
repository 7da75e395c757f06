#!/usr/bin/env python3
"""Compares the gfx950 machine code of two builds of resampler_amd/csrc, function by function (needs no GPU).

    python tools/kernel_code_identity.py PARENT_CSRC NEW_CSRC > profiles/<change>/kernel_code_identity.txt

Both directories hold the objects `make` left (<file>.o for every <file>.hip).  The device code object of each is taken out of the
object's .hip_fatbin section (llvm-objcopy, clang-offload-bundler), and every function symbol's bytes in it are compared with the
same symbol's of the other build: identical, differ, or present in one build only.  A code object is linked: a function that takes
the address of something outside itself (a constant table in .rodata) holds the distance from its own address as a 32-bit literal,
and that literal moves when functions in front of it change size.  Such a function counts as identical -- and is counted again
under "moved" -- when it has the parent's size and at most four 32-bit words differ, all by one and the same distance, a multiple
of 64 bytes (kernel descriptors are 64 bytes, functions 256-byte aligned: what the function and its target moved apart by); any
other difference is "differ".  Prints one line per .hip file and, below, what
differs by file and kernel family (the symbol's demangled name up to its template arguments)."""
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    fat, co = os.path.join(tmp, "x.fatbin"), os.path.join(tmp, "x.co")
    run(f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj)
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}")
    return co


def functions(co):
    """{symbol: (address, bytes)} of a code object's functions."""
    sections = {}
    for line in run(f"{LLVM}/llvm-readelf", "-SW", co).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S*)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            sections[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))      # address, file offset
    data = open(co, "rb").read()
    out = {}
    for line in run(f"{LLVM}/llvm-readelf", "-sW", "--symbols", co).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[6].isdigit():
            value, size, ndx = int(f[1], 16), int(f[2]), int(f[6])
            addr, off = sections[ndx]
            out[f[7]] = (value, data[off + value - addr:off + value - addr + size])
    return out


def same_code(new, parent):
    """-> 0 differ, 1 identical byte for byte, 2 identical but for address literals that moved with the function."""
    (_, b_new), (_, b_parent) = new, parent
    if b_new == b_parent:
        return 1
    if len(b_new) != len(b_parent) or len(b_new) % 4:
        return 0
    deltas = set()
    for i in range(0, len(b_new), 4):
        w_new, w_parent = int.from_bytes(b_new[i:i + 4], "little"), int.from_bytes(b_parent[i:i + 4], "little")
        if w_new != w_parent:
            deltas.add(((w_new - w_parent) & 0xFFFFFFFF, i))
    if len(deltas) > 4 or len({d for d, _ in deltas}) != 1 or next(iter(deltas))[0] % 64:
        return 0
    return 2


def family(symbol):
    name = run("c++filt", symbol).strip()
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(anonymous namespace\)::|rsmp::", "", name)
    return re.split(r"[<(]", name)[0]


def main(parent_dir, new_dir):
    files = sorted(f[:-4] for f in os.listdir(new_dir) if f.endswith(".hip"))
    detail = []
    with tempfile.TemporaryDirectory() as tmp:
        for f in files:
            sides = []
            for d in (new_dir, parent_dir):
                obj = os.path.join(d, f + ".o")
                sides.append(functions(code_object(obj, tmp)) if os.path.exists(obj) else {})
            new, parent = sides
            kind = {s: same_code(new[s], parent[s]) for s in new if s in parent}
            same = [s for s in kind if kind[s]]
            moved = [s for s in kind if kind[s] == 2]
            differ = [s for s in kind if not kind[s]]
            only_new = [s for s in new if s not in parent]
            only_parent = [s for s in parent if s not in new]
            print(f"{f} new {len(new)} parent {len(parent)} identical {len(same)} differ {len(differ)} only new {len(only_new)} only parent {len(only_parent)}"
                  + (f" (moved: {len(moved)} of the identical)" if moved else ""))
            for what, syms in (("moved", moved), ("differ", differ), ("only new", only_new), ("only parent", only_parent)):
                for fam, n in sorted(collections.Counter(family(s) for s in syms).items()):
                    detail.append(f"  {f:<20} {what:<12} {fam:<32} {n}")
    print("\nwhat differs or moved, by file and kernel family (count of symbols):")
    print("\n".join(detail) if detail else "  nothing")


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2])
