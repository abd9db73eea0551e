#!/usr/bin/env python3
"""Are the kernels of two builds of libvr_hip.so the same machine code?

A change that is meant to touch host code only (the C ABI, the context, the launch path, which translation unit compiles what) must
leave every gfx950 function as it was: then no kernel can be slower or compute anything else.  This script disassembles the code
objects of both libraries (tools/check_exec_regions.py: code_objects, disassemble), keys every function on its mangled symbol and
compares the instruction text, addresses, encodings and the padding behind a function's last instruction stripped.  A library is the
UNION of the functions of its code objects: how many translation units a build has, and which of them holds a kernel, is not a
difference.  It prints the symbols that differ or exist on one side only, and the symbols that one library holds in several code
objects with different bodies.

    python tools/device_code_diff.py before/libvr_hip.so after/libvr_hip.so      exit status 0 = no difference
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_exec_regions import code_objects, disassemble  # noqa: E402


def functions(listing):
    """{mangled symbol: [instruction text, ...]} of one disassembly listing (llvm-objdump -d)."""
    out, cur = {}, None
    for line in listing.split("\n"):
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        ins = " ".join(line.split("//")[0].split())  # (the comment holds the address and the encoding)
        if cur is not None and ins:
            cur.append(ins)
    # what follows a function's last instruction up to the next symbol is the assembler's padding (s_nop 0, or zeros shown as "..."):
    # it depends on what is linked behind the function, not on the function
    for ins in out.values():
        while ins and ins[-1] in ("s_nop 0", "..."):
            ins.pop()
    return out


def union(listings):
    """({mangled symbol: instructions} over the listings of one library's code objects, the symbols that occur in several of them
    with different bodies, sorted).  The union keeps such a symbol's first body."""
    out, clash = {}, set()
    for listing in listings:
        for k, ins in functions(listing).items():
            if out.setdefault(k, ins) != ins:
                clash.add(k)
    return out, sorted(clash)


def compare(a, b):
    """(symbols whose instructions differ, symbols only in a, symbols only in b), each sorted.  a, b: one listing, or the list of
    the listings of a library's code objects."""
    a, b = (union([x] if isinstance(x, str) else x)[0] for x in (a, b))
    differ = sorted(k for k in a.keys() & b.keys() if a[k] != b[k])
    return differ, sorted(a.keys() - b.keys()), sorted(b.keys() - a.keys())


def main():
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    libs = [[disassemble(o) for o in code_objects(path)] for path in sys.argv[1:]]
    if not libs[0] or not libs[1]:
        print(f"gfx950 code objects: {len(libs[0])} in {sys.argv[1]}, {len(libs[1])} in {sys.argv[2]}")
        return 2
    (fa, clash_a), (fb, clash_b) = union(libs[0]), union(libs[1])
    differ, only_a, only_b = compare(libs[0], libs[1])
    print(f"{len(fa)} symbols in {len(libs[0])} code objects, {len(fb)} in {len(libs[1])}: {len(differ)} differ, {len(only_a)} missing, "
          f"{len(only_b)} new, {len(clash_a)} + {len(clash_b)} with several bodies in one library")
    for tag, names in (("differs", differ), ("missing", only_a), ("new", only_b), ("several bodies in the first library", clash_a),
                       ("several bodies in the second library", clash_b)):
        for k in names:
            print(f"   {tag}: {k}")
    return 1 if differ or only_a or only_b or clash_a or clash_b else 0


if __name__ == "__main__":
    sys.exit(main())
