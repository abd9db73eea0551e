#!/usr/bin/env python3
"""Are the kernels of two builds of libvr_hip.so the same machine code?

A change that is meant to touch host code only (the C ABI, the context, the launch path) must leave every gfx950 code object as
it was: then no kernel can be slower or compute anything else.  This script disassembles the code objects of both libraries
(tools/check_exec_regions.py: code_objects, disassemble), keys every function on its mangled symbol and compares the
instruction text, addresses, encodings and the padding behind a function's last instruction stripped.  It prints the symbols that differ or exist on one side only.

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


def compare(listing_a, listing_b):
    """(symbols whose instructions differ, symbols only in a, symbols only in b), each sorted."""
    a, b = functions(listing_a), functions(listing_b)
    differ = sorted(k for k in a.keys() & b.keys() if a[k] != b[k])
    return differ, sorted(a.keys() - b.keys()), sorted(b.keys() - a.keys())


def main():
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    objs_a, objs_b = code_objects(sys.argv[1]), code_objects(sys.argv[2])
    if not objs_a or len(objs_a) != len(objs_b):
        print(f"gfx950 code objects: {len(objs_a)} in {sys.argv[1]}, {len(objs_b)} in {sys.argv[2]}")
        return 2
    bad = 0
    for i, (oa, ob) in enumerate(zip(objs_a, objs_b)):
        la, lb = disassemble(oa), disassemble(ob)
        differ, only_a, only_b = compare(la, lb)
        print(f"code object {i}: {len(functions(la))} symbols, {len(differ)} differ, {len(only_a)} missing, {len(only_b)} new")
        for tag, names in (("differs", differ), ("missing", only_a), ("new", only_b)):
            for k in names:
                print(f"   {tag}: {k}")
        bad += len(differ) + len(only_a) + len(only_b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
