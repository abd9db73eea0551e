"""Which gfx950 code object of libvr_hip.so carries which kernel (harness only).

The library has three: the two march units -- the march kernels in namespace vr (separately rounded multiply-adds, vr_march.hip)
and once more in namespace vrf (fused, vr_fused.hip) -- and the C ABI's unit with every kernel that exists once (vr_api.hip).  The
tests of a march family ask march_units() for the family's kernels per march unit; it asserts that exactly two code objects carry
any of them, one under _ZN2vr... alone and one under _ZN3vrf... alone, and hands back what each carries and touches of scratch."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_exec_regions as cer  # noqa: E402

sys.path.pop(0)
LIB = os.path.join(ROOT, "volumerendering_amd", "libvr_hip.so")


def carriers(*wanted):
    """[(names, scratch, listing)] of the code objects that hold a function whose name contains one of `wanted`: those functions'
    names, their instructions that touch scratch as (name, line), and the code object's whole listing."""
    out = []
    for o in cer.code_objects(LIB):
        text = cer.disassemble(o)
        kernel, names, scratch = None, set(), []
        for line in text.split("\n"):
            m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
            if m:
                kernel = m.group(1) if any(w in m.group(1) for w in wanted) else None
                if kernel:
                    names.add(kernel)
                continue
            if kernel and "scratch_" in line:
                scratch.append((kernel, line.strip()))
        if names:
            out.append((names, scratch, text))
    return out


def march_units(*wanted):
    """carriers(*wanted) as [the vr unit's, the vrf unit's]: exactly two code objects carry any of the kernels, one of them in
    namespace vr alone and the other in namespace vrf alone."""
    got = carriers(*wanted)
    assert len(got) == 2, [sorted(names) for names, _, _ in got]
    got.sort(key=lambda c: min(c[0]))  # (_ZN2vr... sorts before _ZN3vrf...)
    assert all(n.startswith("_ZN2vr") for n in got[0][0]), sorted(got[0][0])
    assert all(n.startswith("_ZN3vrf") for n in got[1][0]), sorted(got[1][0])
    return got


def once_in_the_abi_unit(kernel):
    """The kernel exists once: one code object holds it, under one name in namespace vr, and that one is neither march unit (it
    holds no march_kernel).  Returns (names, scratch, listing) of it."""
    got = carriers(kernel)
    assert len(got) == 1 and len(got[0][0]) == 1, [sorted(names) for names, _, _ in got]
    assert min(got[0][0]).startswith("_ZN2vr"), got[0][0]
    assert "march_kernel" not in got[0][2]
    return got[0]
