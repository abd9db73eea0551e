"""CPU tests of the analysis tools that read files (no GPU): tools/launch_gap.py --read on a synthetic kernel trace,
tools/device_code_diff.py's comparison on literal listings."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_gap_reads_a_kernel_trace(tmp_path):
    """Twelve march launches 500 us long and 17 us apart on queue 4, a sort of 60 us on queue 3 behind each, and one launch after a
    host synchronisation (3 ms later: not part of the steady state)."""
    d = tmp_path / "kt" / "host" / "1234_kernel_trace.csv"
    d.parent.mkdir(parents=True)
    rows = ["Kind,Agent_Id,Queue_Id,Kernel_Name,Start_Timestamp,End_Timestamp"]
    t = 1_000_000
    for k in range(12):
        rows.append(f'KERNEL_DISPATCH,1,4,"void vr::march_p2_kernel<1, true, false, false>(vr::MarchBatch, vr::PwQueue)",{t},{t + 500_000}')
        rows.append(f'KERNEL_DISPATCH,1,3,"vr::order_blocks_kernel(unsigned long long const*, int)",{t + 501_000},{t + 561_000}')
        t += 517_000
    t += 3_000_000
    rows.append(f'KERNEL_DISPATCH,1,4,"void vr::march_p2_kernel<1, true, false, false>(vr::MarchBatch, vr::PwQueue)",{t},{t + 500_000}')
    d.write_text("\n".join(rows) + "\n")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "launch_gap.py"), "--read", str(tmp_path / "kt")],
                         capture_output=True, text=True, check=True).stdout
    assert "11 back-to-back march launches" in out
    assert "kernel duration (tracer): median 500.0 us" in out
    assert "end -> next start: median 17.0 us" in out
    assert "vr::order_blocks_kernel: 11 launches, 60.0 us each, queues ['3']" in out
    assert "queues of the march launches: ['4']" in out


def test_device_code_diff_compares_listings():
    """tools/device_code_diff.py on two literal listings: the same instructions at other addresses are equal; a changed
    instruction, a missing and a new symbol are each reported under their mangled names."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import device_code_diff as dcd
    finally:
        sys.path.pop(0)
    a = """
Disassembly of section .text:

0000000000001900 <_ZN2vr12march_kernelILi0EEEvNS_10MarchBatchE>:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000001900: C0060002 00000000
\tv_add_f32_e32 v1, v0, v2                                   // 000000001908: 02020500
\ts_endpgm                                                   // 00000000190C: BF810000

0000000000001a00 <_ZN2vr14present_kernelEPK15HIP_vector_typeIfLj4EEPji>:
\tv_mov_b32_e32 v0, 0                                        // 000000001A00: 7E000280
\ts_endpgm                                                   // 000000001A04: BF810000
"""
    moved = a.replace("0000000000001900", "0000000000002900").replace("// 00000000190", "// 00000000290")
    assert dcd.compare(a, moved) == ([], [], [])
    assert len(dcd.functions(a)["_ZN2vr12march_kernelILi0EEEvNS_10MarchBatchE"]) == 3
    changed = a.replace("v_add_f32_e32 v1, v0, v2", "v_fma_f32 v1, v0, v2, v3")
    assert dcd.compare(a, changed) == (["_ZN2vr12march_kernelILi0EEEvNS_10MarchBatchE"], [], [])
    renamed = a.replace("_ZN2vr14present_kernelE", "_ZN2vr15present2_kernelE")
    differ, missing, new = dcd.compare(a, renamed)
    assert differ == [] and missing == ["_ZN2vr14present_kernelEPK15HIP_vector_typeIfLj4EEPji"]
    assert new == ["_ZN2vr15present2_kernelEPK15HIP_vector_typeIfLj4EEPji"]

    # A library is the union of its code objects: the same two functions in one listing, in two listings either way round, and in
    # three with one that holds neither, are the same library; a change is found wherever the function lives.
    head, march, present = a.split("\n\n0000")
    one = [a]
    two = [head + "\n\n0000" + march + "\n", head + "\n\n0000" + present]
    other_two = [two[1], two[0]]
    three = [head + "\n", two[1], two[0]]
    assert sorted(dcd.union(two)[0]) == sorted(dcd.functions(a)) and dcd.union(two)[0] == dcd.functions(a)
    for x in (one, two, other_two, three):
        assert dcd.union(x)[1] == []
        for y in (one, two, other_two, three):
            assert dcd.compare(x, y) == ([], [], [])
        assert dcd.compare(x, [changed]) == (["_ZN2vr12march_kernelILi0EEEvNS_10MarchBatchE"], [], [])
        assert dcd.compare([renamed], x)[1:] == (["_ZN2vr15present2_kernelEPK15HIP_vector_typeIfLj4EEPji"],
                                                 ["_ZN2vr14present_kernelEPK15HIP_vector_typeIfLj4EEPji"])
    assert dcd.compare(two, [two[0]]) == ([], ["_ZN2vr14present_kernelEPK15HIP_vector_typeIfLj4EEPji"], [])
    # one symbol in two code objects of a library: fine with one body (moved: other addresses), reported with two
    assert dcd.union([a, moved]) == (dcd.functions(a), [])
    assert dcd.union([a, changed])[1] == ["_ZN2vr12march_kernelILi0EEEvNS_10MarchBatchE"]
    assert dcd.union([two[0], two[1], changed])[1] == ["_ZN2vr12march_kernelILi0EEEvNS_10MarchBatchE"]
