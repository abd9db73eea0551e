"""The three translation units of libvr_hip.so stay apart (no GPU, nothing is compiled): what each of vr_api.hip, vr_march.hip and
vr_fused.hip reaches through #include, asked of the compiler the way build.py asks it, and build.py's rule for which objects an
edit makes stale, driven on temporary files."""
import os
import shutil

import pytest

from volumerendering_amd import build

UNITS = ("vr_api", "vr_march", "vr_fused")
# the march code, which the C ABI's unit must not reach ...
MARCH_HEADERS = {"vr_kernels.h", "vr_dp.h", "vr_pw.h", "vr_p2.h", "vr_lt.h", "vr_ray.h", "vr_iso.h", "vr_shadow.h", "vr_bound.h", "vr_launch.h"}
# ... and the tool kernel headers, which the march units must not reach (beside vr_ctx.h and every vr_api_*.h)
TOOL_HEADERS = {"vr_hist.h", "vr_grow.h", "vr_bitrows.h", "vr_morph.h", "vr_dist.h", "vr_raster.h", "vr_scan.h", "vr_outline.h", "vr_comp.h",
                "vr_mesh.h"}


@pytest.fixture(scope="module")
def closures():
    if not (shutil.which("hipcc") or os.path.exists(build.HIPCC)):
        pytest.skip("hipcc not found")
    flags = [f for f in build.HIP_FLAGS if f != "-shared"]
    return {u: build.include_closure(os.path.join(build.CSRC, u + ".hip"), flags) for u in UNITS}


def test_units_are_the_ones_build_compiles():
    assert tuple(build.HIP_UNITS) == UNITS


def test_closures_hold_what_the_units_include(closures):
    """Every closure is made of existing files of this tree, starts from the unit's source and reaches the headers all three share."""
    root = os.path.dirname(os.path.dirname(build.CSRC))
    for u, files in closures.items():
        assert os.path.join(build.CSRC, u + ".hip") in files
        for f in files:
            assert os.path.isfile(f) and f.startswith(root + os.sep), f
        names = {os.path.basename(f) for f in files}
        assert {"vr.h", "vr_device.h", "vr_choice.h", "vr_shared.h"} <= names, (u, sorted(names))


def test_abi_unit_reaches_no_march_header(closures):
    names = {os.path.basename(f) for f in closures["vr_api"]}
    assert not names & MARCH_HEADERS, sorted(names & MARCH_HEADERS)
    assert {"vr_ctx.h", "vr_api_render.h", "vr_prep.h", "vr_skipfield.h", "vr_frame.h"} | TOOL_HEADERS <= names


@pytest.mark.parametrize("unit", ["vr_march", "vr_fused"])
def test_march_units_reach_no_abi_or_tool_header(closures, unit):
    names = {os.path.basename(f) for f in closures[unit]}
    bad = {n for n in names if n == "vr_ctx.h" or n.startswith("vr_api_") or n in TOOL_HEADERS}
    assert not bad, sorted(bad)
    assert MARCH_HEADERS <= names
    assert names == {os.path.basename(f) for f in closures["vr_march"]} - {"vr_march.hip"} | {unit + ".hip"}  # (one text, twice)


def test_an_edit_makes_stale_what_can_reach_it(tmp_path):
    """build.stale_units on files whose times the test sets: objects at t = 100, every header older, then one header newer."""
    def touch(name, t):
        p = tmp_path / name
        p.write_text("")
        os.utime(p, (t, t))
        return str(p)

    hdr = {n: touch(n, 50) for n in ("api_only.h", "march_only.h", "fused_only.h", "both_marches.h", "shared.h")}
    objs = {u: touch(u + ".o", 100) for u in UNITS}
    closures = {"vr_api": [hdr["api_only.h"], hdr["shared.h"]],
                "vr_march": [hdr["march_only.h"], hdr["both_marches.h"], hdr["shared.h"]],
                "vr_fused": [hdr["fused_only.h"], hdr["both_marches.h"], hdr["shared.h"]]}
    stamp = tmp_path / ".build_flags"
    stamp.write_text("-O3 -x")

    def stale(want="-O3 -x"):
        return build.stale_units(objs, closures, str(stamp), want)

    assert stale() == []
    for name, want in (("api_only.h", ["vr_api"]), ("march_only.h", ["vr_march"]), ("fused_only.h", ["vr_fused"]),
                       ("both_marches.h", ["vr_march", "vr_fused"]), ("shared.h", list(UNITS))):
        os.utime(hdr[name], (150, 150))
        assert stale() == want, name
        os.utime(hdr[name], (100, 100))  # as old as the objects: not newer
        assert stale() == [], name
        os.utime(hdr[name], (50, 50))
    # another flag, or no stamp at all: everything
    assert stale("-O3 -x -DVR_DIST_MAX=64") == list(UNITS)
    stamp.unlink()
    assert stale() == list(UNITS)
    stamp.write_text("-O3 -x")
    # a missing object is stale, and it alone
    os.unlink(objs["vr_march"])
    assert stale() == ["vr_march"]
