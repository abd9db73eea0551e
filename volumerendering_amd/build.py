"""Builds the in-tree native libraries: libvr_hip.so (HIP kernels + C ABI, gfx950) and libvr_host.so
(C++ host surface mirroring the reference's Volume / TransferFunction / Camera / MiniApp classes)."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (xnack-: the MI355X runs with XNACK off; code for "either" makes the compiler break every run of vector-memory instructions in
# which a destination overlaps an earlier address register with an s_nop -- seven per request of march_p2_kernel.
# VR_HIP_ARCH=gfx950 in the environment builds the generic form.)
HIP_ARCH = os.environ.get("VR_HIP_ARCH", "gfx950:xnack-")
HIP_FLAGS = ["-O3", "--offload-arch=" + HIP_ARCH, "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
             "-std=c++17", "-Wall", "-Wno-unused-function"]
HOST_FLAGS = ["-O2", "-std=c++20", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall"]


def _newer(target: str, sources: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _sources(d: str, exts: tuple[str, ...]) -> list[str]:
    out = []
    for dp, _, fs in os.walk(d):
        out += [os.path.join(dp, f) for f in fs if f.endswith(exts)]
    return sorted(out)


# libvr_hip.so's translation units: the C ABI with the auxiliary and voxel-tool kernels, and the march kernels once per arithmetic mode
HIP_UNITS = ("vr_api", "vr_march", "vr_fused")


def include_closure(src: str, flags: list[str]) -> list[str]:
    """src and every file it reaches through #include outside the system directories, as the compiler resolves them under
    `flags` (the host pass's preprocessor alone: no code is generated, and none can be forgotten)."""
    out = subprocess.run([HIPCC, *flags, "--cuda-host-only", "-E", "-MM", src], check=True, stdout=subprocess.PIPE, text=True).stdout
    rule = out.replace("\\\n", " ").split(": ", 1)[1]  # (a make rule `object: files`, a space in a name escaped)
    return [os.path.normpath(p.replace("\\ ", " ")) for p in re.split(r"(?<!\\)\s+", rule.strip())]


def stale_units(objs: dict[str, str], closures: dict[str, list[str]], stamp: str, want: str) -> list[str]:
    """The units to compile: all of them where the flags stamp is not `want`, else each whose object is missing or older than a
    file of its own closure."""
    if not os.path.exists(stamp) or open(stamp).read() != want:
        return list(objs)
    return [u for u in objs if _newer(objs[u], closures[u])]


def build_hip(force: bool = False) -> str:
    """Three translation units, compiled side by side: vr_api.hip (the C ABI and every kernel that exists once), vr_march.hip
    (the march kernels with separately rounded multiply-adds) and vr_fused.hip (the march kernels once more with fused
    multiply-adds), linked into one libvr_hip.so.  An edit recompiles the units whose include closure holds the edited file."""
    target = os.path.join(HERE, "libvr_hip.so")
    flags = [f for f in HIP_FLAGS if f != "-shared"] + os.environ.get("VR_EXTRA_HIPCC_FLAGS", "").split()
    # the flags the objects were compiled with: a change (VR_EXTRA_HIPCC_FLAGS) rebuilds them
    stamp = os.path.join(CSRC, ".build_flags")
    want = " ".join(flags)
    srcs = {u: os.path.join(CSRC, u + ".hip") for u in HIP_UNITS}
    objd = {u: os.path.join(CSRC, u + ".o") for u in HIP_UNITS}
    objs = list(objd.values())
    stale = list(HIP_UNITS) if force else stale_units(objd, {u: include_closure(srcs[u], flags) for u in HIP_UNITS}, stamp, want)
    procs = [(u, subprocess.Popen([HIPCC, *flags, "-c", "-o", objd[u], srcs[u]])) for u in stale]
    for name, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, f"hipcc {name}.hip")
    if procs or force or _newer(target, objs):
        subprocess.run([HIPCC, "--offload-arch=" + HIP_ARCH, "-fPIC", "-shared", "-o", target, *objs], check=True)
    with open(stamp, "w") as fh:
        fh.write(want)
    return target


def build_host(force: bool = False) -> str | None:
    hostdir = os.path.join(CSRC, "host")
    cpps = _sources(hostdir, (".cpp",))
    if not cpps:
        return None
    target = os.path.join(HERE, "libvr_host.so")
    deps = _sources(hostdir, (".cpp", ".h")) + [os.path.join(os.path.dirname(HERE), "include", "vr.h")]
    if force or _newer(target, deps):
        subprocess.run(["g++", *HOST_FLAGS, "-I", os.path.join(os.path.dirname(HERE), "include"), "-o", target, *cpps,
                        "-L", HERE, "-lvr_hip", "-Wl,-rpath,$ORIGIN"], check=True)
    return target


def build_mgpu(force: bool = False) -> str:
    """libvr_mgpu.so: the multi-GPU frame loop (C++ host code on the HIP runtime + RCCL, above the C ABI of libvr_hip.so)."""
    target = os.path.join(HERE, "libvr_mgpu.so")
    src = os.path.join(CSRC, "mgpu", "vr_mgpu.cpp")
    inc = os.path.join(os.path.dirname(HERE), "include")
    deps = [src, os.path.join(inc, "vr_mgpu.h"), os.path.join(inc, "vr.h")]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if force or _newer(target, deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", inc,
                        "-I", os.path.join(rocm, "include"), "-o", target, src, "-L", HERE, "-lvr_hip",
                        "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-lrccl",
                        "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    return target


def build_all(force: bool = False):
    build_hip(force)
    build_host(force)
    build_mgpu(force)
