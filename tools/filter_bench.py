#!/usr/bin/env python3
"""Speed of the separable filters (vr_volume_filter, csrc/vr_filter.h) on a BASELINE configuration.

    python tools/filter_bench.py --workload C3 [--steps 10] [--warmup 2] [--no-host] [--out profiles/filter_bench_C3.json]

The scene is workloads.build_scene's (its volume and preparation).  Channel 3 of volume slot 0 (the CT) is smoothed by a Gaussian into
channel 3 of volume slot 1, over the whole volume: sigma = 1 voxel, sigma = 2 voxels, and sigma = 2 mm on a grid of 1 x 1 x 3 mm (2, 2
and 2 / 3 voxels), truncate 4.  For every case and both kernel forms (flavour 0: LDS tiles; flavour 1: one lane per output, every input
from memory) one JSON line: the medians over K calls behind W warm-up calls of the call's wall clock (it is synchronous) and of its four
phases on the device (vr_filter_timing: the first pass, the remaining passes, the write with the result words, the trailing rebuild of
what is derived from the slot), the result, the counters, whether the channel equals the first form's, and for the first pass and for the
remaining ones the bytes they must move -- the field in (16 B a voxel from the float4 source, whose every line is touched, 4 B from a
field) times the halo share of the default form's tile ((256 + 2 r) / 256 along x, (64 + 2 r) / 64 along y and z), and the field out --
with the rate that makes and its share of the MI355X's 8 TB/s.  Then, unless --no-host, the route the call replaces on this machine:
vr_volume_download of the slot, scipy.ndimage.gaussian_filter (mode="nearest", float32) of the channel and vr_volume_upload into the
second slot.  The lines are also written, as a JSON list, to --out.  Nothing outside the repository is read."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from volumerendering_amd import capi, host, workloads as wl  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12  # the MI355X's HBM3E
CASES = [("sigma 1 voxel", (1.0, 1.0, 1.0)), ("sigma 2 voxels", (2.0, 2.0, 2.0)), ("sigma 2 mm at 1 x 1 x 3 mm", (2.0, 2.0, 2.0 / 3.0))]


def pass_bytes(n, radii):
    """Per pass (x, y, z over the whole n^3 volume) the bytes it must move: field in times the halo share, field out."""
    vox = float(n) ** 3
    out = []
    for k, r in enumerate(radii):
        tile = 256 if k == 0 else 64
        out.append(vox * (16 if k == 0 else 4) * (tile + 2 * r) / tile + vox * 4)
    return out


def main():
    ap = argparse.ArgumentParser(description="Speed of the separable filters (vr_volume_filter) on a baseline workload: Gaussians of the CT's "
                                             "channel 3 into a second slot, both kernel forms, phase by phase, against download + scipy + upload.")
    ap.add_argument("--workload", default="C3", choices=sorted(wl.WORKLOADS))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--vol-n", type=int, default=0, help="volume side instead of the workload's (rehearsals)")
    ap.add_argument("--no-host", action="store_true", help="skip the download + scipy + upload route")
    ap.add_argument("--out", default=None, help="where the lines are written as a JSON list (default profiles/filter_bench_<workload>.json)")
    args = ap.parse_args()
    n, W, H, vname = wl.WORKLOADS[args.workload]
    n = args.vol_n or n
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    app = host.Application(W, H, 0)
    wl.build_scene(app, args.workload, vol_n=args.vol_n, quiet=True)
    ctx = app.context()
    shape = (n, n, n)
    ctx.volume_upload(1, np.zeros(shape + (4,), np.float32))
    emit(workload=args.workload, volume=n, slot_bytes=16 * n ** 3, steps=args.steps, warmup=args.warmup, peak_bytes_per_s=PEAK_BYTES_PER_S)
    d = ctx.filter_whole(0, 3, 1, 3)
    for name, sigmas in CASES:
        taps = [capi.filter_gaussian(s) for s in sigmas]
        radii = [t.size // 2 for t in taps]
        must = pass_bytes(n, radii)
        first = None
        for flavour, form in ((0, "lds tiles"), (1, "plain")):
            ctx.set_kernel_flavour(flavour)
            for _ in range(args.warmup):
                res = ctx.volume_filter(d, taps)
            wall, phases = [], []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                res = ctx.volume_filter(d, taps)
                wall.append((time.perf_counter() - t0) * 1e3)
                phases.append(ctx.filter_timing())
            box, computed, passes = ctx.filter_counters()
            channel = ctx.volume_download(1, shape)[..., 3].copy()
            if first is None:
                first = channel
            med = [round(statistics.median(ph[i] for ph in phases), 4) for i in range(4)]
            rate = [must[0] / (med[0] * 1e-3), sum(must[1:]) / (med[1] * 1e-3)]
            emit(workload=args.workload, case=name, sigma_voxels=[round(s, 4) for s in sigmas], radii=radii, form=form,
                 wall_ms=round(statistics.median(wall), 3), wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3),
                 first_pass_ms=med[0], other_passes_ms=med[1], write_ms=med[2], refresh_ms=med[3], device_ms=round(sum(med), 4),
                 first_pass_bytes=int(must[0]), other_passes_bytes=int(sum(must[1:])),
                 first_pass_tb_per_s=round(rate[0] / 1e12, 3), other_passes_tb_per_s=round(rate[1] / 1e12, 3),
                 first_pass_of_peak=round(rate[0] / PEAK_BYTES_PER_S, 3), other_passes_of_peak=round(rate[1] / PEAK_BYTES_PER_S, 3),
                 stored=int(res.stored), nonfinite=int(res.nonfinite), lo_value=float(res.lo_value), hi_value=float(res.hi_value),
                 box=box, computed=computed, passes=passes,
                 equals_first_form=bool(np.array_equal(channel.view(np.uint32), first.view(np.uint32))))
            del channel
        del first
    ctx.set_kernel_flavour(0)
    if not args.no_host:
        import scipy.ndimage as ndi
        for name, sigmas in (CASES[0], CASES[2]):
            t0 = time.perf_counter()
            v = ctx.volume_download(0, shape)
            t1 = time.perf_counter()
            smooth = ndi.gaussian_filter(np.ascontiguousarray(v[..., 3]), sigma=sigmas[::-1], mode="nearest", truncate=4.0, output=np.float32)
            v[..., 3] = smooth
            t2 = time.perf_counter()
            ctx.volume_upload(1, v)
            t3 = time.perf_counter()
            got = ctx.volume_download(1, shape)[..., 3]
            ctx.volume_filter(d, [capi.filter_gaussian(s) for s in sigmas])
            dev = ctx.volume_download(1, shape)[..., 3]
            emit(workload=args.workload, case=name, route="vr_volume_download + scipy.ndimage.gaussian_filter (float32, nearest) + vr_volume_upload on this host",
                 download_ms=round((t1 - t0) * 1e3, 1), scipy_ms=round((t2 - t1) * 1e3, 1), upload_ms=round((t3 - t2) * 1e3, 1),
                 total_ms=round((t3 - t0) * 1e3, 1), max_abs_difference_from_the_device=float(np.abs(got - dev).max()))
            del v, smooth, got, dev
    app.close()
    out = args.out or os.path.join(ROOT, "profiles", f"filter_bench_{args.workload}.json")
    with open(out, "w") as fh:
        json.dump(lines, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
