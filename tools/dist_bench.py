#!/usr/bin/env python3
"""Speed of the distance maps (vr_mask_distance, csrc/vr_dist.h) on a BASELINE configuration.

    python tools/dist_bench.py --workload C3 [--mode signed] [--limit-um 20000] [--spacing-um 1000 1000 3000] [--steps 10] [--warmup 3] [--cpu]

The scene is workloads.build_scene's (its volume and preparation).  As in tools/morph_bench.py a vr_pick of the frame's centre gives a
seed voxel and its value v, and the voxels of volume slot 0 with .a in [v - tolerance, v + tolerance] connected to it become contour 0
of volume slot 1 (vr_segment_grow).  The distance from that contour, on a grid of --spacing-um, with --limit-um (0: none), goes into
component 3 of the same slot in millimetres (scale 0.001, the whole volume).  For both kernel forms (flavour 0: a field is computed only
inside the region outside of which it is known; flavour 1: every voxel of the box) one JSON line: the medians over K calls behind W
warm-up calls of the call's wall clock (it is synchronous) and of its four phases on the device (vr_dist_timing: the pack with the
host's look at the bounding box, the distance passes, the write, the trailing rebuild of what is derived from the slot), the result,
the counters, and whether the channel equals the first form's.  Then the time of a vr_volume_download of the slot, and with --cpu the
time of scipy.ndimage.distance_transform_edt(sampling) on the downloaded mask on this host: the path the call replaces."""
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
from grow_bench import pick_near_centre  # noqa: E402  (tools/ is the script's directory)

MODES = {"outside": capi.DIST_OUTSIDE, "inside": capi.DIST_INSIDE, "signed": capi.DIST_SIGNED}


def main():
    ap = argparse.ArgumentParser(description="Speed of the distance maps (vr_mask_distance) on a baseline workload: the distance from a "
                                             "grown contour, both kernel forms, phase by phase, against a download and scipy on the CPU.")
    ap.add_argument("--workload", default="C3", choices=sorted(wl.WORKLOADS))
    ap.add_argument("--mode", default="signed", choices=sorted(MODES))
    ap.add_argument("--limit-um", type=int, default=0, help="where the map saturates (0: nowhere)")
    ap.add_argument("--spacing-um", type=int, nargs=3, default=[1000, 1000, 3000], metavar=("SX", "SY", "SZ"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tolerance", type=float, default=0.1, help="half width of the value interval around the picked voxel's value")
    ap.add_argument("--vol-n", type=int, default=0, help="volume side instead of the workload's (rehearsals)")
    ap.add_argument("--cpu", action="store_true", help="also time scipy.ndimage.distance_transform_edt on the downloaded mask")
    args = ap.parse_args()
    n, W, H, vname = wl.WORKLOADS[args.workload]
    n = args.vol_n or n
    if vname not in ("BASIC", "LIGHT"):
        raise SystemExit("dist_bench: a workload that vr_pick can be asked about (BASIC or LIGHT)")
    app = host.Application(W, H, 0)
    wl.build_scene(app, args.workload, vol_n=args.vol_n, quiet=True)
    app.OnRender()
    ctx = app.context()
    p = pick_near_centre(app, W, H)
    seed = tuple(int(c) for c in p.voxel)
    value = float(p.value[0][3])
    grown = ctx.segment_grow(ctx.grow_whole(0, 1, 0, value - args.tolerance, value + args.tolerance).copy(seeds=[seed]))
    print(json.dumps(dict(workload=args.workload, volume=n, seed=seed, value=round(value, 6), grown_voxels=int(grown.voxels),
                          grown_lo=list(grown.lo), grown_hi=list(grown.hi), mode=args.mode, limit_um=args.limit_um,
                          spacing_um=list(args.spacing_um), kept_form="settled (every flavour but 1)")), flush=True)
    d = ctx.dist_whole(1, 0, 1, 3, MODES[args.mode]).copy(spacing=args.spacing_um, limit=args.limit_um, scale=0.001)
    first = None
    for flavour, form in ((0, "settled"), (1, "plain")):
        ctx.set_kernel_flavour(flavour)
        for _ in range(args.warmup):
            res = ctx.mask_distance(d)
        wall, phases = [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            res = ctx.mask_distance(d)
            wall.append((time.perf_counter() - t0) * 1e3)
            phases.append(ctx.dist_timing())
        box, computed, rest = ctx.dist_counters()
        channel = ctx.volume_download(1, (n, n, n))[..., 3].copy()
        if first is None:
            first = channel
        med = [round(statistics.median(ph[i] for ph in phases), 4) for i in range(4)]
        finite = channel[np.isfinite(channel)]
        print(json.dumps(dict(workload=args.workload, form=form, mode=args.mode, limit_um=args.limit_um, wall_ms=round(statistics.median(wall), 3),
                              wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3),
                              pack_ms=med[0], passes_ms=med[1], write_ms=med[2], refresh_ms=med[3],
                              src_voxels=int(res.src_voxels), lo=list(res.lo), hi=list(res.hi), beyond=int(res.beyond),
                              box=box, computed=computed, rest=rest, channel_min=float(finite.min()), channel_max=float(finite.max()),
                              equals_settled=bool(np.array_equal(channel.view(np.uint32), first.view(np.uint32))))), flush=True)
        del channel
    ctx.set_kernel_flavour(0)
    times = []
    for _ in range(1 + max(1, args.steps // 3)):
        t0 = time.perf_counter()
        v = ctx.volume_download(1, (n, n, n))
        times.append((time.perf_counter() - t0) * 1e3)
        mask = v[..., 0] != 0.0
        del v
    print(json.dumps(dict(workload=args.workload, case="vr_volume_download of the slot", bytes=16 * n ** 3,
                          ms=round(statistics.median(times[1:]), 1), first_ms=round(times[0], 1))), flush=True)
    if args.cpu:
        import scipy.ndimage as ndi
        sampling = tuple(float(s) for s in args.spacing_um[::-1])
        t0 = time.perf_counter()
        out = ndi.distance_transform_edt(~mask, sampling=sampling)
        t_out = (time.perf_counter() - t0) * 1e3
        t_in = 0.0
        if args.mode != "outside":
            t0 = time.perf_counter()
            ndi.distance_transform_edt(mask, sampling=sampling)
            t_in = (time.perf_counter() - t0) * 1e3
        print(json.dumps(dict(workload=args.workload, case="scipy.ndimage.distance_transform_edt on this host (float64, no limit)",
                              outside_field_ms=round(t_out, 1), inside_field_ms=round(t_in, 1), max_um=float(out.max()))), flush=True)
    app.close()


if __name__ == "__main__":
    main()
