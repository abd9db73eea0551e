#!/usr/bin/env python3
"""Speed of region growing (vr_segment_grow, csrc/vr_grow.h) on a BASELINE configuration.

    python tools/grow_bench.py --workload C3 [--steps 10] [--warmup 3] [--tolerance 0.1]

The scene is workloads.build_scene's (its volume and preparation).  A vr_pick of the frame's centre (the nearest pixel with a hit)
gives the seed voxel and its value v; the region is the voxels of volume slot 0 with .a in [v - tolerance, v + tolerance] connected to
it, written as contour 0 of volume slot 1 (VR_GROW_REPLACE, the whole volume).  For both kernel forms (flavour 0: range records and
a frontier; flavour 1: every voxel loaded, every brick swept) and both connectivities one JSON line: the medians over K calls behind W
warm-up calls of the call's wall clock (it is synchronous) and of its four phases on the device (vr_grow_timing: classify and seed,
the propagation rounds with the host's looks in between, the write, the trailing rebuild of what is derived from the mask slot), the
rounds, the region's voxels and box, the counters, and whether the mask equals the first case's.  Then the time of a vr_volume_download
of the value slot: what a caller pays today before any segmentation on the CPU can begin."""
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


def pick_near_centre(app, W, H):
    """The first hit on a spiral of pixels around the frame's centre."""
    for r in range(0, min(W, H) // 2, 8):
        for dx, dy in ((0, 0), (r, 0), (-r, 0), (0, r), (0, -r)) if r else ((0, 0),):
            p = app.pick(W // 2 + dx, H // 2 + dy)
            if p.hit:
                return p
    raise SystemExit("grow_bench: no pixel near the centre hits the volume")


def main():
    ap = argparse.ArgumentParser(description="Speed of region growing (vr_segment_grow) on a baseline workload: both kernel forms and "
                                             "connectivities from a picked voxel, phase by phase, against a download of the volume.")
    ap.add_argument("--workload", default="C3", choices=sorted(wl.WORKLOADS))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tolerance", type=float, default=0.1, help="half width of the value interval around the picked voxel's value")
    ap.add_argument("--vol-n", type=int, default=0, help="volume side instead of the workload's (rehearsals)")
    args = ap.parse_args()
    n, W, H, vname = wl.WORKLOADS[args.workload]
    n = args.vol_n or n
    if vname not in ("BASIC", "LIGHT"):
        raise SystemExit("grow_bench: a workload that vr_pick can be asked about (BASIC or LIGHT)")
    app = host.Application(W, H, 0)
    wl.build_scene(app, args.workload, vol_n=args.vol_n, quiet=True)
    app.OnRender()
    ctx = app.context()
    p = pick_near_centre(app, W, H)
    seed = tuple(int(c) for c in p.voxel)
    value = float(p.value[0][3])
    lo, hi = value - args.tolerance, value + args.tolerance
    print(json.dumps(dict(workload=args.workload, volume=n, seed=seed, value=round(value, 6), lo=round(lo, 6), hi=round(hi, 6))), flush=True)
    base = ctx.grow_whole(0, 1, 0, lo, hi).copy(seeds=[seed])
    first = None
    for flavour, form in ((0, "frontier"), (1, "sweep")):
        for conn in (capi.GROW_FACES, capi.GROW_ALL):
            ctx.set_kernel_flavour(flavour)
            d = base.copy(connectivity=conn)
            for _ in range(args.warmup):
                res = ctx.segment_grow(d)
            wall, phases = [], []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                res = ctx.segment_grow(d)
                wall.append((time.perf_counter() - t0) * 1e3)
                phases.append(ctx.grow_timing())
            box, loaded, settled = ctx.grow_counters()
            mask = ctx.volume_download(1, (n, n, n))[..., 0].copy()
            if conn == capi.GROW_FACES and first is None:
                first = mask
            med = [round(statistics.median(ph[i] for ph in phases), 4) for i in range(4)]
            print(json.dumps(dict(workload=args.workload, form=form, connectivity=conn, wall_ms=round(statistics.median(wall), 3),
                                  wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3),
                                  classify_ms=med[0], propagate_ms=med[1], write_ms=med[2], refresh_ms=med[3],
                                  rounds=int(res.rounds), voxels=int(res.voxels), lo=list(res.lo), hi=list(res.hi),
                                  box=box, loaded=loaded, settled=settled,
                                  mask_ones=int((mask == 1.0).sum()),
                                  equals_frontier_faces=bool(np.array_equal(mask, first)) if conn == capi.GROW_FACES else None)), flush=True)
            del mask
    ctx.set_kernel_flavour(0)
    times = []
    for _ in range(1 + max(1, args.steps // 3)):
        t0 = time.perf_counter()
        v = ctx.volume_download(0, (n, n, n))
        times.append((time.perf_counter() - t0) * 1e3)
        del v
    print(json.dumps(dict(workload=args.workload, case="vr_volume_download of the value slot", bytes=16 * n ** 3,
                          ms=round(statistics.median(times[1:]), 1), first_ms=round(times[0], 1))), flush=True)
    app.close()


if __name__ == "__main__":
    main()
