#!/usr/bin/env python3
"""Speed of mask morphology (vr_mask_morph, csrc/vr_morph.h) on a BASELINE configuration.

    python tools/morph_bench.py --workload C3 [--op close] [--radius-um 5000] [--spacing-um 1000 1000 3000] [--steps 10] [--warmup 3]

The scene is workloads.build_scene's (its volume and preparation).  As in tools/grow_bench.py a vr_pick of the frame's centre gives a
seed voxel and its value v, and the voxels of volume slot 0 with .a in [v - tolerance, v + tolerance] connected to it become contour 0
of volume slot 1 (vr_segment_grow).  That contour is then put through the operator, with the ball of --radius-um on a grid of
--spacing-um (vr_morph_ball), into contour 1 of the same slot (VR_MORPH_REPLACE, the whole volume).  For both kernel forms (flavour 0:
only the words the result can be set in are computed; flavour 1: every word of the box) one JSON line: the medians over K calls behind
W warm-up calls of the call's wall clock (it is synchronous) and of its four phases on the device (vr_morph_timing: the pack with the
host's look at the bounding box, the dilation launches, the write, the trailing rebuild of what is derived from the slot), the result,
the counters, and whether the mask equals the first form's.  Then the time of a vr_volume_download of the mask slot: what a caller
pays today before any morphology on the CPU can begin."""
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

OPS = {"none": capi.MORPH_NONE, "dilate": capi.MORPH_DILATE, "erode": capi.MORPH_ERODE, "close": capi.MORPH_CLOSE, "open": capi.MORPH_OPEN}


def main():
    ap = argparse.ArgumentParser(description="Speed of mask morphology (vr_mask_morph) on a baseline workload: a grown contour through "
                                             "one operator, both kernel forms, phase by phase, against a download of the volume.")
    ap.add_argument("--workload", default="C3", choices=sorted(wl.WORKLOADS))
    ap.add_argument("--op", default="close", choices=sorted(OPS))
    ap.add_argument("--radius-um", type=int, default=5000)
    ap.add_argument("--spacing-um", type=int, nargs=3, default=[1000, 1000, 3000], metavar=("SX", "SY", "SZ"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tolerance", type=float, default=0.1, help="half width of the value interval around the picked voxel's value")
    ap.add_argument("--vol-n", type=int, default=0, help="volume side instead of the workload's (rehearsals)")
    args = ap.parse_args()
    n, W, H, vname = wl.WORKLOADS[args.workload]
    n = args.vol_n or n
    if vname not in ("BASIC", "LIGHT"):
        raise SystemExit("morph_bench: a workload that vr_pick can be asked about (BASIC or LIGHT)")
    element = capi.morph_ball(args.spacing_um, args.radius_um)
    app = host.Application(W, H, 0)
    wl.build_scene(app, args.workload, vol_n=args.vol_n, quiet=True)
    app.OnRender()
    ctx = app.context()
    p = pick_near_centre(app, W, H)
    seed = tuple(int(c) for c in p.voxel)
    value = float(p.value[0][3])
    grown = ctx.segment_grow(ctx.grow_whole(0, 1, 0, value - args.tolerance, value + args.tolerance).copy(seeds=[seed]))
    print(json.dumps(dict(workload=args.workload, volume=n, seed=seed, value=round(value, 6), grown_voxels=int(grown.voxels),
                          grown_lo=list(grown.lo), grown_hi=list(grown.hi), op=args.op, radius_um=args.radius_um,
                          spacing_um=list(args.spacing_um), radii=list(element.radius), kept_form="settled (every flavour but 1)")), flush=True)
    d = ctx.morph_whole(1, 0, 1, 1, OPS[args.op]).copy(element=element)
    first = None
    for flavour, form in ((0, "settled"), (1, "plain")):
        ctx.set_kernel_flavour(flavour)
        for _ in range(args.warmup):
            res = ctx.mask_morph(d)
        wall, phases = [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            res = ctx.mask_morph(d)
            wall.append((time.perf_counter() - t0) * 1e3)
            phases.append(ctx.morph_timing())
        box, computed, settled = ctx.morph_counters()
        mask = ctx.volume_download(1, (n, n, n))[..., 1].copy()
        if first is None:
            first = mask
        med = [round(statistics.median(ph[i] for ph in phases), 4) for i in range(4)]
        print(json.dumps(dict(workload=args.workload, form=form, op=args.op, wall_ms=round(statistics.median(wall), 3),
                              wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3),
                              pack_ms=med[0], morph_ms=med[1], write_ms=med[2], refresh_ms=med[3],
                              voxels=int(res.voxels), src_voxels=int(res.src_voxels), lo=list(res.lo), hi=list(res.hi),
                              box=box, computed=computed, settled=settled, mask_ones=int((mask == 1.0).sum()),
                              equals_settled=bool(np.array_equal(mask, first)))), flush=True)
        del mask
    ctx.set_kernel_flavour(0)
    times = []
    for _ in range(1 + max(1, args.steps // 3)):
        t0 = time.perf_counter()
        v = ctx.volume_download(1, (n, n, n))
        times.append((time.perf_counter() - t0) * 1e3)
        del v
    print(json.dumps(dict(workload=args.workload, case="vr_volume_download of the mask slot", bytes=16 * n ** 3,
                          ms=round(statistics.median(times[1:]), 1), first_ms=round(times[0], 1))), flush=True)
    app.close()


if __name__ == "__main__":
    main()
