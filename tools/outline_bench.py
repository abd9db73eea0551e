#!/usr/bin/env python3
"""Speed of contour tracing (vr_mask_outlines, csrc/vr_outline.h) on the grid of a BASELINE configuration.

    python tools/outline_bench.py --workload C3 [--steps 10] [--warmup 2] [--tolerance 0.1] [--points 300] [--seed 7]

Two masks on the workload's volume (C3: 512^3), both made on the device: the contour that grow_bench.py grows from a picked voxel
(contour 0 of volume slot 1), and the four structures that raster_bench.py rasterises (its seeded structure set, in micrometres on a
grid of 1 x 1 mm, contours 0 .. 3 of volume slot 2).  For each mask, both kernel forms (flavour 0: the doubling rounds stop after the
first one that changes nothing; flavour 1: ceil(log2(corners)) rounds) and both connect rules one JSON line: the medians over K calls
behind W warm-up calls of the wall clock of Context.mask_outlines (the counting call, the allocation and the call that stores) and of
the storing call's four phases on the device (vr_outlines_timing: pack, corners + scan + link, doubling rounds, emit + copy back), the
corner nodes, polygons and rounds, and whether the output equals the first form's.  Then what a caller pays without the call: the time
of a vr_volume_download of the mask slot, and a numpy tracer (tests/outline_ref.py) timed on ONE slice, the middle one, and
EXTRAPOLATED to the slices of the volume -- an estimate, labelled as such, not a measurement of a whole-volume host trace."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # outline_ref.py: the numpy tracer
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import grow_bench  # noqa: E402
import raster_bench  # noqa: E402
from volumerendering_amd import capi, host, workloads as wl  # noqa: E402


def structures_um(n, points, seed):
    """raster_bench's four structures as (points int32 (N, 2) in micrometres, polygons) on a grid of 1000 x 1000 um off the origin."""
    pts, polys, first = [], [], 0
    for k, contour in enumerate(raster_bench.structure_set(n, points, seed)[:4]):
        for p in contour:
            q = p.reshape(-1, 3).astype(np.float64)
            pts.append(np.rint(q[:, :2] * 1000.0).astype(np.int32))
            polys.append((first, len(q), int(round(q[0, 2] / raster_bench.SPACING_MM[2])), k))
            first += len(q)
    return np.concatenate(pts), polys


def main():
    ap = argparse.ArgumentParser(description="Speed of contour tracing (vr_mask_outlines) on a baseline grid: a grown contour and four "
                                             "rasterised structures, both kernel forms and connect rules, phase by phase, against a "
                                             "download of the mask and a numpy tracer.")
    ap.add_argument("--workload", default="C3", choices=sorted(wl.WORKLOADS))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tolerance", type=float, default=0.1, help="half width of the grown value interval (grow_bench.py)")
    ap.add_argument("--points", type=int, default=300, help="points per polygon of the structure set (raster_bench.py)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--vol-n", type=int, default=0, help="volume side instead of the workload's (rehearsals)")
    args = ap.parse_args()
    n, W, H, vname = wl.WORKLOADS[args.workload]
    n = args.vol_n or n
    if vname not in ("BASIC", "LIGHT"):
        raise SystemExit("outline_bench: a workload that vr_pick can be asked about (BASIC or LIGHT)")
    app = host.Application(W, H, 0)
    wl.build_scene(app, args.workload, vol_n=args.vol_n, quiet=True)
    app.OnRender()
    ctx = app.context()
    p = grow_bench.pick_near_centre(app, W, H)
    value = float(p.value[0][3])
    grown = ctx.segment_grow(ctx.grow_whole(0, 1, 0, value - args.tolerance, value + args.tolerance).copy(seeds=[tuple(int(c) for c in p.voxel)]))
    points, polygons = structures_um(n, args.points, args.seed)
    rd = ctx.polygons_whole(0, 2).copy(contours=15, spacing=(1000, 1000))
    rastered = ctx.mask_polygons(rd, points, polygons)
    print(json.dumps(dict(workload=args.workload, volume=n, grown_voxels=int(grown.voxels), structure_voxels=[int(v) for v in rastered.voxels],
                          structure_polygons=len(polygons))), flush=True)
    masks = (("grown contour", ctx.outlines_whole(1)), ("four structures", ctx.outlines_whole(2).copy(contours=15, spacing=(1000, 1000), offset=(500, 500))))
    for name, base in masks:
        first = {}
        for flavour, form in ((0, "until stable"), (1, "fixed rounds")):
            ctx.set_kernel_flavour(flavour)
            for connect, rule in ((capi.OUTLINE_SPLIT, "split"), (capi.OUTLINE_JOIN, "join")):
                d = base.copy(connect=connect)
                for _ in range(args.warmup):
                    out = ctx.mask_outlines(d)
                wall, phases = [], []
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    out = ctx.mask_outlines(d)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    phases.append(ctx.outlines_timing())
                nodes, polys, rounds = ctx.outlines_counters()
                ref = first.setdefault(connect, out)
                med = [round(statistics.median(ph[i] for ph in phases), 4) for i in range(4)]
                print(json.dumps(dict(workload=args.workload, mask=name, form=form, connect=rule, wall_ms=round(statistics.median(wall), 3),
                                      wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3), pack_ms=med[0], link_ms=med[1],
                                      rounds_ms=med[2], emit_ms=med[3], device_ms=round(sum(med), 4), nodes=nodes, polygons=polys, rounds=rounds,
                                      area2=[int(a) for a in out[2].area2],
                                      equals_first_form=bool(np.array_equal(out[0], ref[0]) and out[1] == ref[1]))), flush=True)
    ctx.set_kernel_flavour(0)
    # without the call: the download, and a numpy tracer on one slice
    import outline_ref as orf
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        v = ctx.volume_download(2, (n, n, n))
        times.append((time.perf_counter() - t0) * 1e3)
    mid = orf.members(v[n // 2:n // 2 + 1])
    del v
    t0 = time.perf_counter()
    got = orf.trace(mid, 15, orf.SPLIT, (0, 0, 0), (n, n, 1), (0, 0), (1000, 1000), (500, 500))
    one = (time.perf_counter() - t0) * 1e3
    print(json.dumps(dict(workload=args.workload, case="vr_volume_download of the mask slot + numpy tracer", bytes=16 * n ** 3,
                          download_ms=round(statistics.median(times[1:]), 1), download_first_ms=round(times[0], 1),
                          numpy_one_slice_ms=round(one, 1), numpy_one_slice_points=got["result"][0],
                          numpy_all_slices_ms_EXTRAPOLATED=round(one * n, 0),
                          note="the last figure is one slice's time multiplied by the slices of the volume: an extrapolation, not a measurement")), flush=True)
    app.close()


if __name__ == "__main__":
    main()
