#!/usr/bin/env python3
"""Speed of connected components (vr_mask_components, csrc/vr_comp.h) on the grid of a BASELINE configuration.

    python tools/comp_bench.py --workload C3 [--steps 5] [--warmup 1] [--tolerance 0.1]

Three calls on the workload's volume (C3: 512^3):
  table      the table-only call (the counting call, then the one that fills the table) on the contour that grow_bench.py grows from a
             picked voxel (contour 0 of volume slot 1);
  largest    keep_largest = 1 of a plain threshold mask (.a of the volume >= the picked value - tolerance, made on the host once and
             uploaded as contour 0 of volume slot 2), written into contour 1 of the same slot;
  fill holes the components of that mask's complement that touch no face of the volume, ORed into contour 2 of the same slot.
For each one JSON line: the medians over K calls behind W warm-up calls of the wall clock of the call (Context.mask_components for the
first, one vr_mask_components for the others) and of its four phases on the device (vr_components_timing: pack; runs + scan + merge +
flatten; numbering .. copy back; the rebuild of what is derived from the written slot), the result and the counters.  Then what a caller
pays without the call: the time of a vr_volume_download of the mask slot, and, where scipy is importable, scipy.ndimage.label of the
same threshold mask on this host (its count must equal the device's)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import grow_bench  # noqa: E402
from volumerendering_amd import capi, host, workloads as wl  # noqa: E402


def timed(ctx, call, steps, warmup):
    """(median wall ms, min, max, the medians of the four phases, what the last call returned)"""
    for _ in range(warmup):
        out = call()
    wall, phases = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        phases.append(ctx.components_timing())
    med = [round(statistics.median(ph[i] for ph in phases), 4) for i in range(4)]
    return round(statistics.median(wall), 3), round(min(wall), 3), round(max(wall), 3), med, out


def main():
    ap = argparse.ArgumentParser(description="Speed of connected components (vr_mask_components) on a baseline grid: the table of a grown "
                                             "contour, keep-largest of a threshold mask and 3-D hole filling, phase by phase, against a "
                                             "download of the mask and scipy.ndimage.label.")
    ap.add_argument("--workload", default="C3", choices=sorted(wl.WORKLOADS))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tolerance", type=float, default=0.1, help="half width of the grown value interval (grow_bench.py)")
    ap.add_argument("--vol-n", type=int, default=0, help="volume side instead of the workload's (rehearsals)")
    args = ap.parse_args()
    n, W, H, vname = wl.WORKLOADS[args.workload]
    n = args.vol_n or n
    if vname not in ("BASIC", "LIGHT"):
        raise SystemExit("comp_bench: a workload that vr_pick can be asked about (BASIC or LIGHT)")
    app = host.Application(W, H, 0)
    wl.build_scene(app, args.workload, vol_n=args.vol_n, quiet=True)
    app.OnRender()
    ctx = app.context()
    p = grow_bench.pick_near_centre(app, W, H)
    value = float(p.value[0][3])
    grown = ctx.segment_grow(ctx.grow_whole(0, 1, 0, value - args.tolerance, value + args.tolerance).copy(seeds=[tuple(int(c) for c in p.voxel)]))
    v = ctx.volume_download(0, (n, n, n))
    above = v[..., 3] >= np.float32(value - args.tolerance)
    del v
    mask = np.zeros((n, n, n, 4), np.float32)
    mask[..., 0] = above
    ctx.volume_upload(2, mask)
    del mask
    print(json.dumps(dict(workload=args.workload, volume=n, grown_voxels=int(grown.voxels), threshold=round(value - args.tolerance, 6),
                          threshold_voxels=int(above.sum()))), flush=True)

    def one(d):
        out = capi.ComponentsResult()
        ctx._chk(ctx.lib.vr_mask_components(ctx.h, C.byref(d), C.byref(out)))
        return out

    whole2 = ctx.components_whole(2, 0)
    cases = (("table", "grown contour", lambda: ctx.mask_components(ctx.components_whole(1, 0))["result"]),
             ("largest", "threshold mask", lambda: one(whole2.copy(keep_largest=1, dst_slot=2, dst_contour=1))),
             ("fill holes", "threshold mask", lambda: one(whole2.copy(background=1, reject_faces=63, dst_slot=2, dst_contour=2, combine=capi.MORPH_OR))))
    device_count = None
    for name, what, call in cases:
        wall, lo, hi, med, out = timed(ctx, call, args.steps, args.warmup)
        box, nodes, pairs = ctx.components_counters()
        if name == "largest":
            device_count = int(out.n_components)
        print(json.dumps(dict(workload=args.workload, case=name, mask=what, wall_ms=wall, wall_ms_min=lo, wall_ms_max=hi, pack_ms=med[0],
                              merge_ms=med[1], number_ms=med[2], refresh_ms=med[3], device_ms=round(sum(med), 4),
                              n_components=int(out.n_components), n_selected=int(out.n_selected), voxels=int(out.voxels),
                              selected_voxels=int(out.selected_voxels), largest=int(out.largest), box=box, nodes=nodes, pairs=pairs)), flush=True)
    # without the call: the download, and scipy on the host
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        v = ctx.volume_download(2, (n, n, n))
        times.append((time.perf_counter() - t0) * 1e3)
        del v
    line = dict(workload=args.workload, case="vr_volume_download of the mask slot", bytes=16 * n ** 3,
                download_ms=round(statistics.median(times[1:]), 1), download_first_ms=round(times[0], 1))
    try:
        from scipy import ndimage
    except ImportError:
        line["scipy"] = "not importable on this host"
    else:
        t0 = time.perf_counter()
        _, count = ndimage.label(above)
        line.update(scipy_label_ms=round((time.perf_counter() - t0) * 1e3, 1), scipy_components=int(count),
                    scipy_equals_device=bool(count == device_count))
    print(json.dumps(line), flush=True)
    app.close()


if __name__ == "__main__":
    main()
