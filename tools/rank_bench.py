#!/usr/bin/env python3
"""Speed of the rank filters (vr_volume_rank, csrc/vr_rank.h) on a BASELINE configuration.

    python tools/rank_bench.py --workload C3 [--steps 5] [--warmup 1] [--host r1|all|none] [--out profiles/rank_bench_C3.json]

The scene is workloads.build_scene's (its volume and preparation).  Channel 3 of volume slot 0 (the CT) is rank-filtered into channel 3
of volume slot 1, over the whole volume: the median at radius 1, 2 and 3, the median at radii (2, 2, 1) -- 2 mm on a grid of
1 x 1 x 3 mm -- and the minimum and the maximum at radius 2.  Two more cases put the default form's generic path on the legs of its two
specialised ones: rank 12 of the 3 x 3 x 3 window (the descent costs the same at every rank; the median, rank 13, takes the network) and
rank 1 of the 5 x 5 x 5 window (rank 0 takes the running minima).  For every case and both kernel forms (flavour 0: LDS tiles; flavour 1:
one lane per output, every input from memory) one JSON line: the medians over K calls behind W warm-up calls of the call's wall clock (it
is synchronous) and of its phases on the device (vr_rank_timing: the selection kernel, the write with the result words, the trailing
rebuild of what is derived from the slot), the result, the counters, whether the channel equals the first form's, the voxels selected per
second, and the bytes the selection must move -- every line of the float4 source once, 16 B a voxel, and the field out, 4 B -- with the
rate that makes and its share of the MI355X's 8 TB/s.  Then, unless --host none, the route the call replaces on this machine:
vr_volume_download of the slot, scipy.ndimage.median_filter (mode="nearest", float32) of the channel and vr_volume_upload into the
second slot, for radius 1 (r1) or for all four medians (all), with whether its channel equals the device's bit for bit.  The lines are
also written, as a JSON list, to --out.  Nothing outside the repository is read."""
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
MEDIANS = [("median r 1", (1, 1, 1), capi.RANK_MEDIAN), ("median r 2", (2, 2, 2), capi.RANK_MEDIAN), ("median r 3", (3, 3, 3), capi.RANK_MEDIAN),
           ("median 2 mm at 1 x 1 x 3 mm", (2, 2, 1), capi.RANK_MEDIAN)]
CASES = MEDIANS + [("minimum r 2", (2, 2, 2), capi.RANK_MIN), ("maximum r 2", (2, 2, 2), capi.RANK_MAX),
                   ("rank 12 of 27: the generic path on the network's leg", (1, 1, 1), 12),
                   ("rank 1 of 125: the generic path on the running minima's leg", (2, 2, 2), 1)]


def main():
    ap = argparse.ArgumentParser(description="Speed of the rank filters (vr_volume_rank) on a baseline workload: medians, minimum and maximum of "
                                             "the CT's channel 3 into a second slot, both kernel forms, phase by phase, against download + scipy + upload.")
    ap.add_argument("--workload", default="C3", choices=sorted(wl.WORKLOADS))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--vol-n", type=int, default=0, help="volume side instead of the workload's (rehearsals)")
    ap.add_argument("--host", default="r1", choices=["r1", "all", "none"], help="the medians the download + scipy + upload route runs")
    ap.add_argument("--out", default=None, help="where the lines are written as a JSON list (default profiles/rank_bench_<workload>.json)")
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
    must = float(n) ** 3 * (16 + 4)
    whole = ctx.rank_whole(0, 3, 1, 3)
    for name, radii, rank in CASES:
        d = whole.copy(radius=radii, rank=rank)
        first = None
        for flavour, form in ((0, "lds tiles"), (1, "plain")):
            ctx.set_kernel_flavour(flavour)
            for _ in range(args.warmup):
                res = ctx.volume_rank(d)
            wall, phases = [], []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                res = ctx.volume_rank(d)
                wall.append((time.perf_counter() - t0) * 1e3)
                phases.append(ctx.rank_timing())
            box, read, k = ctx.rank_counters()
            channel = ctx.volume_download(1, shape)[..., 3].copy()
            if first is None:
                first = channel
            med = [round(statistics.median(ph[i] for ph in phases), 4) for i in range(4)]
            rate = must / (med[0] * 1e-3)
            emit(workload=args.workload, case=name, radii=list(radii), window=(2 * radii[0] + 1) * (2 * radii[1] + 1) * (2 * radii[2] + 1), form=form,
                 wall_ms=round(statistics.median(wall), 3), wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3),
                 selection_ms=med[0], write_ms=med[2], refresh_ms=med[3], device_ms=round(sum(med), 4),
                 gvoxels_per_s=round(box / (med[0] * 1e-3) / 1e9, 3), selection_bytes=int(must), selection_tb_per_s=round(rate / 1e12, 3),
                 selection_of_peak=round(rate / PEAK_BYTES_PER_S, 4),
                 stored=int(res.stored), nonfinite=int(res.nonfinite), changed=int(res.changed), lo_value=float(res.lo_value), hi_value=float(res.hi_value),
                 box=box, read=read, k=k, equals_first_form=bool(np.array_equal(channel.view(np.uint32), first.view(np.uint32))))
            del channel
        del first
    ctx.set_kernel_flavour(0)
    if args.host != "none":
        import scipy.ndimage as ndi
        for name, radii, rank in MEDIANS[:1] if args.host == "r1" else MEDIANS:
            t0 = time.perf_counter()
            v = ctx.volume_download(0, shape)
            t1 = time.perf_counter()
            v[..., 3] = ndi.median_filter(np.ascontiguousarray(v[..., 3]), size=tuple(2 * r + 1 for r in radii[::-1]), mode="nearest")
            t2 = time.perf_counter()
            ctx.volume_upload(1, v)
            t3 = time.perf_counter()
            got = ctx.volume_download(1, shape)[..., 3].copy()
            ctx.volume_rank(whole.copy(radius=radii, rank=rank))
            dev = ctx.volume_download(1, shape)[..., 3]
            emit(workload=args.workload, case=name, radii=list(radii),
                 route="vr_volume_download + scipy.ndimage.median_filter (float32, nearest) + vr_volume_upload on this host",
                 download_ms=round((t1 - t0) * 1e3, 1), scipy_ms=round((t2 - t1) * 1e3, 1), upload_ms=round((t3 - t2) * 1e3, 1),
                 total_ms=round((t3 - t0) * 1e3, 1), equals_the_device=bool(np.array_equal(got.view(np.uint32), dev.view(np.uint32))))
            del v, got, dev
    app.close()
    out = args.out or os.path.join(ROOT, "profiles", f"rank_bench_{args.workload}.json")
    with open(out, "w") as fh:
        json.dump(lines, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
