#!/usr/bin/env python3
"""Speed of the device histograms (vr_histogram_async, csrc/vr_hist.h) on a BASELINE configuration.

    python tools/hist_bench.py --workload C3 [--steps 40] [--warmup 10]

The scene is workloads.build_scene's (its volume and preparation); the histograms are of volume slot 0, at 256 and 4096 bins.
Launches: the whole volume unmasked, a sub-box that is not brick-aligned, and the whole volume through a synthetic four-contour mask in
volume slot 1 (all five rows, and the contour rows alone) -- each in the default form (flavour 0: combining and exact settling) and in
the plain form (flavour 1).  For each case one JSON line: ms per launch (wall clock around K launches on one stream behind W warm-up
launches, one synchronisation at the end), the voxels of the box, loaded and settled, the bytes the launch must read -- 4 per loaded
value (16-byte voxels where there is no density plane to read), 16 per mask voxel, 8 per range record -- over that time, the same for
the plain form and the ratio of the two times; whether the two forms' outputs are equal.  Then the host surface's single-threaded
OpacityTF::ActivateHistogram on the same voxels, in ms, per bin count, and whether the device overload returns the same table (it
does not once a bin passes 2^24 voxels, where the host's float count saturates)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from volumerendering_amd import capi, host, workloads as wl  # noqa: E402


def synthetic_mask(n):
    """Four contours in a cube of n^3: a central organ, a shell-like slab that overlaps it, a small target, and an empty one."""
    m = np.zeros((n, n, n, 4), np.float32)
    a, b = n // 4, 3 * n // 4
    m[a:b, a:b, a:b, 0] = 1.0
    m[n // 3:n // 2, :, a:, 1] = 1.0
    c = n // 2
    m[c - n // 16:c + n // 16, c - n // 16:c + n // 16, c - n // 16:c + n // 16, 2] = 1.0
    return m


def cases(ctx, n, bins):
    whole = ctx.hist_whole(0, bins, float(bins))
    yield "whole", whole
    yield "sub-box", whole.copy(lo=(n // 8 + 1, n // 8 + 2, n // 8 + 3), hi=(n - n // 8 - 1, n - n // 8 - 2, n - n // 8 - 3))
    yield "masked 5 rows", whole.copy(mask_slot=1, rows=0b11111)
    yield "masked contours", whole.copy(mask_slot=1, rows=0b11110)


def main():
    ap = argparse.ArgumentParser(description="Speed of the device histograms (vr_histogram_async) on a baseline workload: whole volume, "
                                             "sub-box and masked, default form against the plain one, and the host histogram.")
    ap.add_argument("--workload", default="C3", choices=sorted(wl.WORKLOADS))
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--vol-n", type=int, default=0, help="volume side instead of the workload's (rehearsals)")
    args = ap.parse_args()
    n, W, H, _ = wl.WORKLOADS[args.workload]
    n = args.vol_n or n
    app = host.Application(W, H, 0)
    _, vols = wl.build_scene(app, args.workload, vol_n=args.vol_n, quiet=True)
    ctx = app.context()
    ctx.volume_upload(1, synthetic_mask(n))
    out = capi.Context(256, 256, 0)  # 1 MiB of device memory: counts, then rows
    stream = ctx.stream(0)

    def measure(d, flavour):
        ctx.set_kernel_flavour(flavour)
        d_counts = out.frame_device_ptr()
        d_rows = d_counts + capi.HIST_ROWS * d.bins * 8
        for _ in range(args.warmup):
            ctx.histogram_async(d, d_counts, d_rows, stream)
        ctx.hist_counters()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ctx.histogram_async(d, d_counts, d_rows, stream)
        box, loaded, settled = ctx.hist_counters()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        plane = d.channel == 3 and d.mask_slot < 0
        must_read = loaded * (4 if plane else 16) + (box * 16 if d.mask_slot >= 0 else 0) + (settled // 64 + (loaded + 63) // 64) * 8 * (flavour != 1 and plane)
        return dict(ms=round(ms, 4), box=box, loaded=loaded, settled=settled, must_read_mb=round(must_read / 1e6, 2),
                    gb_s=round(must_read / ms * 1e-6, 1) if ms > 0 else None, gvoxels_s=round(box / ms * 1e-6, 2) if ms > 0 else None)

    for bins in (256, 4096):
        for name, d in cases(ctx, n, bins):
            ctx.set_kernel_flavour(0)
            a = ctx.histogram(d)
            default = measure(d, 0)
            ctx.set_kernel_flavour(1)
            b = ctx.histogram(d)
            plain = measure(d, 1)
            same = bool(np.array_equal(a[0], b[0]) and a[1] == b[1])
            print(json.dumps(dict(workload=args.workload, case=name, bins=bins, **default, plain=plain,
                                  default_speedup=round(plain["ms"] / default["ms"], 3), forms_equal=same)), flush=True)
    ctx.set_kernel_flavour(0)
    for bins in (256, 4096):
        tf = host.OpacityTF(bins)
        t0 = time.perf_counter()
        h = tf.ActivateHistogram(vols[0])
        ms = (time.perf_counter() - t0) * 1e3
        dev = tf.ActivateHistogramDevice(ctx, 0, vols[0].IsNormalized(), vols[0].GetDataRange())
        print(json.dumps(dict(workload=args.workload, case="host ActivateHistogram", bins=bins, ms=round(ms, 1),
                              device_overload_equal=bool(np.array_equal(h, dev)))), flush=True)
    out.close()
    app.close()


if __name__ == "__main__":
    main()
