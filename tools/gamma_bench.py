#!/usr/bin/env python3
"""Speed of the gamma index (vr_volume_gamma, csrc/vr_gamma.h) on a BASELINE configuration.

    python tools/gamma_bench.py --workload C4 [--steps 3] [--warmup 1] [--count-box 24] [--out profiles/gamma_bench_C4.json]

The reference dose R is the scene's prepared dose (workloads.build_scene: 128 x 128 x 64 voxels, taken as 4 x 4 x 8 mm over the CT's
512 mm).  The evaluated dose E is R moved by (2, -1.5, 1) mm and magnified by 2 % about the centre; vr_volume_resample makes it on the
device.  Three legs at 3 % of the maximum dose (VR_GAMMA_GLOBAL) / 3 mm with the default reach of 6 mm and a cutoff of 10 % of the
maximum: on the dose grid at sub 1, and on the CT's grid (both doses resampled onto it from the dose grid, 1 mm voxels at 512^3) at sub 1
and at sub 2.  On the CT's grid gamma goes in place into channel 0 of the evaluated slot, since three slots of that size are all there is
room for; the doses stay in channel 3.

Per leg and kernel form (flavour 0: LDS tiles with the exact cut; flavour 1: plain, every candidate from memory) one JSON line: the
medians over K calls behind W warm-up calls of the call's wall clock (it is synchronous) and of its phases on the device
(vr_gamma_timing: the search kernel, the write with the result words, the trailing rebuild of what is derived from the slot), K (the
admitted offsets), the result, the pass rate passed / evaluated, the evaluated voxels per second of the search kernel and whether the
channel equals the default form's.  On the CT's grid both forms run on the whole volume and once more on the central box of a quarter of
the side, every voxel of which is above the cutoff.

The table entries the default form walks are NOT counted by the shipped kernel.  A separate counting run does that on the host: the
numpy restatement (tests/gamma_ref.py) with the exact cut, entry by entry, on two boxes of 32 x B x B voxels (B = --count-box; 0: no
counting run) of each leg, aligned to the kernel's tiles: one at the centre and one a quarter of the way along x, on the dose's flank.
Per box it gives what a lane asks for (the entries whose c is below the voxel's minimum, the mean over evaluated voxels) and what the
kernel's loop executes: a wavefront -- 32 x 2 x 4 outputs -- goes on in step until none of its outputs asks, so its trips are the
maximum over them; the mean of that over the box's wavefronts is the figure that bounds the kernel.

No host gamma is timed: no host implementation (pymedphys) is installed here.  The lines are also written, as a JSON list, to --out.
Nothing outside the repository is read."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from volumerendering_amd import capi, host, workloads as wl  # noqa: E402

SHIFT_MM, SCALE = (2.0, -1.5, 1.0), 1.02
DTA_UM, TOL_FRACTION, CUTOFF_FRACTION = 3000, 0.03, 0.10


def main():
    ap = argparse.ArgumentParser(description="Speed of the gamma index (vr_volume_gamma) on a baseline workload: the dose against itself moved and "
                                             "magnified, on the dose grid and on the CT's grid, both kernel forms, phase by phase.")
    ap.add_argument("--workload", default="C4", choices=["C4"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--vol-n", type=int, default=0, help="side of the CT's grid instead of the workload's (rehearsals)")
    ap.add_argument("--count-box", type=int, default=24, help="y and z side of the boxes of the host's counting run, a multiple of 4 (0: none)")
    ap.add_argument("--out", default=None, help="where the lines are written as a JSON list (default profiles/gamma_bench_<workload>.json)")
    args = ap.parse_args()
    n, W, H, _ = wl.WORKLOADS[args.workload]
    n = args.vol_n or n
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    app = host.Application(W, H, 0)
    _, vols = wl.build_scene(app, args.workload, vol_n=args.vol_n, quiet=True)
    dose = np.array(vols[1].data(), np.float32, copy=True)  # (nz, ny, nx, 4) as the scene prepared it
    app.close()
    top = float(dose[..., 3].max())
    tol, cutoff = np.float32(TOL_FRACTION * top), np.float32(CUTOFF_FRACTION * top)
    dn = (dose.shape[2], dose.shape[1], dose.shape[0])
    extent = 512.0  # mm along every axis, whatever the CT's side
    dose_grid = capi.Grid.of(dn, [extent / d / 2 - 0.5 for d in dn], [extent / d for d in dn])
    ct_grid = capi.Grid.of((n, n, n), [extent / n / 2 - 0.5] * 3, [extent / n] * 3)
    centre = extent / 2 - 0.5
    moved = [SCALE, 0, 0, (1 - SCALE) * centre + SHIFT_MM[0], 0, SCALE, 0, (1 - SCALE) * centre + SHIFT_MM[1], 0, 0, SCALE, (1 - SCALE) * centre + SHIFT_MM[2]]
    emit(workload=args.workload, ct_side=n, dose_grid=list(dn), steps=args.steps, warmup=args.warmup, dose_max=top, tolerance=float(tol), cutoff=float(cutoff),
         dta_um=DTA_UM, reach_um=2 * DTA_UM, shift_mm=list(SHIFT_MM), scale=SCALE, host_gamma="not timed: none is installed")

    ctx = capi.Context(W, H, 0)

    def leg(name, desc, shape, dst, box=None):
        """Both forms of one descriptor, and once more on `box` where one is given."""
        runs = [(0, "lds tiles", desc), (1, "plain", desc)] + ([(0, "lds tiles", box), (1, "plain", box)] if box is not None else [])
        first = None  # the default form's channel over the box the plain form runs on next
        for flavour, form, d in runs:
            ctx.set_kernel_flavour(flavour)
            for _ in range(args.warmup):
                res = ctx.volume_gamma(d)
            wall, phases = [], []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                res = ctx.volume_gamma(d)
                wall.append((time.perf_counter() - t0) * 1e3)
                phases.append(ctx.gamma_timing())
            stored, evaluated, K = ctx.gamma_counters()
            med = [round(statistics.median(ph[i] for ph in phases), 4) for i in range(4)]
            lo, hi = list(d.box_lo), list(d.box_hi)
            channel = ctx.volume_download(dst[0], shape)[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0], dst[1]].copy()
            same = None
            if flavour == 1:
                same = bool(np.array_equal(channel.view(np.uint32), first.view(np.uint32)))
            else:
                first = channel
            emit(workload=args.workload, leg=name, form=form, box=[lo, hi], spacing_um=list(d.spacing), sub=d.sub, K=K,
                 wall_ms=round(statistics.median(wall), 3), search_ms=med[0], write_ms=med[2], refresh_ms=med[3], device_ms=round(sum(med), 4),
                 stored=stored, evaluated=evaluated, passed=int(res.passed), nonfinite=int(res.nonfinite), hi_value=float(res.hi_value),
                 pass_rate=round(int(res.passed) / max(1, evaluated), 6), evaluated_mvoxels_per_s=round(evaluated / (med[0] * 1e-3) / 1e6, 2),
                 candidates_per_evaluated_voxel_without_cut=K, equals_first_form=same)
        ctx.set_kernel_flavour(0)

    def count(name, r_slot, e_slot, shape, d):
        """The counting run: the restatement with the exact cut on two boxes of whole wavefronts (32 x 2 x 4 outputs, as the kernel cuts a
        whole-volume call into them)."""
        if args.count_box <= 0:
            return
        import gamma_ref as gr
        n3 = (shape[2], shape[1], shape[0])
        side = [32, min(args.count_box, n3[1]) // 4 * 4, min(args.count_box, n3[2]) // 4 * 4]
        R = ctx.volume_download(r_slot, shape)[..., 3].copy()
        E = ctx.volume_download(e_slot, shape)[..., 3].copy()
        for where, frac in (("centre", 0.5), ("a quarter along x", 0.25)):
            lo = [int(n3[0] * frac) // 32 * 32, (n3[1] - side[1]) // 2 // 2 * 2, (n3[2] - side[2]) // 2 // 4 * 4]
            hi = [l + b for l, b in zip(lo, side)]
            t0 = time.perf_counter()
            _, skipped, _, K, asked = gr.field(R, E, None, tuple(d.spacing), d.dta, d.reach, d.sub, d.mode, d.dose_tolerance, d.cutoff, lo, hi,
                                               cut=True, chunk=1)
            evaluated = int((~skipped).sum())
            waves = asked.reshape(side[2] // 4, 4, side[1] // 2, 2, 32).max(axis=(1, 3, 4))  # (z, y, x) into wavefronts of 4 x 2 x 32
            emit(workload=args.workload, leg=name, counting_run="tests/gamma_ref.py with the exact cut, entry by entry, on the host", where=where,
                 box=[lo, hi], evaluated=evaluated, K=K, entries_asked_per_evaluated_voxel=round(int(asked.sum()) / max(1, evaluated), 2),
                 entries_walked_per_wavefront_mean=round(float(waves.mean()), 2), entries_walked_per_wavefront_max=int(waves.max()),
                 wavefronts=int(waves.size), seconds=round(time.perf_counter() - t0, 1))

    # the dose grid: R in slot 0, E in slot 1, gamma into channel 0 of slot 2
    dshape = dose.shape[:3]
    ctx.volume_upload(0, dose)
    ctx.volume_resample(capi.resample_between(dose_grid, dose_grid, moved, src_slot=0, dst_slot=1, channels=0xF, filter=capi.RESAMPLE_LINEAR))
    um = [int(round(extent / d * 1000)) for d in dn]
    d = ctx.gamma_whole(0, 3, 1, 3, 2, 0).copy(spacing=um, dta=DTA_UM, reach=2 * DTA_UM, dose_tolerance=tol, cutoff=cutoff)
    leg("dose grid, sub 1", d, dshape, (2, 0))
    count("dose grid, sub 1", 0, 1, dshape, d)

    # the CT's grid: the dose in slot 0, E resampled into slot 1 and R into slot 2, gamma in place into channel 0 of slot 1
    cshape = (n, n, n)
    for slot in (1, 2):  # (a filled destination must have the grid's dimensions: the dose grid's slots give way)
        ctx.volume_upload(slot, np.zeros(cshape + (4,), np.float32))
    ctx.volume_resample(capi.resample_between(dose_grid, ct_grid, moved, src_slot=0, dst_slot=1, channels=0xF, filter=capi.RESAMPLE_LINEAR))
    ctx.volume_resample(capi.resample_between(dose_grid, ct_grid, None, src_slot=0, dst_slot=2, channels=0xF, filter=capi.RESAMPLE_LINEAR))
    q = n // 4
    for sub in (1, 2):
        d = ctx.gamma_whole(2, 3, 1, 3, 1, 0).copy(spacing=[int(round(extent / n * 1000))] * 3, dta=DTA_UM, reach=2 * DTA_UM, sub=sub,
                                                 dose_tolerance=tol, cutoff=cutoff)
        box = d.copy(box_lo=[(n - q) // 2] * 3, box_hi=[(n - q) // 2 + q] * 3)
        leg(f"CT grid, sub {sub}", d, cshape, (1, 0), box)
        count(f"CT grid, sub {sub}", 2, 1, cshape, d)
    ctx.close()
    out = args.out or os.path.join(ROOT, "profiles", f"gamma_bench_{args.workload}.json")
    with open(out, "w") as fh:
        json.dump(lines, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
