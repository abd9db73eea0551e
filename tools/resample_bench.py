#!/usr/bin/env python3
"""Speed of resampling a volume slot onto another grid (vr_volume_resample, csrc/vr_resample.h) on a BASELINE configuration.

    python tools/resample_bench.py --workload C4 [--steps 10] [--warmup 3] [--no-cpu] [--out profiles/NAME.json]

The scene is workloads.build_scene's: C4 holds a four-contour mask (slot 0) and a CT (slot 2) of N^3 voxels and a dose of 128 x 128 x 64
(slot 1).  The scene carries no patient geometry, so the bench gives it one: the CT and the mask on a grid of 1 mm from the origin (512 / N mm with --vol-n), the
dose on a grid of 3 x 3 x 6 mm whose voxel (0, 0, 0) lies at (64.4, 60.2, 70.7) mm, inside the CT.  Three legs:

  a  the dose onto the CT's grid, component 3, LINEAR, into slot 0 -- in the default form and the plain one (flavour 1)
  b  the CT onto its own grid rotated by 10 degrees about z through its centre, LINEAR, into slot 0: component 3, and all four
  c  the mask onto the dose's grid, NEAREST, all four components, into slot 1 (the dose is uploaded again behind it)

One JSON line per leg and form: the medians over K calls behind W warm-up calls of the call's wall clock (it is synchronous) and of its
four phases on the device (vr_resample_timing: the source's range records, the kernel, the result words, the rebuild of what is derived
from the destination), the result, the counters and loaded / box, and the kernel's rate against the bytes it MUST move: must-write =
the box's voxels x 4 bytes x the components written; must-read = the source's voxels x 4 bytes x the components read, each once -- or the inside voxels' corners (eight, NEAREST
one) where those are fewer (a destination that covers the source touches all of it; the gather's real traffic is what the caches
leave of the corners).  Then the path the call replaces: vr_volume_download of the source and vr_volume_upload of the destination, timed, and, where
scipy imports, scipy.ndimage.affine_transform(order=1) of component 3 on this host for legs a and b."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from volumerendering_amd import capi, host, workloads as wl  # noqa: E402


def rotation_z(degrees, centre):
    """The row-major 3 x 4 map p -> R (p - centre) + centre for a rotation about z."""
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    centre = np.asarray(centre, np.float64)
    return np.concatenate([R, (centre - R @ centre)[:, None]], axis=1)


def main():
    ap = argparse.ArgumentParser(description="Speed of vr_volume_resample on a baseline workload: dose onto CT, CT rotated onto itself, "
                                             "mask onto the dose grid, phase by phase, against download + scipy + upload.")
    ap.add_argument("--workload", default="C4", choices=["C4"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vol-n", type=int, default=0, help="volume side instead of the workload's (rehearsals)")
    ap.add_argument("--no-cpu", action="store_true", help="do not time scipy.ndimage.affine_transform on this host")
    ap.add_argument("--out", default="", help="also write the JSON lines to this file")
    args = ap.parse_args()
    n, W, H, _ = wl.WORKLOADS[args.workload]
    n = args.vol_n or n
    lines = []

    def emit(**kv):
        lines.append(json.dumps(kv))
        print(lines[-1], flush=True)

    app = host.Application(W, H, 0)
    _, vols = wl.build_scene(app, args.workload, vol_n=args.vol_n, quiet=True)
    ctx = app.context()
    dn = vols[1].GetSize()  # the dose's (nx, ny, nz)
    mm = 512.0 / n  # (a rehearsal's smaller CT covers the same 512 mm)
    ct_grid = capi.Grid.of((n, n, n), (0.0, 0.0, 0.0), (mm, mm, mm))
    dose_grid = capi.Grid.of(dn, (64.4, 60.2, 70.7), (3.0, 3.0, 6.0))
    centre = [(n - 1) / 2.0 * mm] * 3
    dose_host = ctx.volume_download(1, (dn[2], dn[1], dn[0]))
    emit(workload=args.workload, volume=n, dose=list(dn), steps=args.steps, warmup=args.warmup,
         geometry="CT / mask 1 mm from 0; dose 3 x 3 x 6 mm from (64.4, 60.2, 70.7) mm; leg b: 10 degrees about z through the CT's centre")

    def leg(name, d, src_voxels, flavours):
        nch = bin(int(d.channels)).count("1")
        first = None
        for flavour, form in flavours:
            ctx.set_kernel_flavour(flavour)
            for _ in range(args.warmup):
                res = ctx.volume_resample(d)
            wall, phases = [], []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                res = ctx.volume_resample(d)
                wall.append((time.perf_counter() - t0) * 1e3)
                phases.append(ctx.resample_timing())
            box, loaded, unloaded = ctx.resample_counters()
            nx, ny, nz = tuple(d.dst_n)
            out = ctx.volume_download(d.dst_slot, (nz, ny, nx)).view(np.uint32)
            if first is None:
                first = out
            med = [statistics.median(ph[i] for ph in phases) for i in range(4)]
            corners = int(res.inside) * (1 if int(d.filter) == capi.RESAMPLE_NEAREST else 8)
            must_write, must_read = box * 4 * nch, min(src_voxels, corners) * 4 * nch
            k = max(med[1], 1e-6) * 1e-3
            emit(workload=args.workload, leg=name, form=form, channels=int(d.channels), filter=["linear", "nearest"][int(d.filter)],
                 wall_ms=round(statistics.median(wall), 3), wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3),
                 prepare_ms=round(med[0], 4), kernel_ms=round(med[1], 4), words_ms=round(med[2], 4), refresh_ms=round(med[3], 4),
                 inside=int(res.inside), outside=int(res.outside), lo=list(res.lo), hi=list(res.hi), box=box, loaded=loaded,
                 unloaded=unloaded, loaded_of_box=round(loaded / max(box, 1), 4), must_write_bytes=must_write, must_read_bytes=must_read,
                 must_write_gbs=round(must_write / k / 1e9, 1), must_read_gbs=round(must_read / k / 1e9, 1),
                 must_move_gbs=round((must_write + must_read) / k / 1e9, 1), equals_first_form=bool(np.array_equal(out, first)))
            del out
        ctx.set_kernel_flavour(0)

    both = ((0, "default"), (1, "plain"))
    dose_voxels, ct_voxels = dn[0] * dn[1] * dn[2], n ** 3
    # c first: it reads the mask as the scene left it; the dose goes back into its slot behind it
    leg("c: mask onto the dose grid", capi.resample_between(ct_grid, dose_grid, None, src_slot=0, dst_slot=1, channels=15, filter=capi.RESAMPLE_NEAREST),
        ct_voxels, both)
    ctx.volume_upload(1, dose_host)
    leg("a: dose onto the CT grid", capi.resample_between(dose_grid, ct_grid, None, src_slot=1, dst_slot=0, channels=8), dose_voxels, both)
    rot = rotation_z(10.0, centre)
    for channels in (8, 15):
        leg("b: CT rotated 10 degrees about z onto its own grid", capi.resample_between(ct_grid, ct_grid, rot, src_slot=2, dst_slot=0, channels=channels),
            ct_voxels, both)

    # the path the call replaces: download, the host's resampler, upload
    for slot, shape, what in ((1, (dn[2], dn[1], dn[0]), "dose"), (2, (n, n, n), "CT")):
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            v = ctx.volume_download(slot, shape)
            times.append((time.perf_counter() - t0) * 1e3)
        emit(workload=args.workload, case=f"vr_volume_download of the {what}", bytes=int(v.nbytes), ms=round(statistics.median(times[1:]), 1),
             first_ms=round(times[0], 1))
        if what == "CT":
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                ctx.volume_upload(0, v)
                times.append((time.perf_counter() - t0) * 1e3)
            emit(workload=args.workload, case="vr_volume_upload of a volume of the CT's size (with the rebuild)", bytes=int(v.nbytes),
                 ms=round(statistics.median(times[1:]), 1), first_ms=round(times[0], 1))
            ct_a = np.ascontiguousarray(v[..., 3])
        del v
    if not args.no_cpu:
        try:
            import scipy.ndimage as ndi
        except ImportError:
            ndi = None
            emit(workload=args.workload, case="scipy.ndimage.affine_transform on this host", ms=None, note="scipy does not import here")
        if ndi is not None:
            # arrays are (z, y, x): output index o -> input index M o + t, in voxels
            sd, sc = np.array(dose_grid.spacing)[::-1], np.array(ct_grid.spacing)[::-1]
            od, oc = np.array(dose_grid.origin)[::-1], np.array(ct_grid.origin)[::-1]
            t0 = time.perf_counter()
            ndi.affine_transform(np.ascontiguousarray(dose_host[..., 3]), sc / sd, (oc - od) / sd, output_shape=(n, n, n), order=1, mode="nearest")
            t_a = (time.perf_counter() - t0) * 1e3
            R = rot[:, :3][::-1, ::-1]
            t = (rot[:, 3][::-1] + R @ oc - oc) / sc
            t0 = time.perf_counter()
            ndi.affine_transform(ct_a, R, t, output_shape=(n, n, n), order=1, mode="nearest")
            t_b = (time.perf_counter() - t0) * 1e3
            emit(workload=args.workload, case="scipy.ndimage.affine_transform(order=1) of component 3 on this host (one thread, float32)",
                 leg_a_ms=round(t_a, 1), leg_b_ms=round(t_b, 1))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    app.close()


if __name__ == "__main__":
    main()
