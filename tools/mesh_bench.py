#!/usr/bin/env python3
"""Speed of surface extraction (vr_volume_mesh, csrc/vr_mesh.h) on the grid of a BASELINE configuration.

    python tools/mesh_bench.py --workload C3 [--steps 10] [--warmup 2] [--tolerance 0.1] [--out profiles/mesh_bench_C3.json]

Three surfaces on the workload's volume (C3: 512^3): two levels of the CT on channel 3 -- the 10th and the 90th percentile of its
positive values, a skin-like and a bone-like level of the phantom -- in both kernel forms (flavour 0 settles voxels from the range
records, flavour 1 loads every voxel), and the contour that grow_bench.py grows from a picked voxel (contour 0 of volume slot 1, a 0 / 1
mask on a channel without records) at level 0.5, without and with the cap.  For each one JSON line: the medians over K calls behind W
warm-up calls of the wall clock of the counting call alone and of Context.volume_mesh (the counting call, the allocation and the call
that stores), of the storing call's four phases on the device (vr_mesh_timing: pack, counts + scans, vertex emit, triangle emit + copy
back), the counts and the counters, and whether the output equals the first form's.  Then the floor of the host route: the time of a
vr_volume_download of the slot.  A CPU extractor is timed only if one can be imported (skimage.measure.marching_cubes); otherwise the
line says that none was timed.  The lines are also written, as a JSON list, to --out."""
import argparse
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
from volumerendering_amd import host, workloads as wl  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description="Speed of surface extraction (vr_volume_mesh) on a baseline grid: two levels of the CT and a "
                                             "grown contour, both kernel forms, with and without the cap, phase by phase, against a download "
                                             "of the slot.")
    ap.add_argument("--workload", default="C3", choices=sorted(wl.WORKLOADS))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tolerance", type=float, default=0.1, help="half width of the grown value interval (grow_bench.py)")
    ap.add_argument("--vol-n", type=int, default=0, help="volume side instead of the workload's (rehearsals)")
    ap.add_argument("--out", default=None, help="where the lines are written as a JSON list (default profiles/mesh_bench_<workload>.json)")
    args = ap.parse_args()
    n, W, H, vname = wl.WORKLOADS[args.workload]
    n = args.vol_n or n
    if vname not in ("BASIC", "LIGHT"):
        raise SystemExit("mesh_bench: a workload that vr_pick can be asked about (BASIC or LIGHT)")
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    app = host.Application(W, H, 0)
    wl.build_scene(app, args.workload, vol_n=args.vol_n, quiet=True)
    app.OnRender()
    ctx = app.context()
    p = grow_bench.pick_near_centre(app, W, H)
    value = float(p.value[0][3])
    grown = ctx.segment_grow(ctx.grow_whole(0, 1, 0, value - args.tolerance, value + args.tolerance).copy(seeds=[tuple(int(c) for c in p.voxel)]))
    # the host route's floor, and the levels from the values it brings
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        v = ctx.volume_download(0, (n, n, n))
        times.append((time.perf_counter() - t0) * 1e3)
    a = v[..., 3]
    skin, bone = (float(x) for x in np.percentile(a[a > 0], (10, 90)))
    del v, a
    emit(workload=args.workload, volume=n, grown_voxels=int(grown.voxels), skin_level=skin, bone_level=bone)

    cases = [("CT, skin-like level", ctx.mesh_whole(0).copy(level=skin), (0, 1)), ("CT, bone-like level", ctx.mesh_whole(0).copy(level=bone), (0, 1)),
             ("grown contour, open", ctx.mesh_whole(1).copy(channel=0, level=0.5, cap=0), (0,)),
             ("grown contour, capped", ctx.mesh_whole(1).copy(channel=0, level=0.5, cap=1), (0,))]
    for name, d, flavours in cases:
        first = None
        for flavour in flavours:
            ctx.set_kernel_flavour(flavour)
            counting = d.copy(max_vertices=0, max_triangles=0, vertices=None, triangles=None)
            for _ in range(args.warmup):
                out = ctx.volume_mesh(d)
            count_ms, wall, phases = [], [], []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                ctx._chk(ctx.lib.vr_volume_mesh(ctx.h, counting, None))
                count_ms.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                out = ctx.volume_mesh(d)
                wall.append((time.perf_counter() - t0) * 1e3)
                phases.append(ctx.mesh_timing())
            cnt = ctx.mesh_counters()
            first = first or out
            med = [round(statistics.median(ph[i] for ph in phases), 4) for i in range(4)]
            emit(workload=args.workload, surface=name, form="settling" if flavour == 0 else "plain", counting_call_ms=round(statistics.median(count_ms), 3),
                 wall_ms=round(statistics.median(wall), 3), wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3), pack_ms=med[0],
                 count_ms=med[1], vertex_ms=med[2], triangle_ms=med[3], device_ms=round(sum(med), 4), vertices=int(out[2].n_vertices),
                 triangles=int(out[2].n_triangles), inside=int(out[2].inside), cells=int(out[2].cells), points=cnt[0], loaded=cnt[1], settled=cnt[2],
                 mesh_bytes=12 * (int(out[2].n_vertices) + int(out[2].n_triangles)),
                 equals_first_form=bool(np.array_equal(out[0].view(np.uint32), first[0].view(np.uint32)) and np.array_equal(out[1], first[1])))
    ctx.set_kernel_flavour(0)
    try:
        import skimage.measure  # noqa: F401
        cpu = "skimage is importable but was not timed: marching cubes is another surface than this call's tetrahedra"
    except ImportError:
        cpu = "no CPU extractor was timed: skimage is not installed and scipy has none"
    emit(workload=args.workload, case="vr_volume_download of the slot: the floor of the host route", bytes=16 * n ** 3,
         download_ms=round(statistics.median(times[1:]), 1), download_first_ms=round(times[0], 1), cpu_extractor=cpu)
    app.close()
    out_path = args.out or os.path.join(ROOT, "profiles", f"mesh_bench_{args.workload}.json")
    with open(out_path, "w") as fh:
        json.dump(lines, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
