#!/usr/bin/env python3
"""Speed of the surface-position output (vr_set_output(VR_OUTPUT_SURFACE), csrc/vr_surf.h) on a BASELINE configuration.

    python tools/surface_bench.py --workload C3 [--thresholds 0.5 0.95] [--steps 40] [--warmup 10]

The scene is workloads.build_scene's (its volume, preparation, tables and stepping), viewed on bench.py's turntable (projection_bench's
turntable / leg helpers).  One JSON line: per threshold, ms per frame one frame at a time and with four frames in flight for flavour
25 (exact skipping) and flavour 26 (none), the skipping speed-up, fetched / composited and the hits (pixels whose alpha passed the
threshold), beside the same scene's LIGHT colour frame measured in the same run on the same context.  Wall clock around K frames
behind W warm-up frames, one synchronisation at the end."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from projection_bench import leg, turntable  # noqa: E402
from volumerendering_amd import capi, host, workloads as wl  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", default="C3", choices=sorted(wl.WORKLOADS))
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.5, 0.95])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    n, W, H, vname = wl.WORKLOADS[args.workload]
    app = host.Application(W, H, 0)
    wl.build_scene(app, args.workload, quiet=True)
    ctx = app.context()
    us = turntable(app, args.warmup + args.steps + 8)
    others = [capi.Context(W, H, 0) for _ in range(4)]
    outs = [o.frame_device_ptr() for o in others]
    s1, s4 = [ctx.stream(0)], [ctx.stream(i) for i in range(4)]

    def measure(output, flavour):
        ctx.set_output(output)
        ctx.set_kernel_flavour(flavour)
        ctx.hint_frames_in_flight(1)
        ms1, comp, fetched = leg(ctx, capi.LIGHT, us, outs[:1], s1, args.warmup, args.steps)
        ctx.hint_frames_in_flight(4)
        ms4, _, _ = leg(ctx, capi.LIGHT, us, outs, s4, args.warmup, args.steps)
        ctx.hint_frames_in_flight(1)
        ctx.set_uniforms(us[0])
        ctx.render(capi.LIGHT)
        covered = ctx.counters()[1]
        ctx.set_output(capi.OUTPUT_COLOR)
        return dict(ms_one=round(ms1, 4), ms_in_flight4=round(ms4, 4), gsamples_s=round(comp / ms1 * 1e-6, 2),
                    fetched_over_composited=round(fetched / comp, 4) if comp else None,
                    **({"hits": int(covered)} if output == capi.OUTPUT_SURFACE else {"covered_px": int(covered)}),
                    flavour=ctx.last_kernel_flavour())

    colour = measure(capi.OUTPUT_COLOR, 0)
    rows = []
    for tau in args.thresholds:
        ctx.set_surface_threshold(tau)
        skip = measure(capi.OUTPUT_SURFACE, 0)
        plain = measure(capi.OUTPUT_SURFACE, 1)
        rows.append(dict(threshold=tau, **skip, no_skip=plain,
                         skipping_speedup=round(plain["ms_one"] / skip["ms_one"], 3),
                         skipping_speedup_in_flight4=round(plain["ms_in_flight4"] / skip["ms_in_flight4"], 3),
                         over_light_colour=round(skip["ms_one"] / colour["ms_one"], 3),
                         over_light_colour_in_flight4=round(skip["ms_in_flight4"] / colour["ms_in_flight4"], 3)))
    print(json.dumps(dict(workload=args.workload, surface=rows, light_colour=colour)), flush=True)
    ctx.set_kernel_flavour(0)
    for o in others:
        o.close()
    app.close()


if __name__ == "__main__":
    main()
