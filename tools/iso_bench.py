#!/usr/bin/env python3
"""Speed of the shaded isosurface (VR_VARIANT_ISO, csrc/vr_iso.h) on a BASELINE configuration.

    python tools/iso_bench.py --workload C3 [--iso 0.3] [--steps 40] [--warmup 10]

The scene is workloads.build_scene's (its volume, preparation, tables and stepping), viewed on bench.py's turntable (projection_bench's
turntable / leg helpers).  One JSON line: ms per frame one frame at a time and with four frames in flight for flavour 21 (exact
skipping) and flavour 22 (none), the skipping speed-up, fetched / composited, the covered pixels (so that the level is known to hit
tissue), and the scene's own shader (LIGHT for C3 / C5) on the same context for scale.  Wall clock around K frames behind W warm-up
frames, one synchronisation at the end."""
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
    ap.add_argument("--iso", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    n, W, H, vname = wl.WORKLOADS[args.workload]
    app = host.Application(W, H, 0)
    scene_variant, vols = wl.build_scene(app, args.workload, quiet=True)
    ctx = app.context()
    ctx.set_iso_value(args.iso)
    us = turntable(app, args.warmup + args.steps + 8)
    others = [capi.Context(W, H, 0) for _ in range(4)]
    outs = [o.frame_device_ptr() for o in others]
    s1, s4 = [ctx.stream(0)], [ctx.stream(i) for i in range(4)]

    def measure(variant, flavour):
        ctx.set_kernel_flavour(flavour)
        ctx.hint_frames_in_flight(1)
        ms1, comp, fetched = leg(ctx, variant, us, outs[:1], s1, args.warmup, args.steps)
        ctx.hint_frames_in_flight(4)
        ms4, _, _ = leg(ctx, variant, us, outs, s4, args.warmup, args.steps)
        ctx.hint_frames_in_flight(1)
        ctx.set_uniforms(us[0])
        ctx.render(variant)
        covered = ctx.counters()[1]
        return dict(ms_one=round(ms1, 4), ms_in_flight4=round(ms4, 4), gsamples_s=round(comp / ms1 * 1e-6, 2),
                    fetched_over_composited=round(fetched / comp, 4) if comp else None, covered_px=int(covered),
                    flavour=ctx.last_kernel_flavour())

    scale = measure(scene_variant, 0)
    skip = measure(capi.ISO, 0)
    plain = measure(capi.ISO, 1)
    print(json.dumps(dict(workload=args.workload, iso=args.iso, **skip, no_skip=plain,
                          skipping_speedup=round(plain["ms_one"] / skip["ms_one"], 3),
                          skipping_speedup_in_flight4=round(plain["ms_in_flight4"] / skip["ms_in_flight4"], 3),
                          scene_shader=dict(variant=capi.VARIANT_NAMES[scene_variant], **scale))), flush=True)
    ctx.set_kernel_flavour(0)
    for o in others:
        o.close()
    app.close()


if __name__ == "__main__":
    main()
