#!/usr/bin/env python3
"""Speed of the lit shader's shadows (vr_set_shadows, csrc/vr_shadow.h) on a BASELINE configuration.

    python tools/shadow_bench.py --workload C3 [--divisor 4] [--scale 1.0] [--steps 40] [--warmup 10]

The scene is workloads.build_scene's (its volume, preparation, tables and stepping), viewed on bench.py's turntable (projection_bench's
turntable / leg helpers; the light stays where the scene puts it, so the turntable's frames share one light volume).  One JSON line:
ms per frame one frame at a time and with four frames in flight for flavour 23 (exact skipping), flavour 24 (none) and unshadowed
LIGHT on the same context, fetched / composited of 23 and 24, and the light volume's build time at divisors 2, 4 and 8 with and
without skipping.  A build is timed by the render's own device events: vr_last_timing's total (which contains the build) less its
kernel time, less the same difference of a render that builds nothing; the least of three builds (each a new opacity scale: a key
that neither form has built before)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from projection_bench import leg, turntable  # noqa: E402
from volumerendering_amd import capi, host, workloads as wl  # noqa: E402


def build_ms(ctx, u, divisor, scale, flavour):
    """Least of three builds of the light volume at `divisor` (ms), from the events of synchronous renders (see the module's doc)."""
    ctx.set_kernel_flavour(flavour)
    ctx.set_uniforms(u)
    best = None
    for k in range(3):
        ctx.set_shadows(divisor, scale * (1.0 + 1e-3 * (k + 1) + 1e-2 * flavour))  # (a key no earlier build of either form had)
        ctx.render(capi.LIGHT)
        k1, t1 = ctx.last_timing()
        ctx.render(capi.LIGHT)
        k2, t2 = ctx.last_timing()
        ms = (t1 - k1) - (t2 - k2)
        best = ms if best is None else min(best, ms)
    return round(best, 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", default="C3", choices=sorted(wl.WORKLOADS))
    ap.add_argument("--divisor", type=int, default=4)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    n, W, H, vname = wl.WORKLOADS[args.workload]
    app = host.Application(W, H, 0)
    scene_variant, vols = wl.build_scene(app, args.workload, quiet=True)
    if scene_variant != capi.LIGHT:
        raise SystemExit(f"{args.workload} is not a lit scene")
    ctx = app.context()
    us = turntable(app, args.warmup + args.steps + 8)
    others = [capi.Context(W, H, 0) for _ in range(4)]
    outs = [o.frame_device_ptr() for o in others]
    s1, s4 = [ctx.stream(0)], [ctx.stream(i) for i in range(4)]

    def measure(divisor, flavour):
        ctx.set_shadows(divisor, args.scale)
        ctx.set_kernel_flavour(flavour)
        ctx.hint_frames_in_flight(1)
        ms1, comp, fetched = leg(ctx, capi.LIGHT, us, outs[:1], s1, args.warmup, args.steps)
        ctx.hint_frames_in_flight(4)
        ms4, _, _ = leg(ctx, capi.LIGHT, us, outs, s4, args.warmup, args.steps)
        ctx.hint_frames_in_flight(1)
        ctx.set_uniforms(us[0])
        ctx.render(capi.LIGHT)
        return dict(ms_one=round(ms1, 4), ms_in_flight4=round(ms4, 4), gsamples_s=round(comp / ms1 * 1e-6, 2),
                    fetched_over_composited=round(fetched / comp, 4) if comp else None, flavour=ctx.last_kernel_flavour())

    light = measure(0, 0)
    skip = measure(args.divisor, 0)
    plain = measure(args.divisor, 1)
    builds = {str(d): dict(skip=build_ms(ctx, us[0], d, args.scale, 0), no_skip=build_ms(ctx, us[0], d, args.scale, 1)) for d in (2, 4, 8)}
    print(json.dumps(dict(workload=args.workload, divisor=args.divisor, scale=args.scale, **skip, no_skip=plain,
                          skipping_speedup=round(plain["ms_one"] / skip["ms_one"], 3),
                          skipping_speedup_in_flight4=round(plain["ms_in_flight4"] / skip["ms_in_flight4"], 3),
                          unshadowed_light=light, build_ms=builds)), flush=True)
    ctx.set_shadows(0)
    ctx.set_kernel_flavour(0)
    for o in others:
        o.close()
    app.close()


if __name__ == "__main__":
    main()
