#!/usr/bin/env python3
"""Speed of the intensity projections (VR_VARIANT_MIP / MINIP / AVERAGE, csrc/vr_proj.h) on a BASELINE configuration.

    python tools/projection_bench.py --workload C3 [--steps 40] [--warmup 10]

The scene is workloads.build_scene's (its volume, preparation, tables and stepping), viewed on bench.py's turntable (the camera
rotated by Camera::Rotate(2 px, 0) per frame).  For each mode one JSON line: ms per frame one frame at a time and with four
frames in flight (four streams of the context, four output buffers), Gsamples/s of composited samples, fetched / composited,
the same with flavour 1 (no skipping: what skipping buys), and the scene's own shader (LIGHT for C3 / C5) on the same context
for scale.  Wall clock around K frames behind W warm-up frames, one synchronisation at the end."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from volumerendering_amd import capi, host, workloads as wl  # noqa: E402

TURN_PX = 2.0  # bench.py's turntable step (Camera::Rotate(2 px, 0) per frame)


def turntable(app, n):
    cam = app.camera()
    us = []
    for _ in range(n):
        app.OnUpdate()
        us.append(capi.Uniforms.from_buffer_copy(bytes(app.uniforms())))
        cam.Rotate(TURN_PX, 0.0)
    cam.SetOrbit(*wl.CAMERA)
    app.OnUpdate()
    return us


def leg(ctx, variant, us, outs, streams, warmup, steps):
    """(ms per frame, composited per frame, fetched per frame): frames go round-robin over `streams` into `outs`."""
    def run(g0, k):
        for g in range(g0, g0 + k):
            ctx.set_uniforms(us[g % len(us)])
            ctx.render_async(variant, outs[g % len(outs)], streams[g % len(streams)])
        ctx.counters()  # (waits for the last launch)
    run(0, warmup)
    t0 = time.perf_counter()
    run(warmup, steps)
    for i in range(len(streams)):  # every stream's last frame has finished: one more synchronous frame on each
        ctx.render_async(variant, outs[i % len(outs)], streams[i])
        ctx.counters()
    ms = (time.perf_counter() - t0) * 1e3 / (steps + len(streams))
    comp = fetched = 0
    for g in range(steps):
        ctx.set_uniforms(us[(warmup + g) % len(us)])
        ctx.render(variant)
        c, _, f = ctx.counters()
        comp += c
        fetched += f
    return ms, comp / steps, fetched / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", default="C3", choices=sorted(wl.WORKLOADS))
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    n, W, H, vname = wl.WORKLOADS[args.workload]
    app = host.Application(W, H, 0)
    scene_variant, vols = wl.build_scene(app, args.workload, quiet=True)
    ctx = app.context()
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
        return dict(ms_one=round(ms1, 4), ms_in_flight4=round(ms4, 4), gsamples_s=round(comp / ms1 * 1e-6, 2),
                    fetched_over_composited=round(fetched / comp, 4) if comp else None, flavour=ctx.last_kernel_flavour())

    scale = measure(scene_variant, 0)
    for variant in (capi.MIP, capi.MINIP, capi.AVERAGE):
        skip = measure(variant, 0)
        plain = measure(variant, 1)
        print(json.dumps(dict(workload=args.workload, mode=capi.VARIANT_NAMES[variant], **skip, no_skip=plain,
                              skipping_speedup=round(plain["ms_one"] / skip["ms_one"], 3),
                              scene_shader=dict(variant=capi.VARIANT_NAMES[scene_variant], **scale))), flush=True)
    ctx.set_kernel_flavour(0)
    for o in others:
        o.close()
    app.close()


if __name__ == "__main__":
    main()
