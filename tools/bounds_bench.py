#!/usr/bin/env python3
"""Speed of the per-pixel ray bounds (vr_set_ray_bounds, csrc/vr_bound.h) on a BASELINE configuration.

    python tools/bounds_bench.py --workload C3 [--iso 0.3] [--steps 40] [--warmup 10]

The scene is workloads.build_scene's (its volume, preparation, tables and stepping), viewed on bench.py's turntable (projection_bench's
turntable).  LIGHT, one frame at a time and with four frames in flight, for (a) the unbounded frame, whatever flavour the default
picks, (b) flavours 27 and 28 with the trivial bounds near = 0, far = 1, (c) far = the depth of the same view's ISO surface frame at
level --iso (one depth buffer per turntable view, computed on the device before anything is timed: ISO surface frame ->
vr_surface_depth_async), (d) near = that depth.  One JSON line with ms, composited, fetched and the flavour that ran.  Flavours 27 / 28
are one-lane kernels: on whole unbounded frames they are expected to be slower than the two-steps-ahead kernel the default picks.
Wall clock around K frames behind W warm-up frames, one synchronisation at the end."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from projection_bench import turntable  # noqa: E402
from volumerendering_amd import capi, host, workloads as wl  # noqa: E402


def leg(ctx, us, bounds, outs, streams, warmup, steps):
    """(ms per frame, composited per frame, fetched per frame) of LIGHT: frame g with uniforms us[g] between bounds[g] = (near, far)
    device pointers, round-robin over `streams` into `outs`."""
    def frame(g, out, stream):
        ctx.set_uniforms(us[g % len(us)])
        ctx.set_ray_bounds(*bounds[g % len(bounds)])
        ctx.render_async(capi.LIGHT, out, stream)

    def run(g0, k):
        for g in range(g0, g0 + k):
            frame(g, outs[g % len(outs)], streams[g % len(streams)])
        ctx.counters()  # (waits for the last launch)
    run(0, warmup)
    t0 = time.perf_counter()
    run(warmup, steps)
    for i in range(len(streams)):  # every stream's last frame has finished: one more synchronous frame on each
        frame(warmup + steps + i, outs[i % len(outs)], streams[i])
        ctx.counters()
    ms = (time.perf_counter() - t0) * 1e3 / (steps + len(streams))
    comp = fetched = 0
    for g in range(warmup, warmup + steps):
        frame(g, outs[0], streams[0])
        c, _, f = ctx.counters()
        comp += c
        fetched += f
    return ms, comp / steps, fetched / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", default="C3", choices=sorted(wl.WORKLOADS))
    ap.add_argument("--iso", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    n, W, H, vname = wl.WORKLOADS[args.workload]
    app = host.Application(W, H, 0)
    wl.build_scene(app, args.workload, quiet=True)
    ctx = app.context()
    n_views = args.warmup + args.steps + 8
    us = turntable(app, n_views)
    others = [capi.Context(W, H, 0) for _ in range(4)]
    outs = [o.frame_device_ptr() for o in others]
    s1, s4 = [ctx.stream(0)], [ctx.stream(i) for i in range(4)]

    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))

    def device_floats(values=None):
        p = C.c_void_p()
        if hip.hipMalloc(C.byref(p), C.c_size_t(W * H * 4)) != 0:
            raise RuntimeError("hipMalloc failed")
        if values is not None:
            a = np.ascontiguousarray(values, dtype=np.float32)
            if hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) != 0:  # hipMemcpyHostToDevice
                raise RuntimeError("hipMemcpy failed")
        return p

    zero, one = device_floats(np.zeros(W * H)), device_floats(np.ones(W * H))
    # the ISO surface's depth of every view
    ctx.set_iso_value(args.iso)
    ctx.set_output(capi.OUTPUT_SURFACE)
    depth, iso_hits = [], 0
    for u in us:
        d = device_floats()
        ctx.set_uniforms(u)
        ctx.render(capi.ISO)
        iso_hits = ctx.counters()[1]
        ctx.surface_depth(ctx.frame_device_ptr(), d.value)
        depth.append(d)
    ctx.counters()
    ctx.set_output(capi.OUTPUT_COLOR)

    def measure(bounds, flavour):
        ctx.set_kernel_flavour(flavour)
        ctx.hint_frames_in_flight(1)
        ms1, comp, fetched = leg(ctx, us, bounds, outs[:1], s1, args.warmup, args.steps)
        ctx.hint_frames_in_flight(4)
        ms4, _, _ = leg(ctx, us, bounds, outs, s4, args.warmup, args.steps)
        ctx.hint_frames_in_flight(1)
        return dict(ms_one=round(ms1, 4), ms_in_flight4=round(ms4, 4), composited=round(comp), fetched=round(fetched),
                    flavour=ctx.last_kernel_flavour())

    rows = dict(unbounded=measure([(None, None)], 0),
                trivial_27=measure([(zero.value, one.value)], 0),
                trivial_28=measure([(zero.value, one.value)], 1),
                far_iso_27=measure([(None, d.value) for d in depth], 0),
                far_iso_28=measure([(None, d.value) for d in depth], 1),
                near_iso_27=measure([(d.value, None) for d in depth], 0),
                near_iso_28=measure([(d.value, None) for d in depth], 1))
    print(json.dumps(dict(workload=args.workload, iso=args.iso, iso_hits=int(iso_hits), **rows)), flush=True)
    ctx.set_kernel_flavour(0)
    ctx.set_ray_bounds(None, None)
    for p in [zero, one] + depth:
        hip.hipFree(p)
    for o in others:
        o.close()
    app.close()


if __name__ == "__main__":
    main()
