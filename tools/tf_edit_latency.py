#!/usr/bin/env python3
"""What a transfer-function drag costs per frame.

    python3 tools/tf_edit_latency.py [--workload C3] [--frames 120] [--warm 16]

Builds the workload (volumerendering_amd/workloads.py) on bench.py's turntable cameras and prints one JSON line with the wall
time per frame of four loops, each one frame at a time on one stream and again with four frames in flight on vr_stream(0..3):
  (a) no edits;
  (b) a synchronous opacity edit (vr_tf_upload_opacity, drains the device) before every frame;
  (c) an asynchronous one (vr_tf_upload_opacity_async on the frame's stream);
  (d) an asynchronous edit that keeps the zero prefix (the texels above it scaled): no distance-field rebuild, no frame without
      the active-brick box -- what (c) costs beyond (d) is the rebuild and the unbounded-box frames together.
The edit is the reference's drag (OpacityTF::UpdateYAxis): the first non-zero opacity texel moves by one texel per frame, so every
edit moves the table's zero prefix (and rebuilds the empty-space distance field).  Also printed: the frames of (c) that ran without
the active-brick box because the rebuilt field's box had not reached the host yet.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--warm", type=int, default=16)
    args = ap.parse_args()

    import numpy as np
    import torch
    from volumerendering_amd import host, workloads as wl

    n, W, H, vname = wl.WORKLOADS[args.workload]
    app = host.Application(W, H, 0)
    variant, vols = wl.build_scene(app, args.workload, "default", "exact0", quiet=True)
    ctx = app.context()
    total = args.warm + args.frames
    cam = app.camera()
    us = []
    for g in range(total):  # bench.py's turntable: Camera::Rotate(2 px, 0) per frame
        app.OnUpdate()
        us.append(app.uniforms())
        cam.Rotate(2.0, 0.0)
    base = np.ascontiguousarray(app.scene_opacity_tf(0).table(), dtype=np.float32)
    first = int(np.argmax(base > 0.0))  # the first non-zero texel
    tables = []
    for g in range(total):  # the drag: that texel moves one up per frame, and back
        t = base.copy()
        t[:first + 1 + (g % 32)] = 0.0
        tables.append(t)
    keep = []
    for g in range(total):  # (d): the same zero prefix, the texels above it moved
        t = base.copy()
        t[first:] *= np.float32(1.0 - 0.002 * (g % 32))
        keep.append(t)
    R = base.size
    frames = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    streams = [ctx.stream(i) for i in range(4)]
    torch.cuda.synchronize()

    def loop(mode, flight):
        ctx.hint_frames_in_flight(flight)
        ctx.tf_upload(0, base, app.scene_color_tf(0).table())
        miss0 = 0
        t0 = 0.0
        for g in range(total):
            if g == args.warm:
                torch.cuda.synchronize()
                ctx.resize(W, H)  # (drains the device)
                miss0 = ctx.unbounded_box_launches()
                t0 = time.perf_counter()
            s = streams[g % flight]
            if mode == "sync":
                ctx._chk(ctx.lib.vr_tf_upload_opacity(ctx.h, 0, tables[g].ctypes.data, R))
            elif mode == "async":
                ctx.tf_upload_async(0, opacity=tables[g], stream=s)
            elif mode == "async_keep":
                ctx.tf_upload_async(0, opacity=keep[g], stream=s)
            ctx.set_uniforms(us[g])
            ctx.render_async(variant, frames[g % flight].data_ptr(), s)
        torch.cuda.synchronize()
        ctx.resize(W, H)
        ms = (time.perf_counter() - t0) * 1e3 / args.frames
        return ms, ctx.unbounded_box_launches() - miss0

    out = {"workload": args.workload, "frames": args.frames, "table_resolution": R}
    for flight in (1, 4):
        for tag, mode in (("a_no_edit", "none"), ("b_sync_edit", "sync"), ("c_async_edit", "async"),
                          ("d_async_keep_prefix", "async_keep")):
            ms, miss = loop(mode, flight)
            out[f"{tag}_ms_{flight}x"] = round(ms, 4)
            if mode.startswith("async"):
                out[f"{tag[0]}_unbounded_box_frames_{flight}x"] = int(miss)
    ctx.tf_upload(0, base, app.scene_color_tf(0).table())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
