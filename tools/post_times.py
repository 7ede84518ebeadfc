#!/usr/bin/env python3
"""Times of the effects + display passes (awsm_hip_post_pass) on one MI355X, per configuration, after a warm-up.

    python tools/post_times.py [--iters 50] [--warmup 10] [--out profiles/post_times.txt]

sync:    the context runs on the caller's stream; device events around `iters` post passes of one rendered frame -> us per post pass.
overlap: AWSM_CFG_OVERLAP_FRAMES; `iters` whole frames (geometry + opaque [+ post]) enqueued back to back with frame_flush, device-synchronised at
         the end; the frame time with the post pass minus the frame time without it.
Scenes: the 4K atrium and the 1080p helmet.  Bytes moved by display-only: 8 B read + 4 B written per pixel.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from awsm_renderer_amd import scenes                                # noqa: E402
from awsm_renderer_amd.hip_backend import HipDevice                 # noqa: E402
from oracle import oracle_lib                                       # noqa: E402
from tests import helpers                                           # noqa: E402

CONFIGS = [("display only", {}), ("smaa", dict(smaa=True)), ("bloom", dict(bloom=True)), ("dof", dict(dof=True)),
           ("smaa+bloom+dof", dict(smaa=True, bloom=True, dof=True))]


def setup(dev, sc, model, lut):
    dev.resize(sc.width, sc.height, 0)
    dev.upload_mirrors(model.mirrors())
    dev.buffer_write(5, 496, np.array((10.0, 5.6), dtype=np.float32))     # the reference's DoF defaults
    for i, t in enumerate(model.texture_arrays()):
        dev.texture_array_upload(i, t["texels"])
    for i, s in enumerate(sc.samplers):
        dev.sampler_set(i, s)
    dev.env_upload(sc.skybox_rgba, sc.prefiltered_rgb, sc.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(lut))
    dev.set_stage_timers(False)


def time_sync(sc, model, lut, iters, warmup):
    stream = torch.cuda.Stream()
    dev = HipDevice(stream=stream.cuda_stream)
    setup(dev, sc, model, lut)
    dev.geometry_pass(model.collect_draws())
    dev.opaque_pass()
    dev.frame_end()
    out = {}
    for name, kw in CONFIGS:
        for _ in range(warmup):
            dev.post_pass(1, **kw)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(iters):
            dev.post_pass(1, **kw)
        b.record(stream)
        b.synchronize()
        out[name] = a.elapsed_time(b) * 1000.0 / iters
    dev.close()
    return out


def time_overlap(sc, model, lut, iters, warmup):
    dev = HipDevice(overlap_frames=True)
    setup(dev, sc, model, lut)
    draws = model.collect_draws()

    def frames(kw):
        for k in range(warmup + iters):
            if k == warmup:
                dev.frame_end()
                t0 = time.perf_counter()
            dev.geometry_pass(draws)
            dev.opaque_pass()
            if kw is not None:
                dev.post_pass(1, **kw)
            dev.frame_flush()
        dev.frame_end()
        return (time.perf_counter() - t0) * 1e6 / iters

    base = frames(None)
    out = {"frame without post": base}
    for name, kw in CONFIGS:
        out[name] = frames(kw) - base
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lut = oracle_lib.brdf_lut(64, 64)
    lines = [f"# tools/post_times.py --iters {a.iters} --warmup {a.warmup} on {torch.cuda.get_device_name(0)}: microseconds"]
    for label, sc in (("atrium 3840x2160", scenes.atrium_scene(3840, 2160, detail=0.25, tex_scale=1 / 16)),
                      ("helmet 1920x1080", scenes.helmet_scene(1920, 1080, tex_size=256))):
        model = helpers.build_model(sc)
        s = time_sync(sc, model, lut, a.iters, a.warmup)
        o = time_overlap(sc, model, lut, a.iters, a.warmup)
        mb = sc.width * sc.height * 12 / 1e6
        lines.append(f"{label}: display only moves {mb:.1f} MB = {mb / s['display only']:.2f} TB/s")
        for name, _ in CONFIGS:
            lines.append(f"  {name:16s} sync {s[name]:8.1f} us/post pass ({s[name] / s['display only']:.2f} x display only)   overlap +{o[name]:8.1f} us/frame")
        lines.append(f"  overlapped frame without the post pass: {o['frame without post']:.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
