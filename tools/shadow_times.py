#!/usr/bin/env python3
"""What shadows cost a frame on one MI355X.

    python tools/shadow_times.py [--iters 20] [--warmup 3] [--out profiles/shadow_times.txt]

The atrium at 1920x1080 and 3840x2160, single-sampled, one stream, no overlap: frames of geometry pass, shadow pass, opaque pass with device events
around the shadow pass and around the opaque pass (three records per frame; each costs the stream a few microseconds, in both columns alike).  Per
light (a directional one above the hall, a spot under its ceiling), map size S = 1024 / 2048 / 4096 and R = 0 / 1 / 2: the shadow pass's time, and the
opaque pass's with the resolve against the opaque pass of frames without a shadow pass (`off`), so that on - off is k_shadow_resolve.

Bytes the algorithm needs, from the layout as built:
  shadow pass        per caster triangle 168 read (three 56-byte vertices) and 228 written (clip, normal and tangent per vertex, the 80-byte setup record,
                     the info word); 8 S^2 of keys written (every tile of the map is stored)
  k_shadow_resolve   per pixel 8 key bytes read, (2R+1)^2 4-byte gathers from the map, V and m written (8), the RGBA16F image read and written (16);
                     the one-pixel apron is a re-read of lines other workgroups fetch too and is not counted
The time those bytes take at the 5 TB/s a streaming kernel reaches on this part is printed beside the measured time, with the ratio of the two.  The
taps are counted per pixel although neighbouring pixels share most of their texels, so the resolve's byte figure is an upper bound of its traffic: a
ratio under 1 says that the counted bytes cannot all have come from memory, not that bytes bound the kernel.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from awsm_renderer_amd import scenes                                # noqa: E402
from awsm_renderer_amd.hip_backend import HipDevice                 # noqa: E402
from oracle import oracle_lib                                       # noqa: E402
from tests import grid_reference as gr                              # noqa: E402
from tests import helpers                                           # noqa: E402

STREAM_TBS = 5.0
LIGHTS = {
    "directional": dict(eye=(12.0, 34.0, 10.0), target=(0.0, 2.0, 0.0), ortho_half_height=21.0, near=1.0, far=90.0),
    "spot": dict(eye=(1.0, 8.5, 12.0), target=(0.0, 0.0, -4.0), fovy_deg=95.0, near=0.2, far=60.0),
}


def light_of(name, S):
    L = LIGHTS[name]
    block = gr.camera_block(width=S, height=S, **L)
    if name == "spot":
        return block, tuple(L["eye"]) + (1.0,)
    d = np.asarray(L["eye"], np.float64) - np.asarray(L["target"], np.float64)
    return block, tuple(float(v) for v in d / np.linalg.norm(d)) + (0.0,)


def frames(dev, stream, draws, iters, warmup, shadow=None):
    """-> (microseconds per shadow pass, per opaque pass) over `iters` frames"""
    t_shadow = t_opaque = 0.0
    events = []
    for i in range(warmup + iters):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        dev.geometry_pass(draws)
        e[0].record(stream)
        if shadow:
            dev.shadow_pass(shadow[0], draws, **shadow[1])
        e[1].record(stream)
        dev.opaque_pass()
        e[2].record(stream)
        if i >= warmup:
            events.append(e)
    dev.frame_end()
    for e in events:
        t_shadow += e[0].elapsed_time(e[1]); t_opaque += e[1].elapsed_time(e[2])
    return t_shadow * 1000.0 / iters, t_opaque * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lut = oracle_lib.brdf_lut(64, 64)
    lines = [f"# tools/shadow_times.py --iters {a.iters} --warmup {a.warmup} on {torch.cuda.get_device_name(0)}: the atrium, microseconds per pass",
             "# pass = the shadow pass (transform, binning, raster from the light); resolve = opaque pass with it - opaque pass without = k_shadow_resolve<1>",
             "# bytes as tools/shadow_times.py's head states them (the resolve's taps per pixel: an upper bound); at-5-TB/s = the time those bytes alone would take; x = measured / that"]
    for (W, H) in ((1920, 1080), (3840, 2160)):
        sc = scenes.atrium_scene(W, H, detail=0.25, tex_scale=1 / 16)
        model = helpers.build_model(sc)
        stream = torch.cuda.Stream()
        dev, _ = helpers.hip_frame(model, lut, dev=HipDevice(stream=stream.cuda_stream))
        dev.set_stage_timers(False)
        draws = model.collect_draws()
        tris = sum(d["tri_count"] for d in draws)
        _, off = frames(dev, stream, draws, a.iters, a.warmup)
        lines.append(f"{W}x{H}: {tris} caster triangles; opaque pass without shadows {off:8.1f} us")
        for name in LIGHTS:
            for S in (1024, 2048, 4096):
                for R in (0, 1, 2):
                    block, vec = light_of(name, S)
                    t_pass, on = frames(dev, stream, draws, a.iters, a.warmup, (block, dict(map_size=S, pcf_radius=R, light=vec)))
                    V, _ = dev.read_shadow()
                    mb_pass = (tris * 396 + 8 * S * S) / 1e6
                    mb_res = W * H * (8 + 4 * (2 * R + 1) ** 2 + 8 + 16) / 1e6
                    res = on - off
                    lines.append(f"  {name:11s} S = {S:4d} R = {R}: pass {t_pass:7.1f} us ({mb_pass:6.1f} MB, at-5-TB/s {mb_pass / STREAM_TBS:5.1f} us)   "
                                 f"resolve {res:+7.1f} us ({mb_res:6.1f} MB, at-5-TB/s {mb_res / STREAM_TBS:5.1f} us: x {res / (mb_res / STREAM_TBS):4.2f})   "
                                 f"(V < 1 on {100 * float((V < 1.0).mean()):.1f} % of the frame)")
        dev.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
