#!/usr/bin/env python3
"""What shadows from several views cost a frame on one MI355X.

    python tools/shadow_views_times.py [--iters 20] [--warmup 3] [--out profiles/shadow_views_times.txt]

The scene and the method of tools/shadow_times.py: the atrium at a quarter tessellation, 1920x1080 and 3840x2160, single-sampled, one stream, no
overlap, device events around the shadow pass and around the opaque pass; resolve = the opaque pass with the pass in front of it - the opaque pass of
frames without one.  S = 2048, R = 1.  Configurations:
  one view through awsm_hip_shadow_pass (k_shadow_resolve) and through awsm_hip_shadow_pass_views (k_shadow_resolve_views), twice each in turn: the
  second pair gives the run-to-run spread the one-view comparison is to be read against;
  2 and 4 nested windows of the directional light, tightest first (halves of the full window's half height);
  the six faces of a point light under the ceiling (the spot's position).
Every view is handed every draw (no culling by the view's frustum: the host layer's job), so the pass columns are upper bounds.

Bytes, as tools/shadow_times.py counts them: per view 396 bytes per caster triangle and 8 S^2 of keys; the resolve per pixel 8 key bytes, 9 4-byte
gathers, V and m (8), the view byte (1, the new kernel only) and the RGBA16F image read and written (16).  The time those bytes take at 5 TB/s is
printed beside the measured time.
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
from tests import shadow_views_reference as svr                     # noqa: E402

STREAM_TBS = 5.0
S, R = 2048, 1
SUN = dict(eye=(12.0, 34.0, 10.0), target=(0.0, 2.0, 0.0), ortho_half_height=21.0, near=1.0, far=90.0)
LAMP = (1.0, 8.5, 12.0)


def sun_blocks(n):
    """n nested windows, tightest first: half heights 21 / 2^(n-1) ... 21."""
    return [gr.camera_block(width=S, height=S, **dict(SUN, ortho_half_height=SUN["ortho_half_height"] / 2 ** k)) for k in range(n - 1, -1, -1)]


def sun_vec():
    d = np.asarray(SUN["eye"], np.float64) - np.asarray(SUN["target"], np.float64)
    return tuple(float(v) for v in d / np.linalg.norm(d)) + (0.0,)


def frames(dev, stream, draws, iters, warmup, shadow=None):
    """shadow: None, ("old", block, params) or ("views", blocks, params) -> (microseconds per shadow pass, per opaque pass)"""
    t_shadow = t_opaque = 0.0
    events = []
    for i in range(warmup + iters):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        dev.geometry_pass(draws)
        e[0].record(stream)
        if shadow and shadow[0] == "old":
            dev.shadow_pass(shadow[1], draws, **shadow[2])
        elif shadow:
            dev.shadow_pass_views([(b, draws) for b in shadow[1]], **shadow[2])
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
    lines = [f"# tools/shadow_views_times.py --iters {a.iters} --warmup {a.warmup} on {torch.cuda.get_device_name(0)}: the atrium, S = {S}, R = {R}, microseconds per pass",
             "# pass = every view's transform, binning and raster; resolve = opaque pass with it - opaque pass without; bytes as the tool's head states them; x = measured / at-5-TB/s"]
    sun = dict(map_size=S, pcf_radius=R, light=sun_vec())
    lamp = dict(map_size=S, pcf_radius=R, light=svr.point_light(LAMP))
    one = sun_blocks(1)
    configs = [("1 view, shadow_pass", ("old", one[0], sun), 1), ("1 view, shadow_pass_views", ("views", one, sun), 1),
               ("1 view, shadow_pass (again)", ("old", one[0], sun), 1), ("1 view, shadow_pass_views (again)", ("views", one, sun), 1),
               ("2 cascades", ("views", sun_blocks(2), sun), 2), ("4 cascades", ("views", sun_blocks(4), sun), 4),
               ("point light, 6 faces", ("views", svr.cube_face_blocks(LAMP, S, R, near=0.2, far=60.0), lamp), 6)]
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
        for name, shadow, k in configs:
            t_pass, on = frames(dev, stream, draws, a.iters, a.warmup, shadow)
            V, _ = dev.read_shadow()
            none = float((dev.read_shadow_view() == 255).mean()) if shadow[0] == "views" else float("nan")
            mb_pass = k * (tris * 396 + 8 * S * S) / 1e6
            mb_res = W * H * (8 + 4 * (2 * R + 1) ** 2 + 8 + (1 if shadow[0] == "views" else 0) + 16) / 1e6
            res = on - off
            lines.append(f"  {name:34s}: pass {t_pass:7.1f} us ({mb_pass:6.1f} MB, at-5-TB/s {mb_pass / STREAM_TBS:5.1f} us)   "
                         f"resolve {res:+7.1f} us ({mb_res:6.1f} MB, at-5-TB/s {mb_res / STREAM_TBS:5.1f} us: x {res / (mb_res / STREAM_TBS):4.2f})   "
                         f"(V < 1 on {100 * float((V < 1.0).mean()):.1f} %, no view on {100 * none:.1f} % of the frame)")
        dev.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
