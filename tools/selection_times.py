#!/usr/bin/env python3
"""What the editor's selection overlay costs the world transparent pass on one MI355X.

    python tools/selection_times.py [--iters 200] [--warmup 20] [--detail 1.0] [--out profiles/selection_times.txt]

The bench frame's geometry (the atrium at 3840x2160, detail 1.0; small textures: no kernel timed here samples one) with its keys and opaque image
resident, single-sampled and MSAA x4.  awsm_hip_transparent_pass with n_draws = 0 — two small fills, k_bin_scan, k_forward_cover over empty tiles,
k_forward_blend<S> — `iters` times back to back on one stream between two device events, synchronised at the end: with the selection off, and on
with the 1, 8 and 64 meshes of most triangles selected (as many keys as boxes), the ring at R = 2 and R = 4.  Off and on alternate and the whole
round is run twice; the second round is reported.  Everything but the three selection kernels is the same work in both, so on - off =
k_selection_mark + k_selection_edges + k_selection_overlay<S>, provided the device bounds both runs: the host's time to enqueue a pass is measured
in the same loop, before the synchronisation, and a row whose off run was not clearly device-bound says so.

Bytes the overlay kernel needs per pixel: 8 S key bytes and 4 bytes of tri_info per hit sample are read by every tile (the staged apron re-reads
lines other workgroups fetch too and is not counted); the composite's 8 bytes are read and written on ring and box pixels only.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from awsm_renderer_amd import scenes                                # noqa: E402
from awsm_renderer_amd.hip_backend import HipDevice                 # noqa: E402
from oracle import oracle_lib                                       # noqa: E402
from oracle.host_mirror import key_as_ffi                           # noqa: E402
from tests import helpers                                           # noqa: E402

W, H = 3840, 2160
STREAM_TBS = 5.0


def time_passes(sc, model, lut, msaa, picks, iters, warmup):
    """picks: [(label, set_selection arguments or None for off)] -> {label: (device us per pass, host us per pass)}, {label: (ring px, box px)}"""
    stream = torch.cuda.Stream()
    dev = HipDevice(stream=stream.cuda_stream)
    dev.resize(sc.width, sc.height, msaa)
    dev.upload_mirrors(model.mirrors())
    for i, t in enumerate(model.texture_arrays()):
        dev.texture_array_upload(i, t["texels"])
    for i, s in enumerate(sc.samplers):
        dev.sampler_set(i, s)
    dev.env_upload(sc.skybox_rgba, sc.prefiltered_rgb, sc.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(lut))
    dev.set_stage_timers(False)
    dev.geometry_pass(model.collect_draws())
    dev.opaque_pass()
    dev.transparent_pass([])
    dev.frame_end()                                     # the pass's lists are sized now
    out, shown = {}, {}
    for _ in range(2):                                  # twice: the second round is what is reported
        for label, args in picks:
            if args is None:
                dev.set_selection(on=None)
            else:
                dev.set_selection(**args)
            for _ in range(warmup):
                dev.transparent_pass([])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            t0 = time.perf_counter()
            for _ in range(iters):
                dev.transparent_pass([])
            host = (time.perf_counter() - t0) * 1e6 / iters      # before the synchronisation: the enqueue calls alone
            b.record(stream)
            b.synchronize()
            out[label] = (a.elapsed_time(b) * 1000.0 / iters, host)
            if args is not None and label not in shown:
                _, ring, alpha, _ = dev.read_selection()
                shown[label] = (int(ring.sum()), int((alpha > 0).sum()))
    dev.close()
    return out, shown


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lut = oracle_lib.brdf_lut(64, 64)
    sc = scenes.atrium_scene(W, H, detail=a.detail, tex_scale=1 / 16)
    model = helpers.build_model(sc)
    draws = sorted(model.collect_draws(), key=lambda d: -d["tri_count"])
    meshes = [(d["mesh_key"], model.meshes.get(d["mesh_key"])) for d in draws[:64]]
    picks = [("off", None)]
    for n in (1, 8, 64):
        for R in (2, 4):
            chosen = meshes[:n]
            picks.append(("%2d boxes R=%d" % (len(chosen), R), dict(mesh_keys=[key_as_ffi(k) for k, _ in chosen], outline_radius=R,
                                                                   boxes=[list(r.world_aabb.min) + list(r.world_aabb.max) for _, r in chosen])))
            picks.append(("off", None))
    lines = [f"# tools/selection_times.py --iters {a.iters} --warmup {a.warmup} --detail {a.detail} on {torch.cuda.get_device_name(0)}: the atrium at {W}x{H}"
             f" ({sum(d['tri_count'] for d in draws)} triangles in {len(draws)} draws), microseconds per world transparent pass with n_draws = 0",
             "# selection = on - off (the off run taken just before it) = k_selection_mark + k_selection_edges + k_selection_overlay<S>; keys = 8 S bytes per pixel,",
             "# at-5-TB/s = the time the keys alone would take; host = the host's time to enqueue one pass; an off run whose host time is not under 80 % of",
             "# its device time waited for the host, and selection then understates the three kernels by up to the difference (marked)"]
    for msaa in (0, 4):
        S = 4 if msaa else 1
        # every `off` is re-timed before each `on`: key the rows by position
        seq = []
        stream_picks = []
        for i, (label, args) in enumerate(picks):
            stream_picks.append(("%d:%s" % (i, label), args))
        t, shown = time_passes(sc, model, lut, msaa, stream_picks, a.iters, a.warmup)
        mb = W * H * 8 * S / 1e6
        for i, (label, args) in enumerate(picks):
            if args is None:
                continue
            off_dev, off_host = t["%d:off" % (i - 1)]
            on_dev, on_host = t["%d:%s" % (i, label)]
            ring, box = shown["%d:%s" % (i, label)]
            seq.append(f"S = {S}  {label}: off {off_dev:8.1f}   on {on_dev:8.1f}   selection {on_dev - off_dev:+8.1f} us   keys {mb:6.1f} MB, at-5-TB/s {mb / STREAM_TBS:6.1f} us"
                       f"   host {off_host:5.1f} / {on_host:5.1f} us{'   OFF RUN HOST-BOUND: selection is a lower bound' if off_host > 0.8 * off_dev else ''}"
                       f"   ({ring} ring pixels, {box} box pixels)")
        lines += seq
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
